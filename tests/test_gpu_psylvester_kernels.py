"""GPU tier (MI355X): ONE launch of the update kernel of the periodic Sylvester walk (psd_syl_update, csrc/psd_sylv.h: the
matrix-core body, its LDS staging, fragment maps and sub-block map) through the diagnostic entry psd_?_syl_update, against
the extended-precision reference of sylv_kernel_cases.py: tile widths on both sides of a wavefront's 16 x 16 fragment and
of a workgroup's 32 x 32 sub-block, every anti-diagonal, both forms of the operator, both orientations."""
import pytest

import sylv_kernel_cases as kc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("trans", [False, True], ids=["S", "SH"])
@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
def test_update_sweep(gpu_engine, cplx, lr, trans):
    """Worst err / bound seen on the MI355X (L and R): Float64 S 0.0238, S^H 0.0257; ComplexF64 S 0.0258, S^H 0.0298."""
    kc.case_update_sweep(gpu_engine, cplx, lr, trans)


def test_update_arguments(gpu_engine):
    kc.case_update_arguments(gpu_engine)
