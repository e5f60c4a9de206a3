"""CPU tier: ONE launch of the update kernel of the periodic Sylvester walk (psd_syl_update, csrc/psd_sylv.h) through the
diagnostic entry psd_?_syl_update on the TEST-ONLY serial simulation of the device code, against the extended-precision
reference of sylv_kernel_cases.py.  The simulation's update is a serial body of its own: this tier checks the sub-block
map, the operands and the driver's partition, the GPU tier the matrix-core body."""
import pytest

import sylv_kernel_cases as kc


@pytest.mark.parametrize("trans", [False, True], ids=["S", "SH"])
@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
def test_update_sweep(sim_engine, cplx, lr, trans):
    """Worst err / bound seen in the simulation (L and R): Float64 S 0.0276, S^H 0.0315; ComplexF64 S 0.0255, S^H 0.0279."""
    kc.case_update_sweep(sim_engine, cplx, lr, trans)


def test_update_arguments(sim_engine):
    kc.case_update_arguments(sim_engine)
