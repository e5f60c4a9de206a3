"""GPU tier (MI355X): the scalar device routines one call at a time through the diagnostic entry psd_diag_scalar, against
exact rational arithmetic (scalar_cases): the hardware reciprocal / reciprocal-root seeds with their Newton steps, the
frexp / ldexp builtins and the contracted arithmetic of the fast paths, over the whole range their guards admit."""
import pytest

import scalar_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op", sc.OP_NAMES)
def test_scalar_op(gpu_engine, op):
    sc.check_op(gpu_engine, op)


def test_argument_codes(gpu_engine):
    sc.check_argument_codes(gpu_engine)
