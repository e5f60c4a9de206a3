"""CPU tier: the scalar device routines one call at a time on the TEST-ONLY serial simulation, through the diagnostic entry
psd_diag_scalar, against exact rational arithmetic (scalar_cases).  The simulation replaces the three raw fast forms by
their IEEE counterparts, so those meet their gates with room here; what this tier pins is the logic around them: the
range guards, the dlarfg / zlartg rescaling paths, the tau = 0 exits and the sign rules."""
import pytest

import scalar_cases as sc


@pytest.mark.parametrize("op", sc.OP_NAMES)
def test_scalar_op(sim_engine, op):
    sc.check_op(sim_engine, op)


def test_argument_codes(sim_engine):
    sc.check_argument_codes(sim_engine)
