"""CPU tier: periodic Sylvester solves and the condition of an invariant periodic subspace for many small periodic Schur
forms (Engine.psylvester_batch, Engine.subspacecond_batch; csrc/psd_bsylv.h) on the TEST-ONLY serial simulation of the
device code, against the dense Kronecker reference of bsylv_cases.py."""
import os

import pytest

import bsylv_cases as sc
import psd_amd
from batch_common import engine_maker

_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")
FAMILY = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
LR = pytest.mark.parametrize("lr", ["L", "R"])
ALL = pytest.mark.parametrize("k", range(len(sc.PROBLEMS)), ids=sc.IDS)
P1 = pytest.mark.parametrize("k", [k for k, pr in enumerate(sc.PROBLEMS) if pr[1] == 1],
                             ids=[sc.IDS[k] for k, pr in enumerate(sc.PROBLEMS) if pr[1] == 1])
KNOBS = ("PSD_BSYL_NMAX", "PSD_BATCH_GROUP")


def _make():
    return psd_amd.Engine(libpath=_LIB)


@pytest.fixture
def make_engine(monkeypatch):
    return engine_maker(monkeypatch, KNOBS, _make, {})


@LR
@ALL
def test_reference_inputs(k, lr):
    sc.case_reference_inputs(k, lr)


@LR
@ALL
def test_solve_residual(sim_engine, k, lr):
    sc.case_residual(sim_engine, k, lr)


@LR
@ALL
def test_transposed_solve(sim_engine, k, lr):
    sc.case_transposed(sim_engine, k, lr)


@LR
@ALL
def test_s_x_sep_against_reference(sim_engine, k, lr):
    sc.case_reference(sim_engine, k, lr)


@LR
@P1
def test_single_factor_is_trsen(sim_engine, k, lr):
    sc.case_trsen(sim_engine, k, lr)


@FAMILY
def test_mixed_batch(sim_engine, cplx):
    sc.case_mixed(sim_engine, cplx)


@FAMILY
def test_batch_independence_bits(sim_engine, make_engine, cplx):
    sc.case_independence(sim_engine, make_engine({"PSD_BATCH_GROUP": "3"}), cplx)


@FAMILY
def test_singular_problem(sim_engine, cplx):
    sc.case_singular(sim_engine, cplx)


def test_errors_and_cap(sim_engine, make_engine):
    sc.case_errors(sim_engine, make_engine)


@FAMILY
def test_launch_count(sim_engine, cplx):
    sc.case_launch_count(sim_engine, cplx)
