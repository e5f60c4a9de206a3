"""GPU tier (MI355X): periodic Sylvester solves and the condition of an invariant periodic subspace for many small
periodic Schur forms — psd_bsyl_solve, psd_bsyl_norms and psd_bsyl_est_step (csrc/psd_bsylv.h) — against the dense
Kronecker reference of bsylv_cases.py, and the device-resident entries behind pschur_batch_ / ordschur_batch_."""
import pytest

import bsylv_cases as sc
import psd_amd
from batch_common import engine_maker

pytestmark = pytest.mark.gpu
FAMILY = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
LR = pytest.mark.parametrize("lr", ["L", "R"])
ALL = pytest.mark.parametrize("k", range(len(sc.PROBLEMS)), ids=sc.IDS)
P1 = pytest.mark.parametrize("k", [k for k, pr in enumerate(sc.PROBLEMS) if pr[1] == 1],
                             ids=[sc.IDS[k] for k, pr in enumerate(sc.PROBLEMS) if pr[1] == 1])
KNOBS = ("PSD_BSYL_NMAX", "PSD_BATCH_GROUP")


def _make():
    return psd_amd.Engine(device=0)


@pytest.fixture
def make_engine(monkeypatch):
    return engine_maker(monkeypatch, KNOBS, _make, {})


@LR
@ALL
def test_solve_residual(gpu_engine, k, lr):
    sc.case_residual(gpu_engine, k, lr)


@LR
@ALL
def test_transposed_solve(gpu_engine, k, lr):
    sc.case_transposed(gpu_engine, k, lr)


@LR
@ALL
def test_s_x_sep_against_reference(gpu_engine, k, lr):
    sc.case_reference(gpu_engine, k, lr)


@LR
@P1
def test_single_factor_is_trsen(gpu_engine, k, lr):
    sc.case_trsen(gpu_engine, k, lr)


@FAMILY
def test_mixed_batch(gpu_engine, cplx):
    sc.case_mixed(gpu_engine, cplx)


@FAMILY
def test_batch_independence_bits(gpu_engine, make_engine, cplx):
    sc.case_independence(gpu_engine, make_engine({"PSD_BATCH_GROUP": "3"}), cplx)


@FAMILY
def test_singular_problem(gpu_engine, cplx):
    sc.case_singular(gpu_engine, cplx)


def test_errors_and_cap(gpu_engine, make_engine):
    sc.case_errors(gpu_engine, make_engine)


@FAMILY
def test_launch_count(gpu_engine, cplx):
    sc.case_launch_count(gpu_engine, cplx)


@FAMILY
@LR
def test_device_entry(gpu_engine, lr, cplx):
    sc.case_device(gpu_engine, lr, cplx)


def test_empty_and_wrong_device_tensors(gpu_engine):
    sc.case_empty_device(gpu_engine)
