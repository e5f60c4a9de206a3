"""CPU tier: the Float64 signed batched entries (dgphessenberg_batch_, dgpschur_batch_, dgpschur_batch,
dgpschur_hess_batch_, gpschur_batch(real=True)) on the TEST-ONLY serial simulation of the device code (tests/hostsim).
The simulation is built without contraction, so the batched reduction and iteration are compared bit for bit with the
single calls put into the same form: stage 2 serial (PSD_HESS_SERIAL=1), the iteration without trains (set_train_g(0))
and with the single-wave sweep (PSD_GSCAN=0), which is the form psd_gbqz runs."""
import os

import pytest

import batch_cases as gc
import psd_amd

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")


@pytest.mark.parametrize("shape", gc.DG.shapes, ids=gc.shape_id)
def test_reduction(sim_engine, shape):
    gc.case_reduction(sim_engine, gc.DG, shape)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", gc.DG.shapes, ids=gc.shape_id)
def test_full_decomposition(sim_engine, shape, lr):
    gc.case_full(sim_engine, gc.DG, shape, lr)


@pytest.fixture(scope="module")
def single_engine(built):
    """An engine for the single calls with the signed trains off: the iteration the batched kernel runs"""
    eng = psd_amd.Engine(libpath=LIB)
    eng.set_train_g(0)
    return eng


@pytest.fixture
def single_form(monkeypatch):
    """(read by the single call at every reduction / iteration)"""
    monkeypatch.setenv("PSD_HESS_SERIAL", "1")
    monkeypatch.setenv("PSD_GSCAN", "0")


@pytest.mark.parametrize("shape", gc.DG.shapes, ids=gc.shape_id)
def test_reduction_bit_for_bit(sim_engine, single_engine, shape, single_form):
    gc.case_reduction_bits(sim_engine, gc.DG, shape, single_engine)


@pytest.mark.parametrize("shape", gc.DG.shapes, ids=gc.shape_id)
def test_iteration_bit_for_bit(sim_engine, single_engine, shape, single_form):
    gc.case_iteration_bits(sim_engine, gc.DG, single_engine, shape)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", gc.DG.shapes[:7], ids=gc.shape_id)
def test_full_bit_for_bit(sim_engine, single_engine, shape, lr, single_form):
    gc.case_full_bits(sim_engine, single_engine, shape, lr)


@pytest.mark.parametrize("shape", [gc.DG.shapes[1], gc.DG.shapes[2], gc.DG.shapes[4]], ids=gc.shape_id)
def test_place_independence(sim_engine, shape):
    gc.case_places(sim_engine, shape)


def test_all_true_and_null_signature(sim_engine):
    gc.case_all_true_dg(sim_engine)


def test_flags(sim_engine):
    gc.case_flags(sim_engine, gc.DG)


@pytest.mark.parametrize("hole", gc.DG.holes, ids=gc.hole_id)
def test_holes(sim_engine, hole):
    gc.case_holes_dg(sim_engine, hole)


def test_one_problem_fails(sim_engine):
    gc.case_one_fails(sim_engine, gc.DG)


def test_gpschur_batch_real(sim_engine):
    gc.case_gpschur_batch_real(sim_engine)


def test_argument_errors(sim_engine):
    gc.case_argument_errors(sim_engine, gc.DG)


def test_argument_codes_and_device_entry(sim_engine):
    gc.case_abi_codes(sim_engine, gc.DG)


def test_above_the_cap(built, monkeypatch):
    """the fallback above the order cap, which the simulation (a diagnostic build) lowers through PSD_GB_NMAX"""
    monkeypatch.setenv("PSD_GB_NMAX", "8")
    gc.case_above_cap(psd_amd.Engine(libpath=LIB), gc.DG, 12)


def test_groups(built, monkeypatch):
    monkeypatch.delenv("PSD_BATCH_GROUP", raising=False)

    def make(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return psd_amd.Engine(libpath=LIB)

    gc.case_groups(make, gc.DG)
