"""CPU tier: the ComplexF64 signed batched entries (zgphessenberg_batch_, zgpschur_batch_, zgpschur_batch,
zgpschur_hess_batch_, gpschur_batch) on the TEST-ONLY serial simulation of the device code (tests/hostsim).  The
simulation is built without contraction, so the batched reduction and iteration are compared bit for bit with the single
calls, whose stage 2 then takes the serial form (PSD_HESS_SERIAL=1) and whose iteration runs without trains."""
import os

import pytest

import batch_cases as gc
import psd_amd

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")


@pytest.mark.parametrize("shape", gc.ZG.shapes, ids=gc.shape_id)
def test_reduction(sim_engine, shape):
    gc.case_reduction(sim_engine, gc.ZG, shape)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", gc.ZG.shapes, ids=gc.shape_id)
def test_full_decomposition(sim_engine, shape, lr):
    gc.case_full(sim_engine, gc.ZG, shape, lr)


@pytest.fixture(scope="module")
def single_engine(built):
    """An engine for the single calls with the signed trains off: the iteration the batched kernel runs"""
    eng = psd_amd.Engine(libpath=LIB)
    eng.set_train_g(0)
    return eng


@pytest.mark.parametrize("shape", gc.ZG.shapes, ids=gc.shape_id)
def test_reduction_bit_for_bit(sim_engine, single_engine, shape, monkeypatch):
    monkeypatch.setenv("PSD_HESS_SERIAL", "1")  # (read by the single call at every reduction)
    gc.case_reduction_bits(sim_engine, gc.ZG, shape, single_engine)


@pytest.mark.parametrize("shape", gc.ZG.shapes, ids=gc.shape_id)
def test_iteration_bit_for_bit(sim_engine, single_engine, shape, monkeypatch):
    monkeypatch.setenv("PSD_HESS_SERIAL", "1")
    gc.case_iteration_bits(sim_engine, gc.ZG, single_engine, shape)


def test_all_true_signature(sim_engine):
    gc.case_all_true_zg(sim_engine)


def test_gpschur_batch(sim_engine):
    gc.case_gpschur_batch(sim_engine)


@pytest.mark.parametrize("hole", gc.ZG.holes, ids=gc.hole_id)
def test_holes(sim_engine, hole):
    gc.case_holes_zg(sim_engine, hole)


def test_one_problem_fails(sim_engine):
    gc.case_one_fails(sim_engine, gc.ZG)


def test_flags(sim_engine):
    gc.case_flags(sim_engine, gc.ZG)


def test_argument_errors(sim_engine):
    gc.case_argument_errors(sim_engine, gc.ZG)


def test_argument_codes_and_device_entry(sim_engine):
    gc.case_abi_codes(sim_engine, gc.ZG)


def test_groups(built, monkeypatch):
    monkeypatch.delenv("PSD_BATCH_GROUP", raising=False)

    def make(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return psd_amd.Engine(libpath=LIB)

    gc.case_groups(make, gc.ZG)
