"""CPU tier: the ComplexF64 batched entries (zphessenberg_batch_, zpschur_batch_, zpschur_batch, zpschur_hess_batch_) on
the TEST-ONLY serial simulation of the device code (tests/hostsim).  The simulation's single-problem reduction always
takes the one-launch-per-link form, so the batched reduction is compared with it bit for bit at every shape; the
simulation is built without contraction, so the batched iteration is compared bit for bit with the single call too."""
import os

import pytest

import batch_cases as zc
import psd_amd

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")


@pytest.mark.parametrize("shape", zc.Z.shapes, ids=zc.shape_id)
def test_reduction_bit_for_bit(sim_engine, shape):
    zc.case_reduction_bits(sim_engine, zc.Z, shape)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", zc.Z.shapes, ids=zc.shape_id)
def test_full_decomposition(sim_engine, shape, lr):
    zc.case_full(sim_engine, zc.Z, shape, lr)


@pytest.fixture(scope="module")
def onewave_engine(built):
    """An engine whose single calls chase with the one-wave chain (PSD_C3=0 at psd_create), as the batched kernel does"""
    mp = pytest.MonkeyPatch()
    mp.setenv("PSD_C3", "0")
    try:
        return psd_amd.Engine(libpath=LIB)
    finally:
        mp.undo()


@pytest.mark.parametrize("shape", zc.Z.shapes, ids=zc.shape_id)
def test_iteration_bit_for_bit(sim_engine, onewave_engine, shape):
    zc.case_iteration_bits(sim_engine, zc.Z, onewave_engine, shape)


@pytest.mark.parametrize("hole", zc.Z.holes, ids=lambda h: "n%d_p%d_f%d_i%d" % h)
def test_holes(sim_engine, hole):
    zc.case_holes_z(sim_engine, hole)


def test_one_problem_fails(sim_engine):
    zc.case_one_fails(sim_engine, zc.Z)


def test_flags(sim_engine):
    zc.case_flags(sim_engine, zc.Z)


def test_argument_errors(sim_engine):
    zc.case_argument_errors(sim_engine, zc.Z)


def test_argument_codes_and_device_entry(sim_engine):
    zc.case_abi_codes(sim_engine, zc.Z)


def test_groups(built, monkeypatch):
    monkeypatch.delenv("PSD_BATCH_GROUP", raising=False)

    def make(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return psd_amd.Engine(libpath=LIB)

    zc.case_groups(make, zc.Z)
