"""CPU tier: the batched entries (phessenberg_batch_, pschur_batch_, pschur_batch) on the TEST-ONLY serial simulation of
the device code (tests/hostsim).  The simulation's single-problem reduction always takes the one-launch-per-link form,
so the batched reduction is compared with it bit for bit at every shape."""
import os

import pytest

import batch_cases as bc
import psd_amd


@pytest.mark.parametrize("shape", bc.D.hess_shapes + bc.D.hess_shapes_p3, ids=bc.shape_id)
def test_reduction_bit_for_bit(sim_engine, shape):
    bc.case_reduction_bits(sim_engine, bc.D, shape)


@pytest.mark.parametrize("shape", bc.D.hess_shapes_p3, ids=bc.shape_id)
def test_reduction_factorization(sim_engine, shape):
    bc.case_reduction_close(sim_engine, bc.D, shape)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", bc.D.shapes, ids=bc.shape_id)
def test_full_decomposition(sim_engine, shape, lr):
    bc.case_full_d(sim_engine, shape, lr)


def test_flags(sim_engine):
    bc.case_flags(sim_engine, bc.D)


def test_one_problem_fails(sim_engine):
    bc.case_one_fails(sim_engine, bc.D, single_pattern=True)


def test_argument_errors(sim_engine):
    bc.case_argument_errors(sim_engine, bc.D)


def test_device_entry_and_argument_codes(sim_engine):
    bc.case_dev_abi(sim_engine)


def test_argument_codes(sim_engine):
    bc.case_abi_codes_d(sim_engine)


def test_groups(built, monkeypatch):
    lib = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")
    monkeypatch.delenv("PSD_BATCH_GROUP", raising=False)

    def make(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return psd_amd.Engine(libpath=lib)

    bc.case_groups(make, bc.D)
