"""CPU tier: Engine.eigvecs_batch (csrc/psd_bevec.h, driver psd_bevec_host.inl) on the TEST-ONLY serial simulation of the
device code: eigenvectors of many small periodic Schur forms in one call, against the numpy prototype of the
back-substitution and the gates of the single-problem tests (bevec_cases.py)."""
import os

import pytest

import bevec_cases as bc
import psd_amd

_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")


def test_mixed_batch(sim_engine):
    bc.case_mixed(sim_engine, bc.D)


def test_batch_independence_bits(sim_engine, monkeypatch):
    monkeypatch.setenv("PSD_BATCH_GROUP", "3")
    grouped = psd_amd.Engine(libpath=_LIB)
    monkeypatch.delenv("PSD_BATCH_GROUP")
    bc.case_independence(sim_engine, bc.D, grouped)


@pytest.mark.parametrize("shape", bc.D.layouts, ids=bc.D.layout_id)
def test_factor_layouts(sim_engine, shape):
    bc.case_layout(sim_engine, bc.D, shape)


def test_depth(sim_engine):
    bc.case_depth(sim_engine, bc.D)


def test_negative_eigenvalue_even_period(sim_engine):
    bc.case_special_negative(sim_engine)


def test_repeated_eigenvalues(sim_engine):
    bc.case_special_repeated(sim_engine, bc.D)


def test_zero_eigenvalue(sim_engine):
    bc.case_special_zero(sim_engine, bc.D)


def test_rescaled_columns(sim_engine):
    bc.case_special_rescale(sim_engine, bc.D)


def test_skipped_problems(sim_engine):
    bc.case_skipped(sim_engine, bc.D)


def test_launch_count(sim_engine):
    bc.case_launch_count(sim_engine, bc.D)


def test_above_the_cap(sim_engine):
    bc.case_above_cap(sim_engine, bc.D)


def test_errors(sim_engine):
    bc.case_errors(sim_engine, bc.D, lambda: psd_amd.Engine(libpath=_LIB))


def test_device_entry_and_argument_codes(sim_engine):
    bc.case_dev_abi(sim_engine, bc.D)
