"""CPU tier: Engine.zeigvecs_batch (csrc/psd_zbevec.h, driver psd_zbevec_host.inl) on the TEST-ONLY serial simulation of
the device code: eigenvectors of many small ComplexF64 periodic Schur forms in one call, against the numpy prototype of the
back-substitution and the gates of the single-problem tests (zbevec_cases.py)."""
import os

import pytest

import psd_amd
import zbevec_cases as zc

_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")


def test_mixed_batch(sim_engine):
    zc.case_mixed(sim_engine)


def test_batch_independence_bits(sim_engine, monkeypatch):
    monkeypatch.setenv("PSD_BATCH_GROUP", "3")
    grouped = psd_amd.Engine(libpath=_LIB)
    monkeypatch.delenv("PSD_BATCH_GROUP")
    zc.case_independence(sim_engine, grouped)


@pytest.mark.parametrize("shape", zc.LAYOUTS, ids=zc.layout_id)
def test_factor_layouts(sim_engine, shape):
    zc.case_layout(sim_engine, shape)


def test_depth(sim_engine):
    zc.case_depth(sim_engine)


def test_repeated_eigenvalues(sim_engine):
    zc.case_special_repeated(sim_engine)


def test_zero_eigenvalue(sim_engine):
    zc.case_special_zero(sim_engine)


def test_rescaled_columns(sim_engine):
    zc.case_special_rescale(sim_engine)


def test_skipped_problems(sim_engine):
    zc.case_skipped(sim_engine)


def test_launch_count(sim_engine):
    zc.case_launch_count(sim_engine)


def test_above_the_cap(sim_engine):
    zc.case_above_cap(sim_engine)


def test_errors(sim_engine):
    zc.case_errors(sim_engine, lambda: psd_amd.Engine(libpath=_LIB))


def test_device_entry_and_argument_codes(sim_engine):
    zc.case_dev_abi(sim_engine)
