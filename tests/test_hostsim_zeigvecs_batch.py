"""CPU tier: Engine.zeigvecs_batch (csrc/psd_zbevec.h, driver psd_zbevec_host.inl) on the TEST-ONLY serial simulation of
the device code: eigenvectors of many small ComplexF64 periodic Schur forms in one call, against the numpy prototype of the
back-substitution and the gates of the single-problem tests (bevec_cases.py)."""
import os

import pytest

import bevec_cases as zc
import psd_amd

_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")


def test_mixed_batch(sim_engine):
    zc.case_mixed(sim_engine, zc.Z)


def test_batch_independence_bits(sim_engine, monkeypatch):
    monkeypatch.setenv("PSD_BATCH_GROUP", "3")
    grouped = psd_amd.Engine(libpath=_LIB)
    monkeypatch.delenv("PSD_BATCH_GROUP")
    zc.case_independence(sim_engine, zc.Z, grouped)


@pytest.mark.parametrize("shape", zc.Z.layouts, ids=zc.Z.layout_id)
def test_factor_layouts(sim_engine, shape):
    zc.case_layout(sim_engine, zc.Z, shape)


def test_depth(sim_engine):
    zc.case_depth(sim_engine, zc.Z)


def test_repeated_eigenvalues(sim_engine):
    zc.case_special_repeated(sim_engine, zc.Z)


def test_zero_eigenvalue(sim_engine):
    zc.case_special_zero(sim_engine, zc.Z)


def test_rescaled_columns(sim_engine):
    zc.case_special_rescale(sim_engine, zc.Z)


def test_skipped_problems(sim_engine):
    zc.case_skipped(sim_engine, zc.Z)


def test_launch_count(sim_engine):
    zc.case_launch_count(sim_engine, zc.Z)


def test_above_the_cap(sim_engine):
    zc.case_above_cap(sim_engine, zc.Z)


def test_errors(sim_engine):
    zc.case_errors(sim_engine, zc.Z, lambda: psd_amd.Engine(libpath=_LIB))


def test_device_entry_and_argument_codes(sim_engine):
    zc.case_dev_abi(sim_engine, zc.Z)
