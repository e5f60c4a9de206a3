"""CPU tier: Engine.zgeigvecs_batch (csrc/psd_zgbevec.h, driver psd_zgbevec_host.inl) on the TEST-ONLY serial simulation
of the device code: geigvecs of many small signed ComplexF64 periodic Schur forms in one call, against the numpy prototype
of the cyclic system and the gates of the single-problem tests (bevec_cases.py)."""
import os

import pytest

import bevec_cases as zg
import psd_amd

_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")


def test_mixed_batch(sim_engine):
    zg.case_mixed(sim_engine, zg.ZG)


def test_batch_independence_bits(sim_engine, monkeypatch):
    monkeypatch.setenv("PSD_BATCH_GROUP", "3")
    grouped = psd_amd.Engine(libpath=_LIB)
    monkeypatch.delenv("PSD_BATCH_GROUP")
    zg.case_independence(sim_engine, zg.ZG, grouped)


@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("shape", zg.ZG.layouts, ids=zg.ZG.layout_id)
def test_lane_layouts(sim_engine, shape, lr):
    zg.case_layout(sim_engine, zg.ZG, shape, lr)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_all_false_signature(sim_engine, lr):
    zg.case_all_false(sim_engine, zg.ZG, lr)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_depth(sim_engine, lr):
    zg.case_depth(sim_engine, zg.ZG, lr)


@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("n", [128, 129])
def test_cap(sim_engine, n, lr):
    zg.case_cap(sim_engine, zg.ZG, n, lr)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_zero_and_infinite_eigenvalues(sim_engine, lr):
    zg.case_zero_infinite(sim_engine, zg.ZG, lr)


def test_repeated_eigenvalue(sim_engine):
    zg.case_repeated(sim_engine, zg.ZG)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_rescaled_columns(sim_engine, lr):
    zg.case_rescale(sim_engine, zg.ZG, lr)


def test_all_true_signature(sim_engine):
    zg.case_all_true_zg(sim_engine)


def test_skipped_problems(sim_engine):
    zg.case_skipped(sim_engine, zg.ZG)


def test_launch_count(sim_engine):
    zg.case_launch_count(sim_engine, zg.ZG)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_pipeline_host_forms(sim_engine, lr):
    zg.case_pipeline_host(sim_engine, zg.ZG, lr)


def test_gpschur_batch_end_to_end(sim_engine):
    zg.case_gpschur_batch(sim_engine, zg.ZG)


def test_errors(sim_engine):
    zg.case_errors(sim_engine, zg.ZG, lambda: psd_amd.Engine(libpath=_LIB))


def test_device_entry_and_argument_codes(sim_engine):
    zg.case_dev_abi(sim_engine, zg.ZG)
