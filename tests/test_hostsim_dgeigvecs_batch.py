"""CPU tier: Engine.dgeigvecs_batch (csrc/psd_gbevec.h, driver psd_gbevec_host.inl) on the TEST-ONLY serial simulation of
the device code: geigvecs of many small signed Float64 periodic Schur forms in one call, against the numpy prototype of the
cyclic system, the single geigvecs (the same bits where the sums run in the same order) and the gates of the
single-problem tests (bevec_cases.py)."""
import os

import pytest

import bevec_cases as dg
import psd_amd

_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")


def test_mixed_batch(sim_engine):
    dg.case_mixed(sim_engine, dg.DG)


def test_batch_independence_bits(sim_engine, monkeypatch):
    monkeypatch.setenv("PSD_BATCH_GROUP", "3")
    grouped = psd_amd.Engine(libpath=_LIB)
    monkeypatch.delenv("PSD_BATCH_GROUP")
    dg.case_independence(sim_engine, dg.DG, grouped)


@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("shape", dg.DG.layouts, ids=dg.DG.layout_id)
def test_lane_layouts(sim_engine, shape, lr):
    dg.case_layout(sim_engine, dg.DG, shape, lr)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_all_false_signature(sim_engine, lr):
    dg.case_all_false(sim_engine, dg.DG, lr)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_depth(sim_engine, lr):
    dg.case_depth(sim_engine, dg.DG, lr)


@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("n", [128, 129])
def test_cap(sim_engine, n, lr):
    dg.case_cap(sim_engine, dg.DG, n, lr)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_zero_and_infinite_eigenvalues(sim_engine, lr):
    dg.case_zero_infinite(sim_engine, dg.DG, lr)


def test_repeated_eigenvalue(sim_engine):
    dg.case_repeated(sim_engine, dg.DG)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_rescaled_columns(sim_engine, lr):
    dg.case_rescale(sim_engine, dg.DG, lr)


def test_all_true_signature(sim_engine):
    dg.case_all_true_dg(sim_engine)


def test_skipped_problems(sim_engine):
    dg.case_skipped(sim_engine, dg.DG)


def test_launch_count(sim_engine):
    dg.case_launch_count(sim_engine, dg.DG)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_pipeline_host_forms(sim_engine, lr):
    dg.case_pipeline_host(sim_engine, dg.DG, lr)


def test_gpschur_batch_end_to_end(sim_engine):
    dg.case_gpschur_batch(sim_engine, dg.DG)


def test_errors(sim_engine):
    dg.case_errors(sim_engine, dg.DG, lambda: psd_amd.Engine(libpath=_LIB))


def test_device_entry_and_argument_codes(sim_engine):
    dg.case_dev_abi(sim_engine, dg.DG)


def test_zz_figures():
    """the worst figures the cases above measured (run with -s to read them)"""
    dg.print_figures()
