"""GPU tier (MI355X): Engine.eigvecs_batch — the whole back-substitution of a batch in one launch (psd_bev_solve: several
columns per wavefront), the batched back-transform and normalisation — against the numpy prototype and the gates of the
single-problem tests (bevec_cases.py), and the device-resident pipeline behind pschur_batch_."""
import pytest

import bevec_cases as bc
import psd_amd

pytestmark = pytest.mark.gpu


def test_mixed_batch(gpu_engine):
    bc.case_mixed(gpu_engine)


def test_batch_independence_bits(gpu_engine, monkeypatch):
    monkeypatch.setenv("PSD_BATCH_GROUP", "3")
    grouped = psd_amd.Engine(device=0)
    monkeypatch.delenv("PSD_BATCH_GROUP")
    bc.case_independence(gpu_engine, grouped)


@pytest.mark.parametrize("shape", bc.LAYOUTS, ids=bc.layout_id)
def test_factor_layouts(gpu_engine, shape):
    bc.case_layout(gpu_engine, shape)


def test_depth(gpu_engine):
    bc.case_depth(gpu_engine)


def test_negative_eigenvalue_even_period(gpu_engine):
    bc.case_special_negative(gpu_engine)


def test_repeated_eigenvalues(gpu_engine):
    bc.case_special_repeated(gpu_engine)


def test_zero_eigenvalue(gpu_engine):
    bc.case_special_zero(gpu_engine)


def test_rescaled_columns(gpu_engine):
    bc.case_special_rescale(gpu_engine)


def test_skipped_problems(gpu_engine):
    bc.case_skipped(gpu_engine)


def test_launch_count(gpu_engine):
    bc.case_launch_count(gpu_engine)


def test_above_the_cap(gpu_engine):
    bc.case_above_cap(gpu_engine)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_pipeline_device_resident(gpu_engine, lr):
    bc.case_pipeline(gpu_engine, lr)


def test_errors(gpu_engine):
    bc.case_errors(gpu_engine, lambda: psd_amd.Engine(device=0))
