"""GPU tier (MI355X): Engine.eigvecs_batch — the whole back-substitution of a batch in one launch (psd_bev_solve: several
columns per wavefront), the batched back-transform and normalisation — against the numpy prototype and the gates of the
single-problem tests (bevec_cases.py), and the device-resident pipeline behind pschur_batch_."""
import pytest

import bevec_cases as bc
import psd_amd

pytestmark = pytest.mark.gpu


def test_mixed_batch(gpu_engine):
    bc.case_mixed(gpu_engine, bc.D)


def test_batch_independence_bits(gpu_engine, monkeypatch):
    monkeypatch.setenv("PSD_BATCH_GROUP", "3")
    grouped = psd_amd.Engine(device=0)
    monkeypatch.delenv("PSD_BATCH_GROUP")
    bc.case_independence(gpu_engine, bc.D, grouped)


@pytest.mark.parametrize("shape", bc.D.layouts, ids=bc.D.layout_id)
def test_factor_layouts(gpu_engine, shape):
    bc.case_layout(gpu_engine, bc.D, shape)


def test_depth(gpu_engine):
    bc.case_depth(gpu_engine, bc.D)


def test_negative_eigenvalue_even_period(gpu_engine):
    bc.case_special_negative(gpu_engine)


def test_repeated_eigenvalues(gpu_engine):
    bc.case_special_repeated(gpu_engine, bc.D)


def test_zero_eigenvalue(gpu_engine):
    bc.case_special_zero(gpu_engine, bc.D)


def test_rescaled_columns(gpu_engine):
    bc.case_special_rescale(gpu_engine, bc.D)


def test_skipped_problems(gpu_engine):
    bc.case_skipped(gpu_engine, bc.D)


def test_launch_count(gpu_engine):
    bc.case_launch_count(gpu_engine, bc.D)


def test_above_the_cap(gpu_engine):
    bc.case_above_cap(gpu_engine, bc.D)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_pipeline_device_resident(gpu_engine, lr):
    bc.case_pipeline(gpu_engine, bc.D, lr)


def test_errors(gpu_engine):
    bc.case_errors(gpu_engine, bc.D, lambda: psd_amd.Engine(device=0))


def test_empty_device_batch(gpu_engine):
    """nb = 0: the shapes and dtypes of a call describe themselves, its stats are those of no problem, no kernel runs"""
    import numpy as np
    import torch

    T = torch.zeros((0, 2, 3, 3), dtype=torch.float64, device="cuda")
    gpu_engine.eigvecs_batch_stats = gpu_engine.eigvecs_batch_counts = None
    V, nvec = gpu_engine.eigvecs_batch(T, T.clone(), np.zeros((0, 3)), np.zeros((0, 3), dtype=bool))
    assert tuple(V.shape) == (0, 2, 3, 0) and V.dtype == torch.complex128 and V.is_cuda
    assert nvec.shape == (0,) and nvec.dtype == np.int32
    st = gpu_engine.eigvecs_batch_stats
    assert isinstance(st, psd_amd.BevecStats) and st.nb == 0 and st.nlaunch == 0
    assert gpu_engine.eigvecs_batch_counts.shape == (0, 3) and gpu_engine.eigvecs_batch_counts.dtype == np.int32
    V1, _ = gpu_engine.eigvecs_batch(T, T.clone(), np.zeros((0, 3)), [True] * 3, shifted=False)
    assert tuple(V1.shape) == (0, 1, 3, 0)
