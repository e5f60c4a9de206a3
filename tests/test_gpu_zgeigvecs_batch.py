"""GPU tier (MI355X): Engine.zgeigvecs_batch — the whole homogeneous back-substitution of a signed ComplexF64 batch in one
launch (psd_zgbev_solve: several columns per wavefront, forward and backward segmented scans), the complex back-transform
and the normalisation — against the numpy prototype and the gates of the single-problem tests (bevec_cases.py), and the
device-resident pipeline behind zgpschur_batch_ and zgordschur_batch_."""
import pytest

import bevec_cases as zg
import psd_amd

pytestmark = pytest.mark.gpu


def test_mixed_batch(gpu_engine):
    zg.case_mixed(gpu_engine, zg.ZG)


def test_batch_independence_bits(gpu_engine, monkeypatch):
    monkeypatch.setenv("PSD_BATCH_GROUP", "3")
    grouped = psd_amd.Engine(device=0)
    monkeypatch.delenv("PSD_BATCH_GROUP")
    zg.case_independence(gpu_engine, zg.ZG, grouped)


@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("shape", zg.ZG.layouts, ids=zg.ZG.layout_id)
def test_lane_layouts(gpu_engine, shape, lr):
    zg.case_layout(gpu_engine, zg.ZG, shape, lr)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_all_false_signature(gpu_engine, lr):
    zg.case_all_false(gpu_engine, zg.ZG, lr)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_depth(gpu_engine, lr):
    zg.case_depth(gpu_engine, zg.ZG, lr)


@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("n", [128, 129])
def test_cap(gpu_engine, n, lr):
    zg.case_cap(gpu_engine, zg.ZG, n, lr)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_zero_and_infinite_eigenvalues(gpu_engine, lr):
    zg.case_zero_infinite(gpu_engine, zg.ZG, lr)


def test_repeated_eigenvalue(gpu_engine):
    zg.case_repeated(gpu_engine, zg.ZG)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_rescaled_columns(gpu_engine, lr):
    zg.case_rescale(gpu_engine, zg.ZG, lr)


def test_all_true_signature(gpu_engine):
    zg.case_all_true_zg(gpu_engine)


def test_skipped_problems(gpu_engine):
    zg.case_skipped(gpu_engine, zg.ZG)


def test_launch_count(gpu_engine):
    zg.case_launch_count(gpu_engine, zg.ZG)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_pipeline_device_resident(gpu_engine, lr):
    zg.case_pipeline_signed(gpu_engine, zg.ZG, lr)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_pipeline_host_forms(gpu_engine, lr):
    zg.case_pipeline_host(gpu_engine, zg.ZG, lr)


def test_gpschur_batch_end_to_end(gpu_engine):
    zg.case_gpschur_batch(gpu_engine, zg.ZG)


def test_errors(gpu_engine):
    zg.case_errors(gpu_engine, zg.ZG, lambda: psd_amd.Engine(device=0))


def test_empty_device_batch(gpu_engine):
    """nb = 0: the shapes and dtypes of a call describe themselves, its stats are those of no problem, no kernel runs"""
    import numpy as np
    import torch

    T = torch.zeros((0, 2, 3, 3), dtype=torch.complex128, device="cuda")
    gpu_engine.eigvecs_batch_stats = gpu_engine.eigvecs_batch_counts = None
    V, a, nvec = gpu_engine.zgeigvecs_batch(T, T.clone(), np.zeros((0, 3), dtype=bool), S=[True, False])
    assert tuple(V.shape) == (0, 2, 3, 0) and V.dtype == torch.complex128 and V.is_cuda
    assert a.shape == (0, 2, 0) and a.dtype == np.complex128
    assert nvec.shape == (0,) and nvec.dtype == np.int32
    st = gpu_engine.eigvecs_batch_stats
    assert isinstance(st, psd_amd.BevecStats) and st.nb == 0 and st.nlaunch == 0
    assert gpu_engine.eigvecs_batch_counts.shape == (0, 3) and gpu_engine.eigvecs_batch_counts.dtype == np.int32
    V1, _, _ = gpu_engine.zgeigvecs_batch(T, T.clone(), [True] * 3, shifted=False)
    assert tuple(V1.shape) == (0, 1, 3, 0)
