"""GPU tier (MI355X): left eigenvectors and eigenvalue condition numbers of many small periodic Schur forms — the
flip-adjoint launch (psd_lbev_flip) in front of the batched back-substitution, the column reversal behind it and
psd_bev_cond — against the numpy prototype on the flip-adjoint form (lbevec_cases.py), and the device-resident pipeline
behind pschur_batch_ / zpschur_batch_."""
import pytest

import bevec_cases as bc
import lbevec_cases as lc
import psd_amd

pytestmark = pytest.mark.gpu
FAMILY = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])


def _make():
    return psd_amd.Engine(device=0)


@FAMILY
def test_mixed_batch(gpu_engine, cplx):
    lc.case_mixed(gpu_engine, cplx)


def test_batch_independence_bits(gpu_engine, monkeypatch):
    monkeypatch.setenv("PSD_BATCH_GROUP", "3")
    grouped = _make()
    monkeypatch.delenv("PSD_BATCH_GROUP")
    lc.case_independence(gpu_engine, grouped)


@pytest.mark.parametrize("shape", bc.D.layouts, ids=bc.D.layout_id)
def test_factor_layouts(gpu_engine, shape):
    lc.case_layout(gpu_engine, shape)


def test_orientation_and_schurindex(gpu_engine):
    lc.case_orientation(gpu_engine)


@FAMILY
@pytest.mark.parametrize("p", [4, 3])
def test_negative_real_eigenvalue(gpu_engine, p, cplx):
    lc.case_negative(gpu_engine, p, cplx)


def test_zero_eigenvalue(gpu_engine):
    lc.case_zero(gpu_engine)


def test_rescaled_columns(gpu_engine):
    lc.case_rescale(gpu_engine)


def test_repeated_eigenvalues(gpu_engine):
    lc.case_repeated(gpu_engine)


def test_depth(gpu_engine):
    lc.case_depth(gpu_engine)


def test_above_the_cap(gpu_engine):
    lc.case_above_cap(gpu_engine)


@FAMILY
def test_condition_formula(gpu_engine, cplx):
    lc.case_cond_formula(gpu_engine, cplx)


def test_condition_single_factor_is_trsna(gpu_engine):
    lc.case_cond_p1(gpu_engine)


@FAMILY
def test_condition_first_order_perturbation(gpu_engine, cplx):
    lc.case_cond_perturbation(gpu_engine, cplx)


def test_condition_extremes(gpu_engine):
    lc.case_cond_extremes(gpu_engine)


def test_errors(gpu_engine):
    lc.case_errors(gpu_engine, _make)


@FAMILY
@pytest.mark.parametrize("lr", ["R", "L"])
def test_pipeline_device_resident(gpu_engine, lr, cplx):
    lc.case_pipeline(gpu_engine, lr, cplx)


def test_empty_device_batch(gpu_engine):
    lc.case_empty_device(gpu_engine)
