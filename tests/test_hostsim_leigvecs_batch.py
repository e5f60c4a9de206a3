"""CPU tier: left eigenvectors and eigenvalue condition numbers of many small periodic Schur forms (side="L" / "B" of
Engine.eigvecs_batch / zeigvecs_batch, Engine.eigcond_batch; csrc/psd_lbevec.h) on the TEST-ONLY serial simulation of the
device code, against the numpy prototype of the back-substitution on the flip-adjoint form (lbevec_cases.py)."""
import os

import pytest

import bevec_cases as bc
import lbevec_cases as lc
import psd_amd

_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")
FAMILY = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])


def _make():
    return psd_amd.Engine(libpath=_LIB)


@FAMILY
def test_mixed_batch(sim_engine, cplx):
    lc.case_mixed(sim_engine, cplx)


def test_batch_independence_bits(sim_engine, monkeypatch):
    monkeypatch.setenv("PSD_BATCH_GROUP", "3")
    grouped = _make()
    monkeypatch.delenv("PSD_BATCH_GROUP")
    lc.case_independence(sim_engine, grouped)


@pytest.mark.parametrize("shape", bc.D.layouts, ids=bc.D.layout_id)
def test_factor_layouts(sim_engine, shape):
    lc.case_layout(sim_engine, shape)


def test_orientation_and_schurindex(sim_engine):
    lc.case_orientation(sim_engine)


@FAMILY
@pytest.mark.parametrize("p", [4, 3])
def test_negative_real_eigenvalue(sim_engine, p, cplx):
    lc.case_negative(sim_engine, p, cplx)


def test_zero_eigenvalue(sim_engine):
    lc.case_zero(sim_engine)


def test_rescaled_columns(sim_engine):
    lc.case_rescale(sim_engine)


def test_repeated_eigenvalues(sim_engine):
    lc.case_repeated(sim_engine)


def test_depth(sim_engine):
    lc.case_depth(sim_engine)


def test_above_the_cap(sim_engine):
    lc.case_above_cap(sim_engine)


@FAMILY
def test_condition_formula(sim_engine, cplx):
    lc.case_cond_formula(sim_engine, cplx)


def test_condition_single_factor_is_trsna(sim_engine):
    lc.case_cond_p1(sim_engine)


@FAMILY
def test_condition_first_order_perturbation(sim_engine, cplx):
    lc.case_cond_perturbation(sim_engine, cplx)


def test_condition_extremes(sim_engine):
    lc.case_cond_extremes(sim_engine)


def test_errors(sim_engine):
    lc.case_errors(sim_engine, _make)


def test_entries_and_argument_codes(sim_engine):
    lc.case_abi(sim_engine, _make)
