"""CPU tier: the batched signed Float64 reordering (dgordschur_batch_, dgordschur_batch; csrc/psd_gbord.h) on the
TEST-ONLY serial simulation of the device code (tests/hostsim)."""
import os

import pytest

import batch_common as bcm
import ord_batch_cases as gc
import psd_amd

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")
KNOBS = ("PSD_BATCH_GROUP", "PSD_BORD_W", "PSD_BORD_NMAX", "PSD_ORD_PIPE")


@pytest.fixture
def make_engine(built, monkeypatch):
    return bcm.engine_maker(monkeypatch, KNOBS, lambda: psd_amd.Engine(libpath=LIB), {})


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", gc.DG.windows, ids=gc.shape_id)
def test_windows(sim_engine, shape, lr):
    gc.case_windows(sim_engine, gc.DG, shape, lr)


def test_expected_windows():
    # (what rord_lds_bytes gives for the shapes above: the longest span of a window is 25, and at p = 70 the per-factor
    #  scratch leaves room for the narrowest window only)
    assert [gc.expected_window(gc.DG, s[1], s[2]) for s in gc.DG.windows[:4]] == [25, 24, 6, 12]


@pytest.mark.parametrize("lr", ["R", "L"])
def test_windows_narrow(make_engine, lr):
    gc.case_windows(make_engine({"PSD_BORD_W": "6"}), gc.DG, gc.DG.narrow, lr, expect_window=6)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_reference_shape(sim_engine, lr):
    gc.case_reference(sim_engine, gc.DG, lr)


def test_pairs_reference(sim_engine):
    gc.case_pairs_reference(sim_engine)


@pytest.mark.parametrize("shape", [gc.DG.windows[0], gc.DG.windows[3]], ids=gc.shape_id)
def test_independence(sim_engine, shape):
    gc.case_independence(sim_engine, gc.DG, shape)


def test_groups(make_engine):
    gc.case_groups(make_engine, gc.DG)


def test_fallback_above_the_cap(make_engine):
    gc.case_above_cap(make_engine, gc.DG)


def test_all_true_signature(sim_engine):
    gc.case_all_true_dg(sim_engine)


def test_per_problem_selections(sim_engine):
    gc.case_selections(sim_engine, gc.DG)


def test_one_problem_fails(sim_engine):
    gc.case_one_fails(sim_engine, gc.DG)


def test_argument_codes(sim_engine):
    gc.case_argument_codes(sim_engine, gc.DG)


def test_python_errors(sim_engine):
    gc.case_python_errors(sim_engine, gc.DG)


def test_device_entry_bits(sim_engine):
    gc.case_dev_abi(sim_engine, gc.DG)


def test_device_entry_bits_grouped(make_engine):
    # (5 problems in groups of 2, 2 and 1: the last group is a partial one)
    gc.case_dev_abi(make_engine({"PSD_BATCH_GROUP": "2"}), gc.DG, launches=3)
