"""CPU tier: the batched signed ComplexF64 reordering (zgordschur_batch_, zgordschur_batch; csrc/psd_zgbord.h) on the
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
def test_reference_shape(sim_engine, lr):
    gc.case_reference(sim_engine, gc.ZG, lr)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", gc.ZG.windows, ids=gc.shape_id)
def test_windows(sim_engine, shape, lr):
    gc.case_windows(sim_engine, gc.ZG, shape, lr)


def test_expected_windows():
    # (what zgord_lds_bytes gives for the shapes above: the narrow window near the LDS limit is 10 wide)
    assert [gc.expected_window(gc.ZG, s[1], s[2]) for s in gc.ZG.windows[:4]] == [32, 20, 10, 12]


@pytest.mark.parametrize("lr", ["R", "L"])
def test_windows_narrow(make_engine, lr):
    gc.case_windows(make_engine({"PSD_BORD_W": "6"}), gc.ZG, gc.ZG.narrow, lr, expect_window=6)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", gc.ZG.windows, ids=gc.shape_id)
def test_against_serial_single_driver(make_engine, shape, lr):
    # (built with -ffp-contract=off: the same arithmetic gives the same bits)
    assert gc.case_against_serial(make_engine, gc.ZG, shape, lr, exact=True) == 0


@pytest.mark.parametrize("shape", [gc.ZG.windows[0], gc.ZG.windows[3]], ids=gc.shape_id)
def test_independence(sim_engine, shape):
    gc.case_independence(sim_engine, gc.ZG, shape)


def test_groups(make_engine):
    gc.case_groups(make_engine, gc.ZG)


def test_all_true_signature(sim_engine):
    gc.case_all_true_zg(sim_engine)


def test_per_problem_selections(sim_engine):
    gc.case_selections(sim_engine, gc.ZG)


def test_one_problem_fails(sim_engine):
    gc.case_one_fails(sim_engine, gc.ZG)


def test_fallback_above_the_cap(make_engine):
    gc.case_above_cap(make_engine, gc.ZG)


def test_argument_codes(sim_engine):
    gc.case_argument_codes(sim_engine, gc.ZG)


def test_python_errors(sim_engine):
    gc.case_python_errors(sim_engine, gc.ZG)


def test_device_entry_bits(sim_engine):
    gc.case_dev_abi(sim_engine, gc.ZG)


def test_device_entry_bits_grouped(make_engine):
    # (5 problems in groups of 2, 2 and 1: the last group is a partial one)
    gc.case_dev_abi(make_engine({"PSD_BATCH_GROUP": "2"}), gc.ZG, launches=3)
