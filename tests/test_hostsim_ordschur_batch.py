"""CPU tier: the batched reordering (ordschur_batch_, ordschur_batch; csrc/psd_bord.h) on the TEST-ONLY serial simulation of
the device code (tests/hostsim)."""
import os

import pytest

import ord_batch_cases as oc
import psd_amd

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")
KNOBS = ("PSD_BATCH_GROUP", "PSD_BORD_W", "PSD_BORD_NMAX")


@pytest.fixture
def make_engine(built, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)

    def make(env):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return psd_amd.Engine(libpath=LIB)

    return make


@pytest.mark.parametrize("lr", ["R", "L"])
def test_reference_shape(sim_engine, lr):
    oc.case_reference(sim_engine, lr)


def test_reference_pairs(sim_engine):
    oc.case_pairs(sim_engine)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", oc.WINDOW_SHAPES, ids=oc.shape_id)
def test_windows(sim_engine, shape, lr):
    oc.case_windows(sim_engine, shape, lr)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_windows_narrow(make_engine, lr):
    oc.case_windows(make_engine({"PSD_BORD_W": "6"}), oc.NARROW_SHAPE, lr, expect_window=6)


@pytest.mark.parametrize("shape", [oc.WINDOW_SHAPES[0], oc.WINDOW_SHAPES[3]], ids=oc.shape_id)
def test_independence(sim_engine, shape):
    oc.case_independence(sim_engine, shape)


def test_groups(make_engine):
    oc.case_groups(make_engine)


def test_per_problem_selections(sim_engine):
    oc.case_selections(sim_engine)


def test_one_problem_fails(sim_engine):
    oc.case_one_fails(sim_engine)


def test_fallback_above_the_cap(make_engine):
    oc.case_above_cap(make_engine)


def test_argument_codes(sim_engine):
    oc.case_argument_codes(sim_engine)


def test_python_errors(sim_engine):
    oc.case_python_errors(sim_engine)


def test_device_entry_bits(sim_engine):
    oc.case_dev_abi(sim_engine)


def test_device_entry_bits_grouped(make_engine):
    # (5 problems in groups of 2, 2 and 1: the last group is a partial one)
    oc.case_dev_abi(make_engine({"PSD_BATCH_GROUP": "2"}), launches=3)
