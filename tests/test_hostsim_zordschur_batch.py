"""CPU tier: the batched ComplexF64 reordering (zordschur_batch_, zordschur_batch; csrc/psd_zbord.h) on the TEST-ONLY
serial simulation of the device code (tests/hostsim)."""
import os

import pytest

import batch_common as bcm
import ord_batch_cases as zc
import psd_amd

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")
KNOBS = ("PSD_BATCH_GROUP", "PSD_BORD_W", "PSD_BORD_NMAX", "PSD_ORD_PIPE")


@pytest.fixture
def make_engine(built, monkeypatch):
    return bcm.engine_maker(monkeypatch, KNOBS, lambda: psd_amd.Engine(libpath=LIB), {})


@pytest.mark.parametrize("lr", ["R", "L"])
def test_reference_shape(sim_engine, lr):
    zc.case_reference(sim_engine, zc.Z, lr)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", zc.Z.windows, ids=zc.shape_id)
def test_windows(sim_engine, shape, lr):
    zc.case_windows(sim_engine, zc.Z, shape, lr)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_windows_narrow(make_engine, lr):
    zc.case_windows(make_engine({"PSD_BORD_W": "6"}), zc.Z, zc.Z.narrow, lr, expect_window=6)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", zc.Z.windows, ids=zc.shape_id)
def test_against_serial_single_driver(make_engine, shape, lr):
    # (built with -ffp-contract=off: the same arithmetic gives the same bits)
    assert zc.case_against_serial(make_engine, zc.Z, shape, lr, exact=True) == 0


@pytest.mark.parametrize("shape", [zc.Z.windows[0], zc.Z.windows[3]], ids=zc.shape_id)
def test_independence(sim_engine, shape):
    zc.case_independence(sim_engine, zc.Z, shape)


def test_groups(make_engine):
    zc.case_groups(make_engine, zc.Z)


def test_per_problem_selections(sim_engine):
    zc.case_selections(sim_engine, zc.Z)


def test_one_problem_fails(sim_engine):
    zc.case_one_fails(sim_engine, zc.Z)


def test_fallback_above_the_cap(make_engine):
    zc.case_above_cap(make_engine, zc.Z)


def test_argument_codes(sim_engine):
    zc.case_argument_codes(sim_engine, zc.Z)


def test_python_errors(sim_engine):
    zc.case_python_errors(sim_engine, zc.Z)


def test_device_entry_bits(sim_engine):
    zc.case_dev_abi(sim_engine, zc.Z)


def test_device_entry_bits_grouped(make_engine):
    # (5 problems in groups of 2, 2 and 1: the last group is a partial one)
    zc.case_dev_abi(make_engine({"PSD_BATCH_GROUP": "2"}), zc.Z, launches=3)
