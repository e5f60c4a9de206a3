"""CPU tier: the batched verifier (checkpsd_batch; csrc/psd_bcheck.h, psd_bcheck_host.inl) on the TEST-ONLY serial
simulation of the device code (tests/hostsim): the host driver, the (a, b) rule, the sub-diagonal rule, grouping, the
fallback above the cap and the ABI codes; the matrix-core kernel itself has a plain-loop stand-in there."""
import os

import pytest

import check_batch_cases as cc
import psd_amd

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")
LRS = ["R", "L"]


@pytest.fixture
def make_engine(built, sim_engine, monkeypatch):
    made = {}

    def make(env):
        if not env:
            return sim_engine
        key = tuple(sorted(env.items()))
        if key not in made:
            for k in cc.KNOBS:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            made[key] = psd_amd.Engine(libpath=LIB)
        return made[key]

    return make


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=cc.shape_id)
@pytest.mark.parametrize("fam", cc.FAMILIES, ids=repr)
def test_against_reference(sim_engine, fam, shape, lr):
    cc.case_reference(sim_engine, fam, shape, lr)


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=cc.shape_id)
@pytest.mark.parametrize("fam", cc.FAMILIES, ids=repr)
def test_against_single_entry(sim_engine, fam, shape, lr):
    cc.case_single(sim_engine, fam, shape, lr)


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("fam", cc.FAMILIES, ids=repr)
def test_says_no_to_the_right_problem(sim_engine, fam, lr):
    cc.case_says_no(sim_engine, fam, lr)


@pytest.mark.parametrize("fam", [cc.Z, cc.ZG], ids=repr)
def test_nan_fails(sim_engine, fam):
    cc.case_nan(sim_engine, fam, "R")


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("fam", cc.FAMILIES, ids=repr)
def test_independence(make_engine, fam, lr):
    cc.case_independence(make_engine, fam, lr)


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("fam", cc.FAMILIES, ids=repr)
def test_fallback_above_a_lowered_cap(make_engine, fam, lr):
    cc.case_fallback(make_engine, fam, lr)


@pytest.mark.parametrize("fam", [cc.D, cc.Z], ids=repr)
def test_above_the_default_cap(sim_engine, fam):
    cc.case_above_default_cap(sim_engine, fam)


def test_cap_knob_only_lowers(make_engine):
    cc.case_cap_knob(make_engine)


@pytest.mark.parametrize("fam", cc.FAMILIES, ids=repr)
def test_argument_codes(sim_engine, fam):
    cc.case_abi(sim_engine, fam)


@pytest.mark.parametrize("fam", [cc.D, cc.ZG], ids=repr)
def test_argument_codes_device_entry(sim_engine, fam):
    cc.case_abi(sim_engine, fam, dev=cc.host_dev)


def test_python_errors(sim_engine):
    cc.case_python_errors(sim_engine)


@pytest.mark.parametrize("n", [3, 17, 64])
def test_zcheckpsd_dev(sim_engine, n):
    cc.case_zcheckpsd_dev(sim_engine, n, cc.host_dev)
