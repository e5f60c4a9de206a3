"""GPU tier (MI355X): the batched reordering — one wavefront per problem, a group in one launch of psd_bord — against
the single calls on the same engine and the oracle, the fallback above PSD_BORD_NMAX, and the device-resident chain
pschur_batch_ -> ordschur_batch_ -> eigvecs_batch."""
import pytest

import ord_batch_cases as oc
import psd_amd

pytestmark = pytest.mark.gpu

KNOBS = ("PSD_BATCH_GROUP", "PSD_BORD_W", "PSD_BORD_NMAX")


@pytest.fixture
def make_engine(gpu_engine, monkeypatch):
    def make(env):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return psd_amd.Engine(device=0) if env else gpu_engine

    return make


@pytest.mark.parametrize("lr", ["R", "L"])
def test_reference_shape(gpu_engine, lr):
    oc.case_reference(gpu_engine, lr)


def test_reference_pairs(gpu_engine):
    oc.case_pairs(gpu_engine)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", oc.WINDOW_SHAPES, ids=oc.shape_id)
def test_windows(gpu_engine, shape, lr):
    oc.case_windows(gpu_engine, shape, lr)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_windows_narrow(make_engine, lr):
    oc.case_windows(make_engine({"PSD_BORD_W": "6"}), oc.NARROW_SHAPE, lr, expect_window=6)


@pytest.mark.parametrize("shape", [oc.WINDOW_SHAPES[0], oc.WINDOW_SHAPES[3]], ids=oc.shape_id)
def test_independence(gpu_engine, shape):
    oc.case_independence(gpu_engine, shape)


def test_groups(make_engine):
    oc.case_groups(make_engine)


def test_per_problem_selections(gpu_engine):
    oc.case_selections(gpu_engine)


def test_one_problem_fails(gpu_engine):
    oc.case_one_fails(gpu_engine)


def test_fallback_above_the_cap(make_engine):
    oc.case_above_cap(make_engine)


def test_argument_codes(gpu_engine):
    oc.case_argument_codes(gpu_engine)


def test_python_errors(gpu_engine):
    oc.case_python_errors(gpu_engine)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_device_resident_chain(gpu_engine, lr):
    oc.case_device_chain(gpu_engine, lr)
