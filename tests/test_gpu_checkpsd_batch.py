"""GPU tier (MI355X): the batched verifier — a workgroup per (problem, factor), a group in one launch of psd_bck_check on
the matrix cores — against the numpy restatement of the reference and the single entry on the same device, its
verdicts on damaged inputs, its independence of the batch (bit for bit), the fallback above PSD_BCK_NMAX, the ABI, the
complex twin of the single device entry, and the device-resident chain *pschur_batch_ -> checkpsd_batch."""
import pytest

import check_batch_cases as cc
import psd_amd
import psdtest as pt

pytestmark = pytest.mark.gpu

LRS = ["R", "L"]
_engines = {}


@pytest.fixture
def make_engine(gpu_engine, monkeypatch):
    def make(env):
        if not env:
            return gpu_engine
        key = tuple(sorted(env.items()))
        if key not in _engines:  # (an engine with knobs is made once and shared by the tests of this file)
            for k in cc.KNOBS:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            _engines[key] = psd_amd.Engine(device=0)
        return _engines[key]

    return make


def gpu_dev(mats):
    """a packed [len][n][n] column-major block on the device: (address, the tensor that owns it)"""
    import torch

    t = torch.from_numpy(pt.pack(mats, dtype=mats[0].dtype)).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=cc.shape_id)
@pytest.mark.parametrize("fam", cc.FAMILIES, ids=repr)
def test_against_reference(gpu_engine, fam, shape, lr):
    cc.case_reference(gpu_engine, fam, shape, lr)


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=cc.shape_id)
@pytest.mark.parametrize("fam", cc.FAMILIES, ids=repr)
def test_against_single_entry(gpu_engine, fam, shape, lr):
    cc.case_single(gpu_engine, fam, shape, lr)


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("fam", cc.FAMILIES, ids=repr)
def test_says_no_to_the_right_problem(gpu_engine, fam, lr):
    cc.case_says_no(gpu_engine, fam, lr)


@pytest.mark.parametrize("fam", [cc.Z, cc.ZG], ids=repr)
def test_nan_fails(gpu_engine, fam):
    cc.case_nan(gpu_engine, fam, "R")


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("fam", cc.FAMILIES, ids=repr)
def test_independence(make_engine, fam, lr):
    cc.case_independence(make_engine, fam, lr)


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("fam", cc.FAMILIES, ids=repr)
def test_fallback_above_a_lowered_cap(make_engine, fam, lr):
    cc.case_fallback(make_engine, fam, lr)


@pytest.mark.parametrize("fam", [cc.D, cc.Z], ids=repr)
def test_above_the_default_cap(gpu_engine, fam):
    cc.case_above_default_cap(gpu_engine, fam)


def test_cap_knob_only_lowers(make_engine):
    cc.case_cap_knob(make_engine)


@pytest.mark.parametrize("fam", cc.FAMILIES, ids=repr)
def test_argument_codes(gpu_engine, fam):
    cc.case_abi(gpu_engine, fam)


@pytest.mark.parametrize("fam", [cc.D, cc.ZG], ids=repr)
def test_argument_codes_device_entry(gpu_engine, fam):
    cc.case_abi(gpu_engine, fam, dev=gpu_dev)


def test_python_errors(gpu_engine):
    cc.case_python_errors(gpu_engine)


@pytest.mark.parametrize("n", [3, 17, 64])
def test_zcheckpsd_dev(gpu_engine, n):
    cc.case_zcheckpsd_dev(gpu_engine, n, gpu_dev)


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("fam", [cc.Z, cc.DG], ids=repr)
def test_device_resident_chain(gpu_engine, fam, lr):
    cc.case_device_chain(gpu_engine, fam, lr)


def test_empty_device_batch(gpu_engine):
    cc.case_empty_device_batch(gpu_engine)
