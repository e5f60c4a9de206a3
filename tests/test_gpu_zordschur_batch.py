"""GPU tier (MI355X): the batched ComplexF64 reordering — one wavefront per problem, a group in one launch of psd_zbord —
against the single calls on the same device and the oracle, the fallback above PSD_BORD_NMAX, the device entry on packed
blocks for all four alignments, and the device-resident chain zpschur_batch_ -> zordschur_batch_."""
import pytest

import batch_common as bcm
import ord_batch_cases as zc
import psd_amd

pytestmark = pytest.mark.gpu

KNOBS = ("PSD_BATCH_GROUP", "PSD_BORD_W", "PSD_BORD_NMAX", "PSD_ORD_PIPE")
_engines = {}


@pytest.fixture
def make_engine(gpu_engine, monkeypatch):
    # (an engine with knobs is made once and shared by the tests of this file)
    return bcm.engine_maker(monkeypatch, KNOBS, lambda: psd_amd.Engine(device=0), _engines, default=gpu_engine)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_reference_shape(gpu_engine, lr):
    zc.case_reference(gpu_engine, zc.Z, lr)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", zc.Z.windows, ids=zc.shape_id)
def test_windows(gpu_engine, shape, lr):
    zc.case_windows(gpu_engine, zc.Z, shape, lr)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_windows_narrow(make_engine, lr):
    zc.case_windows(make_engine({"PSD_BORD_W": "6"}), zc.Z, zc.Z.narrow, lr, expect_window=6)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", zc.Z.windows, ids=zc.shape_id)
def test_against_serial_single_driver(make_engine, shape, lr):
    # (1e-12 * scale: contraction may differ between the kernels; the count of differing bits is printed)
    zc.case_against_serial(make_engine, zc.Z, shape, lr, exact=False)


@pytest.mark.parametrize("shape", [zc.Z.windows[0], zc.Z.windows[3]], ids=zc.shape_id)
def test_independence(gpu_engine, shape):
    zc.case_independence(gpu_engine, zc.Z, shape)


def test_groups(make_engine):
    zc.case_groups(make_engine, zc.Z)


def test_per_problem_selections(gpu_engine):
    zc.case_selections(gpu_engine, zc.Z)


def test_one_problem_fails(gpu_engine):
    zc.case_one_fails(gpu_engine, zc.Z)


def test_fallback_above_the_cap(make_engine):
    zc.case_above_cap(make_engine, zc.Z)


def test_argument_codes(gpu_engine):
    zc.case_argument_codes(gpu_engine, zc.Z)


def test_python_errors(gpu_engine):
    zc.case_python_errors(gpu_engine, zc.Z)


def test_device_entry_bits(gpu_engine):
    zc.case_dev_abi(gpu_engine, zc.Z, device=True)


def test_device_entry_bits_grouped(make_engine):
    # (5 problems in groups of 2, 2 and 1: the last group is a partial one)
    zc.case_dev_abi(make_engine({"PSD_BATCH_GROUP": "2"}), zc.Z, launches=3, device=True)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_device_resident_chain(gpu_engine, lr):
    zc.case_device_chain(gpu_engine, zc.Z, lr)


def test_empty_device_batch(gpu_engine):
    """nb = 0: the tensors come back as they are, the call's stats and swap counts are those of no problem, no kernel runs"""
    import numpy as np
    import torch

    T = torch.zeros((0, 2, 3, 3), dtype=torch.complex128, device="cuda")
    Z = T.clone()
    gpu_engine.zordschur_batch_stats, gpu_engine.zordschur_batch_nswaps = None, np.ones(3, dtype=np.int32)
    infos = [7]
    T0, Z0, values, st = gpu_engine.zordschur_batch_(T, Z, np.zeros((0, 3), dtype=bool), infos_out=infos)
    assert T0 is T and Z0 is Z and values.shape == (0, 3) and values.dtype == np.complex128 and infos == []
    assert isinstance(st, psd_amd.Stats) and st.nlaunch_step == 0 and st.nsweeps == 0
    assert gpu_engine.zordschur_batch_stats.nlaunch_step == 0 and gpu_engine.zordschur_batch_stats.nsweeps == 0
    assert gpu_engine.zordschur_batch_nswaps.shape == (0,) and gpu_engine.zordschur_batch_nswaps.dtype == np.int32
    T1, Z1, _, _ = gpu_engine.zordschur_batch(T, None, [True] * 3, lr="L", schurindex=2, wantZ=False)
    assert tuple(T1.shape) == (0, 2, 3, 3) and T1.dtype == torch.complex128 and Z1 is None


def test_device_copy_policy(gpu_engine):
    """what zpschur_batch_ returns is reordered in place; any other layout is copied and stays as it was"""
    import numpy as np
    import torch

    rng = np.random.default_rng(8)
    A = torch.from_numpy(rng.standard_normal((3, 2, 4, 4)) + 1j * rng.standard_normal((3, 2, 4, 4))).cuda()
    T, Z, values, _ = gpu_engine.zpschur_batch_(A)
    sels = np.array([zc.median_select(v) for v in values])
    T1, Z1, values1, _ = gpu_engine.zordschur_batch_(T, Z, sels)
    assert T1.data_ptr() == T.data_ptr() and Z1.data_ptr() == Z.data_ptr() and T1.stride() == T.stride()
    Tc, Zc = T1.contiguous(), Z1.contiguous()
    keepT, keepZ = Tc.clone(), Zc.clone()
    T2, Z2, _, _ = gpu_engine.zordschur_batch_(Tc, Zc, ~np.array([zc.median_select(v) for v in values1]))
    assert T2.data_ptr() != Tc.data_ptr() and Z2.data_ptr() != Zc.data_ptr()
    assert torch.equal(Tc, keepT) and torch.equal(Zc, keepZ) and not torch.equal(T2, Tc)
