"""GPU tier (MI355X): the batched signed ComplexF64 reordering — one wavefront per problem, a group in one launch of
psd_zgbord — against the single calls on the same device and the oracle, the fallback above PSD_BORD_NMAX, the device
entry on packed blocks for both alignments of each orientation, and the device-resident chain zgpschur_batch_ ->
zgordschur_batch_."""
import pytest

import batch_common as bcm
import ord_batch_cases as gc
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
    gc.case_reference(gpu_engine, gc.ZG, lr)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", gc.ZG.windows, ids=gc.shape_id)
def test_windows(gpu_engine, shape, lr):
    gc.case_windows(gpu_engine, gc.ZG, shape, lr)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_windows_narrow(make_engine, lr):
    gc.case_windows(make_engine({"PSD_BORD_W": "6"}), gc.ZG, gc.ZG.narrow, lr, expect_window=6)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", gc.ZG.windows, ids=gc.shape_id)
def test_against_serial_single_driver(make_engine, shape, lr):
    # (1e-12 * scale: contraction may differ between the kernels; the count of differing bits is printed)
    gc.case_against_serial(make_engine, gc.ZG, shape, lr, exact=False)


@pytest.mark.parametrize("shape", [gc.ZG.windows[0], gc.ZG.windows[3]], ids=gc.shape_id)
def test_independence(gpu_engine, shape):
    gc.case_independence(gpu_engine, gc.ZG, shape)


def test_groups(make_engine):
    gc.case_groups(make_engine, gc.ZG)


def test_all_true_signature(gpu_engine):
    gc.case_all_true_zg(gpu_engine)


def test_per_problem_selections(gpu_engine):
    gc.case_selections(gpu_engine, gc.ZG)


def test_one_problem_fails(gpu_engine):
    gc.case_one_fails(gpu_engine, gc.ZG)


def test_fallback_above_the_cap(make_engine):
    gc.case_above_cap(make_engine, gc.ZG)


def test_argument_codes(gpu_engine):
    gc.case_argument_codes(gpu_engine, gc.ZG)


def test_python_errors(gpu_engine):
    gc.case_python_errors(gpu_engine, gc.ZG)


def test_device_entry_bits(gpu_engine):
    gc.case_dev_abi(gpu_engine, gc.ZG, device=True)


def test_device_entry_bits_grouped(make_engine):
    # (5 problems in groups of 2, 2 and 1: the last group is a partial one)
    gc.case_dev_abi(make_engine({"PSD_BATCH_GROUP": "2"}), gc.ZG, launches=3, device=True)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_device_resident_chain(gpu_engine, lr):
    gc.case_device_chain(gpu_engine, gc.ZG, lr)


def test_empty_device_batch(gpu_engine):
    """nb = 0: the tensors come back as they are, the call's stats and swap counts are those of no problem, no kernel runs"""
    import numpy as np
    import torch

    T = torch.zeros((0, 2, 3, 3), dtype=torch.complex128, device="cuda")
    Z = T.clone()
    gpu_engine.zgordschur_batch_stats, gpu_engine.zgordschur_batch_nswaps = None, np.ones(3, dtype=np.int32)
    infos = [7]
    T0, Z0, values, st = gpu_engine.zgordschur_batch_(T, Z, np.zeros((0, 3), dtype=bool), S=[True, False], infos_out=infos)
    assert T0 is T and Z0 is Z and values.shape == (0, 3) and values.dtype == np.complex128 and infos == []
    assert isinstance(st, psd_amd.Stats) and st.nlaunch_step == 0 and st.nsweeps == 0
    assert gpu_engine.zgordschur_batch_stats.nlaunch_step == 0 and gpu_engine.zgordschur_batch_stats.nsweeps == 0
    assert gpu_engine.zgordschur_batch_nswaps.shape == (0,) and gpu_engine.zgordschur_batch_nswaps.dtype == np.int32
    T1, Z1, _, _ = gpu_engine.zgordschur_batch(T, None, [True] * 3, S=[False, True], lr="L", schurindex=2, wantZ=False)
    assert tuple(T1.shape) == (0, 2, 3, 3) and T1.dtype == torch.complex128 and Z1 is None


def test_device_copy_policy(gpu_engine):
    """what zgpschur_batch_ returns is reordered in place; any other layout is copied and stays as it was"""
    import numpy as np
    import torch

    rng = np.random.default_rng(8)
    A = torch.from_numpy(np.eye(4) + 0.25 * (rng.standard_normal((3, 2, 4, 4)) + 1j * rng.standard_normal((3, 2, 4, 4)))).cuda()
    S = [True, False]
    T, Z, values, _ = gpu_engine.zgpschur_batch_(A, S)
    sels = np.array([gc.median_select(v) for v in values])
    T1, Z1, values1, _ = gpu_engine.zgordschur_batch_(T, Z, sels, S=S)
    assert T1.data_ptr() == T.data_ptr() and Z1.data_ptr() == Z.data_ptr() and T1.stride() == T.stride()
    Tc, Zc = T1.contiguous(), Z1.contiguous()
    keepT, keepZ = Tc.clone(), Zc.clone()
    T2, Z2, _, _ = gpu_engine.zgordschur_batch_(Tc, Zc, ~np.array([gc.median_select(v) for v in values1]), S=S)
    assert T2.data_ptr() != Tc.data_ptr() and Z2.data_ptr() != Zc.data_ptr()
    assert torch.equal(Tc, keepT) and torch.equal(Zc, keepZ) and not torch.equal(T2, Tc)
