"""GPU tier (MI355X): the batched signed Float64 reordering — one wavefront per problem, a group in one launch of
psd_gbord — against the single calls on the same device and the oracle, the fallback above PSD_BORD_NMAX, the device
entry on packed blocks for both alignments of each orientation, and the device-resident chain dgpschur_batch_ ->
dgordschur_batch_."""
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
@pytest.mark.parametrize("shape", gc.DG.windows, ids=gc.shape_id)
def test_windows(gpu_engine, shape, lr):
    gc.case_windows(gpu_engine, gc.DG, shape, lr)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_windows_narrow(make_engine, lr):
    gc.case_windows(make_engine({"PSD_BORD_W": "6"}), gc.DG, gc.DG.narrow, lr, expect_window=6)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_reference_shape(gpu_engine, lr):
    gc.case_reference(gpu_engine, gc.DG, lr)


def test_pairs_reference(gpu_engine):
    gc.case_pairs_reference(gpu_engine)


@pytest.mark.parametrize("shape", [gc.DG.windows[0], gc.DG.windows[3]], ids=gc.shape_id)
def test_independence(gpu_engine, shape):
    gc.case_independence(gpu_engine, gc.DG, shape)


def test_groups(make_engine):
    gc.case_groups(make_engine, gc.DG)


def test_fallback_above_the_cap(make_engine):
    gc.case_above_cap(make_engine, gc.DG)


def test_all_true_signature(gpu_engine):
    gc.case_all_true_dg(gpu_engine)


def test_per_problem_selections(gpu_engine):
    gc.case_selections(gpu_engine, gc.DG)


def test_one_problem_fails(gpu_engine):
    gc.case_one_fails(gpu_engine, gc.DG)


def test_argument_codes(gpu_engine):
    gc.case_argument_codes(gpu_engine, gc.DG)


def test_python_errors(gpu_engine):
    gc.case_python_errors(gpu_engine, gc.DG)


def test_device_entry_bits(gpu_engine):
    gc.case_dev_abi(gpu_engine, gc.DG, device=True)


def test_device_entry_bits_grouped(make_engine):
    # (5 problems in groups of 2, 2 and 1: the last group is a partial one)
    gc.case_dev_abi(make_engine({"PSD_BATCH_GROUP": "2"}), gc.DG, launches=3, device=True)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_device_resident_chain(gpu_engine, lr):
    gc.case_device_chain(gpu_engine, gc.DG, lr)


def test_empty_device_batch(gpu_engine):
    """nb = 0: the tensors come back as they are, the call's stats and swap counts are those of no problem, no kernel runs"""
    import numpy as np
    import torch

    T = torch.zeros((0, 2, 3, 3), dtype=torch.float64, device="cuda")
    Z = T.clone()
    gpu_engine.dgordschur_batch_stats, gpu_engine.dgordschur_batch_nswaps = None, np.ones(3, dtype=np.int32)
    infos = [7]
    T0, Z0, values, st = gpu_engine.dgordschur_batch_(T, Z, np.zeros((0, 3), dtype=bool), S=[True, False], infos_out=infos)
    assert T0 is T and Z0 is Z and values.shape == (0, 3) and values.dtype == np.complex128 and infos == []
    assert isinstance(st, psd_amd.Stats) and st.nlaunch_step == 0 and st.nsweeps == 0
    assert gpu_engine.dgordschur_batch_stats.nlaunch_step == 0 and gpu_engine.dgordschur_batch_stats.nsweeps == 0
    assert gpu_engine.dgordschur_batch_nswaps.shape == (0,) and gpu_engine.dgordschur_batch_nswaps.dtype == np.int32
    T1, Z1, _, _ = gpu_engine.dgordschur_batch(T, None, [True] * 3, S=[False, True], lr="L", schurindex=2, wantZ=False)
    assert tuple(T1.shape) == (0, 2, 3, 3) and T1.dtype == torch.float64 and Z1 is None


def test_device_copy_policy(gpu_engine):
    """what dgpschur_batch_ returns is reordered in place; any other layout is copied and stays as it was"""
    import numpy as np
    import torch

    rng = np.random.default_rng(8)
    A = torch.from_numpy(np.eye(4) + 0.25 * rng.standard_normal((3, 2, 4, 4))).cuda()
    S = [True, False]
    T, Z, values, _ = gpu_engine.dgpschur_batch_(A, S)
    sels = np.array([gc.median_select(v) for v in values])
    T1, Z1, values1, _ = gpu_engine.dgordschur_batch_(T, Z, sels, S=S)
    assert T1.data_ptr() == T.data_ptr() and Z1.data_ptr() == Z.data_ptr() and T1.stride() == T.stride()
    Tc, Zc = T1.contiguous(), Z1.contiguous()
    keepT, keepZ = Tc.clone(), Zc.clone()
    sel2 = np.zeros((3, 4), dtype=bool)
    sel2[:, 3] = True  # (the last row, alone or with its partner, has to move)
    T2, Z2, _, _ = gpu_engine.dgordschur_batch_(Tc, Zc, sel2, S=S)
    assert T2.data_ptr() != Tc.data_ptr() and Z2.data_ptr() != Zc.data_ptr()
    assert torch.equal(Tc, keepT) and torch.equal(Zc, keepZ) and not torch.equal(T2, Tc)
