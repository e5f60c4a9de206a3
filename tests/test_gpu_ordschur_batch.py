"""GPU tier (MI355X): the batched reordering — one wavefront per problem, a group in one launch of psd_bord — against
the single calls on the same engine and the oracle, the fallback above PSD_BORD_NMAX, and the device-resident chain
pschur_batch_ -> ordschur_batch_ -> eigvecs_batch."""
import pytest

import batch_common as bcm
import ord_batch_cases as oc
import psd_amd

pytestmark = pytest.mark.gpu

KNOBS = ("PSD_BATCH_GROUP", "PSD_BORD_W", "PSD_BORD_NMAX")


@pytest.fixture
def make_engine(gpu_engine, monkeypatch):
    return bcm.engine_maker(monkeypatch, KNOBS, lambda: psd_amd.Engine(device=0), {}, default=gpu_engine)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_reference_shape(gpu_engine, lr):
    oc.case_reference(gpu_engine, oc.D, lr)


def test_reference_pairs(gpu_engine):
    oc.case_pairs(gpu_engine)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", oc.D.windows, ids=oc.shape_id)
def test_windows(gpu_engine, shape, lr):
    oc.case_windows(gpu_engine, oc.D, shape, lr)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_windows_narrow(make_engine, lr):
    oc.case_windows(make_engine({"PSD_BORD_W": "6"}), oc.D, oc.D.narrow, lr, expect_window=6)


@pytest.mark.parametrize("shape", [oc.D.windows[0], oc.D.windows[3]], ids=oc.shape_id)
def test_independence(gpu_engine, shape):
    oc.case_independence(gpu_engine, oc.D, shape)


def test_groups(make_engine):
    oc.case_groups(make_engine, oc.D)


def test_per_problem_selections(gpu_engine):
    oc.case_selections_d(gpu_engine)


def test_one_problem_fails(gpu_engine):
    oc.case_one_fails(gpu_engine, oc.D)


def test_fallback_above_the_cap(make_engine):
    oc.case_above_cap(make_engine, oc.D)


def test_argument_codes(gpu_engine):
    oc.case_argument_codes(gpu_engine, oc.D)


def test_python_errors(gpu_engine):
    oc.case_python_errors(gpu_engine, oc.D)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_device_resident_chain(gpu_engine, lr):
    oc.case_device_chain(gpu_engine, oc.D, lr)


def test_empty_device_batch(gpu_engine):
    """nb = 0: the tensors come back as they are, the call's stats and swap counts are those of no problem, no kernel runs"""
    import numpy as np
    import torch

    T = torch.zeros((0, 2, 3, 3), dtype=torch.float64, device="cuda")
    Z = T.clone()
    gpu_engine.ordschur_batch_stats, gpu_engine.ordschur_batch_nswaps = None, np.ones(3, dtype=np.int32)
    infos = [7]
    T0, Z0, values, st = gpu_engine.ordschur_batch_(T, Z, np.zeros((0, 3), dtype=bool), infos_out=infos)
    assert T0 is T and Z0 is Z and values.shape == (0, 3) and values.dtype == np.complex128 and infos == []
    assert isinstance(st, psd_amd.Stats) and st.nlaunch_step == 0 and st.nsweeps == 0
    assert gpu_engine.ordschur_batch_stats.nlaunch_step == 0 and gpu_engine.ordschur_batch_stats.nsweeps == 0
    assert gpu_engine.ordschur_batch_nswaps.shape == (0,) and gpu_engine.ordschur_batch_nswaps.dtype == np.int32
    T1, Z1, _, _ = gpu_engine.ordschur_batch(T, None, [True] * 3, lr="L", schurindex=2, wantZ=False)
    assert tuple(T1.shape) == (0, 2, 3, 3) and T1.dtype == torch.float64 and Z1 is None


def test_device_copy_policy(gpu_engine):
    """what pschur_batch_ returns is reordered in place; any other layout is copied and stays as it was"""
    import numpy as np
    import torch

    A = torch.from_numpy(np.random.default_rng(7).standard_normal((3, 2, 4, 4))).cuda()
    T, Z, values, _ = gpu_engine.pschur_batch_(A)
    sels = np.array([oc.median_select(v) for v in values])
    T1, Z1, values1, _ = gpu_engine.ordschur_batch_(T, Z, sels)
    assert T1.data_ptr() == T.data_ptr() and Z1.data_ptr() == Z.data_ptr() and T1.stride() == T.stride()
    Tc, Zc = T1.contiguous(), Z1.contiguous()
    keepT, keepZ = Tc.clone(), Zc.clone()
    T2, Z2, _, _ = gpu_engine.ordschur_batch_(Tc, Zc, ~np.array([oc.median_select(v) for v in values1]))
    assert T2.data_ptr() != Tc.data_ptr() and Z2.data_ptr() != Zc.data_ptr()
    assert torch.equal(Tc, keepT) and torch.equal(Zc, keepZ) and not torch.equal(T2, Tc)
