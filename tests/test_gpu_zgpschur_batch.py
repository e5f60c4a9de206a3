"""GPU tier (MI355X): the ComplexF64 signed batched entries — one workgroup per problem in stage 1 of the signed
Hessenberg reduction (psd_zgbhess1), one wavefront per problem in stage 2 and in the iteration (psd_zgbqz) — against the
reference's checks and the CPU oracle, the fallback above the order cap, and the device-resident entry."""
import pytest

import batch_cases as gc
import psd_amd
from batch_common import cap

pytestmark = pytest.mark.gpu


def _zgb_nmax():
    """The order cap of the signed batch kernels as the sources define it: PSD_ZGB_NMAX if the host driver has one,
    PSD_ZB_NMAX (the cap of the all-true path, reused) otherwise."""
    for name, macro in (("psd_zgbqz.h", "PSD_ZGB_NMAX"), ("psd_zbhess.h", "PSD_ZB_NMAX")):
        nmax = cap(name, macro)
        if nmax is not None:
            return nmax
    raise AssertionError("no order cap found")


@pytest.mark.parametrize("shape", gc.ZG.shapes, ids=gc.shape_id)
def test_reduction(gpu_engine, shape):
    gc.case_reduction(gpu_engine, gc.ZG, shape)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", gc.ZG.shapes, ids=gc.shape_id)
def test_full_decomposition(gpu_engine, shape, lr):
    gc.case_full(gpu_engine, gc.ZG, shape, lr)


def test_all_true_signature(gpu_engine):
    gc.case_all_true_zg(gpu_engine)


def test_gpschur_batch(gpu_engine):
    gc.case_gpschur_batch(gpu_engine)


@pytest.mark.parametrize("hole", gc.ZG.holes, ids=gc.hole_id)
def test_holes(gpu_engine, hole):
    gc.case_holes_zg(gpu_engine, hole)


def test_one_problem_fails(gpu_engine):
    gc.case_one_fails(gpu_engine, gc.ZG)


def test_flags(gpu_engine):
    gc.case_flags(gpu_engine, gc.ZG)


def test_argument_errors(gpu_engine):
    gc.case_argument_errors(gpu_engine, gc.ZG)


def test_groups(monkeypatch):
    import torch

    torch.cuda.init()
    monkeypatch.delenv("PSD_BATCH_GROUP", raising=False)

    def make(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return psd_amd.Engine(device=0)

    gc.case_groups(make, gc.ZG)


def test_device_resident(gpu_engine):
    gc.case_device_resident(gpu_engine, gc.ZG)


def test_above_the_cap(gpu_engine):
    """order cap + 1: the single call's signed reduction and iteration, problem by problem on the batch buffer"""
    gc.case_above_cap(gpu_engine, gc.ZG, _zgb_nmax() + 1)


def test_empty_device_batch(gpu_engine):
    """nb = 0: the shapes and dtypes of a call describe themselves, and no kernel runs; the signature is still checked"""
    import numpy as np
    import torch

    dA = torch.zeros((0, 2, 3, 3), dtype=torch.complex128, device="cuda")
    infos = [7]
    T, Z, values, st = gpu_engine.zgpschur_batch_(dA, [True, False], infos_out=infos)
    assert tuple(T.shape) == tuple(Z.shape) == (0, 2, 3, 3) and T.dtype == Z.dtype == torch.complex128 and T.is_cuda
    assert values.shape == (0, 3) and values.dtype == np.complex128 and infos == []
    assert isinstance(st, psd_amd.Stats) and st.nlaunch_step == 0 and st.niter == 0
    assert gpu_engine.zpschur_batch(dA, "L", S=[False, True], wantZ=False)[1] is None
    with pytest.raises(psd_amd.DimensionMismatch):
        gpu_engine.zgpschur_batch_(dA, [True, False, True])
