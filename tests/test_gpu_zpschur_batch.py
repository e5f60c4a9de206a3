"""GPU tier (MI355X): the ComplexF64 batched entries — one workgroup per problem in the reduction (psd_zbhess), one per
(problem, factor) in the Q formation, one wavefront per problem in the iteration (psd_zbqz) — against numpy and the CPU
oracle, the fallback above PSD_ZB_NMAX, and the device-resident entry."""
import pytest

import batch_cases as zc
import psd_amd
from batch_common import cap

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [s for s in zc.Z.shapes if s[2] < 3], ids=zc.shape_id)
def test_reduction_bit_for_bit(gpu_engine, shape):
    """p < 3: the single call is the one-launch-per-link form, whose bodies the batched kernel calls in the same order"""
    zc.case_reduction_bits(gpu_engine, zc.Z, shape)


@pytest.mark.parametrize("shape", [s for s in zc.Z.shapes if s[2] >= 3], ids=zc.shape_id)
def test_reduction_against_lookahead_form(gpu_engine, shape):
    """p >= 3: the single call takes the look-ahead form and rounds differently"""
    zc.case_reduction_close(gpu_engine, zc.Z, shape)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", zc.Z.shapes, ids=zc.shape_id)
def test_full_decomposition(gpu_engine, shape, lr):
    zc.case_full(gpu_engine, zc.Z, shape, lr)


@pytest.mark.parametrize("hole", zc.Z.holes, ids=lambda h: "n%d_p%d_f%d_i%d" % h)
def test_holes(gpu_engine, hole):
    zc.case_holes_z(gpu_engine, hole)


def test_one_problem_fails(gpu_engine):
    zc.case_one_fails(gpu_engine, zc.Z)


def test_flags(gpu_engine):
    zc.case_flags(gpu_engine, zc.Z)


def test_argument_errors(gpu_engine):
    zc.case_argument_errors(gpu_engine, zc.Z)


def test_groups(monkeypatch):
    import torch

    torch.cuda.init()
    monkeypatch.delenv("PSD_BATCH_GROUP", raising=False)

    def make(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return psd_amd.Engine(device=0)

    zc.case_groups(make, zc.Z)


def test_device_resident(gpu_engine):
    zc.case_device_resident(gpu_engine, zc.Z)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_above_the_cap(gpu_engine, lr):
    """order PSD_ZB_NMAX + 1: the single call's reduction, Q formation and iteration, problem by problem on the batch
    buffer"""
    zc.case_full(gpu_engine, zc.Z, (2, cap("psd_zbhess.h", "PSD_ZB_NMAX") + 1, 2), lr)


def test_empty_device_batch(gpu_engine):
    """nb = 0: the shapes and dtypes of a call describe themselves, and no kernel runs"""
    import numpy as np
    import torch

    dA = torch.zeros((0, 2, 3, 3), dtype=torch.complex128, device="cuda")
    infos = [7]
    T, Z, values, st = gpu_engine.zpschur_batch_(dA, infos_out=infos)
    assert tuple(T.shape) == tuple(Z.shape) == (0, 2, 3, 3) and T.dtype == Z.dtype == torch.complex128 and T.is_cuda
    assert values.shape == (0, 3) and values.dtype == np.complex128 and infos == []
    assert isinstance(st, psd_amd.Stats) and st.nlaunch_step == 0 and st.niter == 0
    assert gpu_engine.zpschur_batch(dA, "L", wantZ=False)[1] is None


def test_device_input_is_left(gpu_engine):
    """the device entry always works on a copy, also of a tensor that already has the layout it works on"""
    import numpy as np
    import torch

    rng = np.random.default_rng(6)
    A = torch.from_numpy(rng.standard_normal((3, 2, 4, 4)) + 1j * rng.standard_normal((3, 2, 4, 4))).cuda()
    keep = A.clone()
    for X in (A, A.transpose(2, 3)):  # (contiguous; a transposed view of contiguous blocks)
        T, Z, values, _ = gpu_engine.zpschur_batch_(X)
        assert torch.equal(A, keep) and T.data_ptr() != A.data_ptr() and Z.data_ptr() != A.data_ptr()
        assert not torch.equal(T, X) and values.shape == (3, 4)
