"""GPU tier (MI355X): the batched entries — one workgroup per problem in the reduction (psd_bhess), one per (problem,
factor) in the Q formation, the iteration 32 problems at a time — against the single calls on the same engine, the
fallback above PSD_BH_NMAX, and the device-resident entry."""
import pytest

import batch_cases as bc
import psd_amd
from batch_common import cap

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", bc.D.hess_shapes, ids=bc.shape_id)
def test_reduction_bit_for_bit(gpu_engine, shape):
    """p < 3: the single call is the one-launch-per-link form, whose bodies the batched kernel calls in the same order"""
    bc.case_reduction_bits(gpu_engine, bc.D, shape)


@pytest.mark.parametrize("shape", bc.D.hess_shapes_p3, ids=bc.shape_id)
def test_reduction_against_lookahead_form(gpu_engine, shape):
    """p >= 3: the single call takes the look-ahead form and rounds differently"""
    bc.case_reduction_close(gpu_engine, bc.D, shape)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", bc.D.shapes, ids=bc.shape_id)
def test_full_decomposition(gpu_engine, shape, lr):
    bc.case_full_d(gpu_engine, shape, lr)


def test_flags(gpu_engine):
    bc.case_flags(gpu_engine, bc.D)


def test_one_problem_fails(gpu_engine):
    """(the inputs are built for the simulation's single call; here the batch's own pattern and results are checked)"""
    bc.case_one_fails(gpu_engine, bc.D)


def test_argument_errors(gpu_engine):
    bc.case_argument_errors(gpu_engine, bc.D)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_above_the_cap(gpu_engine, lr):
    """order PSD_BH_NMAX + 1: the multi-workgroup reduction and Q formation, problem by problem on the batch buffer"""
    bc.case_full_d(gpu_engine, (2, cap("psd_bhess.h", "PSD_BH_NMAX") + 1, 2), lr)


def test_device_resident(gpu_engine):
    bc.case_device_resident(gpu_engine, bc.D)


def test_argument_codes(gpu_engine):
    bc.case_abi_codes_d(gpu_engine)


def test_groups(monkeypatch):
    import torch

    torch.cuda.init()
    monkeypatch.delenv("PSD_BATCH_GROUP", raising=False)

    def make(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return psd_amd.Engine(device=0)

    bc.case_groups(make, bc.D)


def test_empty_device_batch(gpu_engine):
    """nb = 0: the shapes and dtypes of a call describe themselves, and no kernel runs"""
    import numpy as np
    import torch

    dA = torch.zeros((0, 2, 3, 3), dtype=torch.float64, device="cuda")
    infos = [7]
    T, Z, values, st = gpu_engine.pschur_batch_(dA, infos_out=infos)
    assert tuple(T.shape) == tuple(Z.shape) == (0, 2, 3, 3) and T.dtype == Z.dtype == torch.float64 and T.is_cuda
    assert values.shape == (0, 3) and values.dtype == np.complex128 and infos == []
    assert isinstance(st, psd_amd.Stats) and st.nlaunch_step == 0 and st.niter == 0
    assert gpu_engine.pschur_batch(dA, "L", wantZ=False)[1] is None


def test_device_input_is_left(gpu_engine):
    """the device entry always works on a copy, also of a tensor that already has the layout it works on"""
    import numpy as np
    import torch

    A = torch.from_numpy(np.random.default_rng(5).standard_normal((3, 2, 4, 4))).cuda()
    keep = A.clone()
    for X in (A, A.transpose(2, 3)):  # (contiguous; a transposed view of contiguous blocks)
        T, Z, values, _ = gpu_engine.pschur_batch_(X)
        assert torch.equal(A, keep) and T.data_ptr() != A.data_ptr() and Z.data_ptr() != A.data_ptr()
        assert not torch.equal(T, X) and values.shape == (3, 4)
