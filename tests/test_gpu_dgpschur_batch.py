"""GPU tier (MI355X): the Float64 signed batched entries — one workgroup per problem in stage 1 of the signed Hessenberg
reduction (psd_gbhess1), one wavefront per problem in stage 2 and in the iteration (psd_gbqz) — against the reference's
checks and the CPU oracle, place independence, holes, a failing problem, the argument codes, the device-resident entry
and the group loop."""
import pytest

import batch_cases as gc
import psd_amd
from batch_common import cap

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", gc.DG.shapes, ids=gc.shape_id)
def test_reduction(gpu_engine, shape):
    gc.case_reduction(gpu_engine, gc.DG, shape)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", gc.DG.shapes, ids=gc.shape_id)
def test_full_decomposition(gpu_engine, shape, lr):
    gc.case_full(gpu_engine, gc.DG, shape, lr)


@pytest.mark.parametrize("shape", [gc.DG.shapes[1], gc.DG.shapes[2], gc.DG.shapes[4]], ids=gc.shape_id)
def test_place_independence(gpu_engine, shape):
    gc.case_places(gpu_engine, shape)


def test_all_true_and_null_signature(gpu_engine):
    gc.case_all_true_dg(gpu_engine)


def test_flags(gpu_engine):
    gc.case_flags(gpu_engine, gc.DG)


@pytest.mark.parametrize("hole", gc.DG.holes, ids=gc.hole_id)
def test_holes(gpu_engine, hole):
    gc.case_holes_dg(gpu_engine, hole)


def test_one_problem_fails(gpu_engine):
    gc.case_one_fails(gpu_engine, gc.DG)


def test_argument_errors(gpu_engine):
    gc.case_argument_errors(gpu_engine, gc.DG)


def test_argument_codes(gpu_engine):
    """the codes of the four C entries (every one returns before anything reaches the device, or runs a batch of one)"""
    gc.case_abi_codes_gpu(gpu_engine, gc.DG)


def test_device_resident(gpu_engine):
    gc.case_device_resident(gpu_engine, gc.DG)


def test_above_the_cap(gpu_engine):
    """order cap + 1: the single call's signed reduction and iteration, problem by problem on the batch buffer"""
    gc.case_above_cap(gpu_engine, gc.DG, cap("psd_gbqz.h", "PSD_GB_NMAX") + 1)


def test_groups(monkeypatch):
    import torch

    torch.cuda.init()
    monkeypatch.delenv("PSD_BATCH_GROUP", raising=False)

    def make(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return psd_amd.Engine(device=0)

    gc.case_groups(make, gc.DG)
