"""GPU tier (MI355X): the ComplexF64 batched entries — one workgroup per problem in the reduction (psd_zbhess), one per
(problem, factor) in the Q formation, one wavefront per problem in the iteration (psd_zbqz) — against numpy and the CPU
oracle, the fallback above PSD_ZB_NMAX, and the device-resident entry."""
import os
import re

import pytest

import psd_amd
import zbatch_cases as zc

pytestmark = pytest.mark.gpu


def _zb_nmax():
    """PSD_ZB_NMAX as the kernel header defines it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "periodicschurdecompositions.jl_amd", "csrc", "psd_zbhess.h")) as fh:
        return int(re.search(r"^#define PSD_ZB_NMAX (\d+)", fh.read(), re.M).group(1))


@pytest.mark.parametrize("shape", [s for s in zc.SHAPES if s[2] < 3], ids=zc.shape_id)
def test_reduction_bit_for_bit(gpu_engine, shape):
    """p < 3: the single call is the one-launch-per-link form, whose bodies the batched kernel calls in the same order"""
    zc.case_reduction_bits(gpu_engine, shape)


@pytest.mark.parametrize("shape", [s for s in zc.SHAPES if s[2] >= 3], ids=zc.shape_id)
def test_reduction_against_lookahead_form(gpu_engine, shape):
    """p >= 3: the single call takes the look-ahead form and rounds differently"""
    zc.case_reduction_close(gpu_engine, shape)


@pytest.mark.parametrize("lr", ["R", "L"])
@pytest.mark.parametrize("shape", zc.SHAPES, ids=zc.shape_id)
def test_full_decomposition(gpu_engine, shape, lr):
    zc.case_full(gpu_engine, shape, lr)


@pytest.mark.parametrize("hole", zc.HOLES, ids=lambda h: "n%d_p%d_f%d_i%d" % h)
def test_holes(gpu_engine, hole):
    zc.case_holes(gpu_engine, hole)


def test_one_problem_fails(gpu_engine):
    zc.case_one_fails(gpu_engine)


def test_flags(gpu_engine):
    zc.case_flags(gpu_engine)


def test_argument_errors(gpu_engine):
    zc.case_argument_errors(gpu_engine)


def test_groups(monkeypatch):
    import torch

    torch.cuda.init()
    monkeypatch.delenv("PSD_BATCH_GROUP", raising=False)

    def make(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return psd_amd.Engine(device=0)

    zc.case_groups(make)


def test_device_resident(gpu_engine):
    zc.case_device_resident(gpu_engine)


@pytest.mark.parametrize("lr", ["R", "L"])
def test_above_the_cap(gpu_engine, lr):
    """order PSD_ZB_NMAX + 1: the single call's reduction, Q formation and iteration, problem by problem on the batch
    buffer"""
    zc.case_full(gpu_engine, (2, _zb_nmax() + 1, 2), lr)
