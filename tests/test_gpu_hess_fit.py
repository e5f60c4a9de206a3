"""Launch geometry of the look-ahead Hessenberg reduction fitted to the trailing block (csrc/psd_hess2.h: psd_h2_fit_chain,
psd_h2_fit_panel) against the full-size launches of PSD_H2_FIT=0: the narrower instantiations drop only loop steps that the
kernels' guards skip anyway, so the packed factors and tau must be the SAME BITS, in every form of the reduction and across
every switch of the register depth NK (the smallest of 4, 8, 16, 32 with 64 NK >= reflector length: the switches lie at
m = 1024, 512, 256).  The fitted results are also held against the CPU oracle with the tolerances of
test_phessenberg_two_stream_vs_oracle.

Sizes: n off the 8-row strips and the 64-column steps; periods that are no multiple of K, so that a batch of panel
updates straddles a switch; n - 1 = 64, 65, 128, 129 puts the steps of the strip and column-group counts on the first
columns and ends in the m = 1, 2 columns (tau = 0 for the last)."""
import numpy as np
import pytest

import psdtest as pt

pytestmark = pytest.mark.gpu

ONE_STREAM = {}


def multi(K, pipe, depth=None):
    env = {"PSD_HESS_ASYNC": str(K), "PSD_H2_PIPE": pipe}
    if depth:
        env["PSD_H2_DEPTH"] = depth
    return env


# (n, p, environment of the form)
CASES = [
    pytest.param(140, 5, ONE_STREAM, id="140x5-one-stream"),    # <4,8>: the grids alone follow the block
    pytest.param(530, 3, ONE_STREAM, id="530x3-one-stream"),    # <16,4>: crosses 512 and 256
    pytest.param(140, 9, multi(4, "2"), id="140x9-K4-pipe"),
    pytest.param(140, 9, multi(4, "0"), id="140x9-K4-back-to-back"),
    pytest.param(270, 16, multi(8, "2"), id="270x16-K8-pipe"),
    pytest.param(270, 16, multi(8, "0"), id="270x16-K8-back-to-back"),
    pytest.param(270, 16, multi(8, "2", "2"), id="270x16-K8-pipe-depth2"),
    pytest.param(530, 40, multi(16, "2"), id="530x40-K16-pipe"),
    pytest.param(530, 40, multi(16, "0"), id="530x40-K16-back-to-back"),
    pytest.param(64, 70, multi(16, "2"), id="64x70-K16-pipe"),
    pytest.param(64, 70, multi(16, "0"), id="64x70-K16-back-to-back"),
    # edge columns: n - 1 = 64, 65, 128, 129
    pytest.param(65, 3, ONE_STREAM, id="65x3-edge"),
    pytest.param(66, 3, ONE_STREAM, id="66x3-edge"),
    pytest.param(129, 3, ONE_STREAM, id="129x3-edge"),
    pytest.param(130, 3, ONE_STREAM, id="130x3-edge"),
    pytest.param(1100, 3, ONE_STREAM, id="1100x3-one-stream"),  # <32,8>: crosses 1024
]
# bits only (the oracle takes too long at this size): <32,8> in the pipe form, panel launches with one column per wavefront
BITS_ONLY = [pytest.param(1030, 9, multi(4, "2"), id="1030x9-K4-pipe")]

_inputs, _oracle, _runs = {}, {}, {}


def factors(n, p):
    if (n, p) not in _inputs:
        _inputs[(n, p)] = pt.bench_factors(n, p, seed=270 + n + p)
    return _inputs[(n, p)]


def oracle(n, p):
    if (n, p) not in _oracle:
        _, _, packed, tauo = pt.oracle_phessenberg(factors(n, p))
        _oracle[(n, p)] = (packed, tauo)
    return _oracle[(n, p)]


def reduce_(monkeypatch, n, p, env, fit):
    """(packed factors, tau) of phessenberg_ with a fresh engine in the given form; fit: None (default) or "0" """
    key = (n, p, tuple(sorted(env.items())), fit)
    if key not in _runs:
        import torch

        torch.cuda.init()
        import psd_amd

        for k, v in env.items():
            monkeypatch.setenv(k, v)
        if fit is None:
            monkeypatch.delenv("PSD_H2_FIT", raising=False)
        else:
            monkeypatch.setenv("PSD_H2_FIT", fit)
        eng = psd_amd.Engine(device=0)
        W = [a.copy(order="F") for a in factors(n, p)]
        _, tau, _ = eng.phessenberg_(W)
        del eng
        _runs[key] = (W, np.array(tau))
    return _runs[key]


@pytest.mark.parametrize("n,p,env", CASES + BITS_ONLY)
def test_fitted_launches_give_the_same_bits(monkeypatch, n, p, env):
    Wfix, taufix = reduce_(monkeypatch, n, p, env, "0")
    Wfit, taufit = reduce_(monkeypatch, n, p, env, None)
    for j in range(p):
        assert np.array_equal(Wfit[j], Wfix[j]), (j, np.abs(Wfit[j] - Wfix[j]).max())
    assert np.array_equal(taufit, taufix)
    # (the reduction did run: an identity result would compare equal too)
    assert np.count_nonzero(taufit) >= (n - 2) * p


@pytest.mark.parametrize("n,p,env", CASES)
def test_fitted_launches_vs_oracle(monkeypatch, n, p, env):
    W, tau = reduce_(monkeypatch, n, p, env, None)
    packed, tauo = oracle(n, p)
    for j in range(p):
        assert np.linalg.norm(W[j] - packed[j]) < 1e-11 * max(np.linalg.norm(packed[j]), 1.0), (j,)
        assert np.allclose(tau[j], tauo[j], rtol=0, atol=1e-11)
    # the last column holds the one-entry reflector (m = 1, tau = 0: H = I): exact zeros where the oracle has them
    assert np.array_equal(tau[:, n - 2:] == 0.0, tauo[:, n - 2:] == 0.0)
    assert np.count_nonzero(tauo[:, n - 2] == 0.0) == 1
