"""GPU tier (MI355X): partial_pschur (periodic Krylov-Schur, src/krylov.jl:446-798) on the device — the cases of the
simulated tier, large dense factors against the device's own full pschur!, the device-resident entry with torch tensors,
and run-to-run bit identity."""
import numpy as np
import pytest

import krylov_cases as kc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", ["LM", "SR", "LR"])
def test_real_targets(gpu_engine, which):
    As = kc.mkmats1(30, 3, seed=11)
    kc.pkstest(gpu_engine, As, which, kc.full_values(As))


@pytest.mark.parametrize("which", ["LM", "SR", "LR", "LI", "SI"])
def test_complex_targets(gpu_engine, which):
    As = kc.mkmats1(30, 3, cplx=True, seed=12)
    kc.pkstest(gpu_engine, As, which, kc.full_values(As))


@pytest.mark.parametrize("cplx", [False, True])
def test_period_one_and_n200(gpu_engine, cplx):
    As = kc.mkmats1(30, 1, cplx=cplx, seed=14)
    kc.pkstest(gpu_engine, As, "LM", kc.full_values(As))
    As = kc.mkmats1(200, 8, xpnd=1.05, cplx=cplx, seed=13, unit=True)
    kc.pkstest(gpu_engine, As, "LM", kc.full_values(As))


def test_rank_deficient(gpu_engine):
    As = kc.rank_deficient(30, 3, 3)
    P, h = gpu_engine.partial_pschur(As, 2, "LM", mindim=6, maxdim=12, tol=1e-10, restarts=60, seed=5)
    assert P.stats.nreinit > 0 and P.stats.ndeflate > 0
    kc.check(P, As, 1e-10)


def test_bit_identical_runs(gpu_engine):
    As = kc.mkmats1(200, 8, xpnd=1.05, seed=21, unit=True)
    kw = dict(mindim=6, maxdim=12, tol=1e-10, restarts=60, seed=9)
    kc.same_bits(*gpu_engine.partial_pschur(As, 4, "LM", **kw), *gpu_engine.partial_pschur(As, 4, "LM", **kw))


def test_device_resident_matches_host_entry(gpu_engine):
    import torch

    As = kc.mkmats1(300, 4, xpnd=1.02, seed=22, unit=True)
    kw = dict(mindim=6, maxdim=12, tol=1e-10, restarts=60, seed=3)
    Ph, hh = gpu_engine.partial_pschur(As, 4, "LM", **kw)
    dA = torch.stack([torch.from_numpy(np.ascontiguousarray(a)) for a in As]).cuda()
    Pd, hd = gpu_engine.partial_pschur(dA, 4, "LM", **kw)
    assert isinstance(Pd.Z[0], torch.Tensor) and Pd.Z[0].is_cuda
    kc.same_bits(Ph, hh, Pd, hd)
    Vd = gpu_engine.eigvecs(Pd, [True] + [False] * (Pd.Z[0].shape[1] - 1))
    assert isinstance(Vd[0], torch.Tensor)


def test_real_2048x16_vs_device_pschur(gpu_engine):
    n, p, nev = 2048, 16, 6
    As = kc.dominant(n, p, seed=31)
    P, h = gpu_engine.partial_pschur(As, nev, "LM", tol=1e-10, restarts=100, seed=1)
    assert h.nconverged >= nev, h
    kc.check(P, As, 1e-10)
    full = np.asarray(gpu_engine.pschur([a.copy(order="F") for a in As], "L").values)
    kc.check_values(P, full, "LM", nev)
    top = full[np.argsort(-np.abs(full), kind="stable")[:nev]]
    for lam in top[:nev // 2]:  # the dominant values themselves are found
        assert np.min(np.abs(P.values - lam)) <= 1e-6 * abs(lam), (lam, P.values)


def test_complex_2048x8_vs_device_pschur(gpu_engine):
    n, p, nev = 2048, 8, 6
    As = kc.dominant(n, p, cplx=True, seed=32)
    P, h = gpu_engine.partial_pschur(As, nev, "LM", tol=1e-10, restarts=100, seed=2)
    assert h.nconverged >= nev, h
    kc.check(P, As, 1e-10)
    full = np.asarray(gpu_engine.pschur([a.copy(order="F") for a in As], "L").values)
    kc.check_values(P, full, "LM", nev)


def test_real_8192x8_device_resident(gpu_engine):
    """4 GB of factors generated and kept on the device: relation residuals and orthonormality by torch on the device."""
    import torch

    n, p, nev = 8192, 8, 6
    g = torch.Generator(device="cuda").manual_seed(41)
    dA = torch.randn((p, n, n), generator=g, device="cuda", dtype=torch.float64).mul_(0.3 / np.sqrt(n))
    d = torch.ones(n, device="cuda", dtype=torch.float64)
    d[:16] = torch.linspace(2.0, 1.3, 16, device="cuda", dtype=torch.float64)
    dA.diagonal(dim1=1, dim2=2).add_(d)
    P, h = gpu_engine.partial_pschur(dA, nev, "LM", tol=1e-10, restarts=100, seed=4)
    assert h.nconverged >= nev // 2, h
    k = P.Z[0].shape[1]
    eps = np.finfo(np.float64).eps
    lmax = float(np.max(np.abs(P.values)))
    for l in range(p):
        Zl, Zn = P.Z[l], P.Z[(l + 1) % p]
        Tl = torch.as_tensor(P.Ts[l], device="cuda")
        res = torch.linalg.vector_norm(dA[l] @ Zl - Zn @ Tl, dim=0).max().item()
        an = torch.linalg.matrix_norm(dA[l]).item()  # (Frobenius: an upper bound of the 2-norm)
        bound = 1e3 * n * eps * an + (100 * 1e-10 * lmax if l == p - 1 else 0.0)
        assert res <= bound, (l, res, bound)
        orth = torch.linalg.matrix_norm(Zl.T @ Zl - torch.eye(k, device="cuda", dtype=torch.float64)).item()
        assert orth < 100 * n * eps, (l, orth)


@pytest.mark.parametrize("n,p,kw", [(31, 3, {}), (257, 2, dict(xpnd=1.05, unit=True)), (513, 2, dict(xpnd=1.02, unit=True))])
def test_odd_real_orders(gpu_engine, n, p, kw):
    """Odd orders take the one-row body psd_kr_mv<false, 1> of the Float64 matvec through the whole driver (one row
    either side of a tile at 257 and 513)."""
    As = kc.mkmats1(n, p, **kw)
    kc.pkstest(gpu_engine, As, "LM", kc.full_values(As))


@pytest.mark.parametrize("cplx", [False, True])
def test_wide_subspace(gpu_engine, cplx):
    """maxdim = 300 > 256: see krylov_cases.wide_subspace."""
    P, h = kc.wide_subspace(gpu_engine, cplx)
    assert P.stats.restarts >= 1


def test_bit_identical_runs_odd_order(gpu_engine):
    As = kc.mkmats1(257, 2, xpnd=1.05, seed=23, unit=True)
    kw = dict(mindim=6, maxdim=12, tol=1e-10, restarts=60, seed=9)
    kc.same_bits(*gpu_engine.partial_pschur(As, 4, "LM", **kw), *gpu_engine.partial_pschur(As, 4, "LM", **kw))
