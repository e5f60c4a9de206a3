"""GPU tier (MI355X): geigvecs — eigenvectors of signed and singular periodic products on the device
(csrc/psd_gevec.h): the cases of the simulated tier, all vectors of 512 x 16 signed problems through geigvecs_dev checked
by torch products on the device, and run-to-run bit identity."""
import numpy as np
import pytest

import gevec_cases as gc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("spat", ["alt", "tfft"])
@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("cplx", [False, True])
def test_signed_forms(gpu_engine, cplx, lr, spat):
    gc.case_signed(gpu_engine, cplx, lr, spat)


@pytest.mark.parametrize("cplx", [False, True])
def test_end_to_end_signed(gpu_engine, cplx):
    gc.case_end_to_end(gpu_engine, cplx)


@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("cplx", [False, True])
def test_zero_and_infinite_eigenvalues(gpu_engine, cplx, lr):
    gc.case_zero_infinite(gpu_engine, cplx, lr)


@pytest.mark.parametrize("cplx", [False, True])
def test_periodic_schur_zero_eigenvalue(gpu_engine, cplx):
    gc.case_plain_zero(gpu_engine, cplx)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_conjugate_pairs(gpu_engine, lr):
    gc.case_pairs(gpu_engine, lr)


@pytest.mark.parametrize("cplx", [False, True])
def test_pair_across_chunks(gpu_engine, cplx):
    gc.case_chunk_pair(gpu_engine, cplx)


@pytest.mark.parametrize("cplx", [False, True])
def test_repeated_eigenvalues(gpu_engine, cplx):
    gc.case_repeated(gpu_engine, cplx)


def test_rescaled_columns(gpu_engine):
    gc.case_rescale(gpu_engine)


@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("cplx", [False, True])
def test_all_true_matches_eigvecs(gpu_engine, cplx, lr):
    gc.case_vs_eigvecs(gpu_engine, cplx, lr)


def test_argument_errors(gpu_engine):
    gc.case_errors(gpu_engine)


def device_problem(n, p, cplx, seed, S=None):
    """a signed Schur form of n x n factors (alternating S), uploaded: (P, dA, dT, dZ) with the [p][n][n] column-major
    blocks the _dev entry points take (A kept for the checks)"""
    import torch

    S = gc.S_ALT(p) if S is None else S
    rs = np.random.RandomState(seed)
    diag = [(0.5 + rs.rand(n)) * np.where(rs.rand(n) < 0.3, -1, 1) for _ in range(p)]
    P, As = gc.signed_form(n, p, S, "L", diag=diag, seed=seed, cplx=cplx, pairs=() if cplx else tuple(range(3, n - 1, 37)),
                           si=p - 1)
    tt = torch.complex128 if cplx else torch.float64
    up = lambda ms: torch.stack([torch.from_numpy(np.ascontiguousarray(m.T)) for m in ms]).to(tt).to("cuda:0")  # noqa
    return P, up(As), up(P.Ts), up(P.Z)


def device_ratio(dA, S, Vs, a):
    """max over l, j of ||lhs - rhs|| / (||A_l||_F ||v|| + |a_l| ||v'||) by torch on the device (A_l = dA[l].T)"""
    import torch

    p = dA.shape[0]
    da = torch.as_tensor(a, device=dA.device)
    worst = 0.0
    for l in range(p):
        A = dA[l].transpose(0, 1).to(torch.complex128)
        x, y = Vs[l], Vs[(l + 1) % p]
        if not S[l]:
            x, y = y, x
        res = A @ x - y * da[l][None, :]
        den = (torch.linalg.matrix_norm(A) * torch.linalg.vector_norm(x, dim=0)
               + da[l].abs() * torch.linalg.vector_norm(y, dim=0))
        worst = max(worst, (torch.linalg.vector_norm(res, dim=0) / den).max().item())
    return worst


@pytest.mark.parametrize("cplx", [False, True])
def test_all_vectors_512x16_signed_device_resident(gpu_engine, cplx):
    n, p = 512, 16
    P, dA, dT, dZ = device_problem(n, p, cplx, seed=71 + cplx)
    T0, Z0 = dT.clone(), dZ.clone()
    Vs, a = gpu_engine.geigvecs_dev(dT, dZ, [True] * n, "L", P.schurindex, S=P.S)
    st = gpu_engine.eigvecs_stats
    assert st.nvec == n and st.nzero == 0
    assert len(Vs) == p and tuple(Vs[0].shape) == (n, n) and a.shape == (p, n)
    r = device_ratio(dA, P.S, Vs, a)
    print(f"512x16 signed {'ComplexF64' if cplx else 'Float64'}: worst relation ratio {r:.2e}, {st.ms_kernels:.1f} ms")
    assert r <= gc.GATE, r
    assert bool((dT == T0).all()) and bool((dZ == Z0).all())  # the factors are not modified
    V1, a1 = gpu_engine.geigvecs_dev(dT, dZ, [True] * n, "L", P.schurindex, S=P.S, shifted=False)
    assert len(V1) == 1 and bool((V1[0] == Vs[0]).all()) and np.array_equal(a1, a)


def test_bit_identical_runs(gpu_engine):
    n, p = 256, 8
    P, _, dT, dZ = device_problem(n, p, False, seed=81)
    sel = [i % 3 != 1 for i in range(n)]
    x, ax = gpu_engine.geigvecs_dev(dT, dZ, sel, "L", P.schurindex, S=P.S)
    y, ay = gpu_engine.geigvecs_dev(dT, dZ, sel, "L", P.schurindex, S=P.S)
    assert np.array_equal(ax, ay)
    for u, v in zip(x, y):
        assert bool((u == v).all())
