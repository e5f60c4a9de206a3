"""GPU tier (MI355X): eigvecs(ps, select; shifted, method="backsub") — periodic back-substitution on the device
(csrc/psd_evec.h): the cases of the simulated tier, all vectors of 512 x 16 problems from pschur_dev through eigvecs_dev
checked by torch products on the device, and run-to-run bit identity."""
import numpy as np
import pytest

import evec_cases as vc
import psdtest as pt

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("p", [1, 5])
def test_vectors_jl_problems(gpu_engine, cplx, p):
    vc.case_vectors_jl(gpu_engine, cplx, p)


@pytest.mark.parametrize("cplx", [False, True])
def test_agrees_with_ordschur(gpu_engine, cplx):
    vc.case_vs_ordschur(gpu_engine, cplx)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_conjugate_pairs(gpu_engine, lr):
    vc.case_pairs(gpu_engine, lr)


def test_negative_eigenvalue_even_period(gpu_engine):
    vc.case_negative_even_p(gpu_engine)


@pytest.mark.parametrize("cplx", [False, True])
def test_repeated_eigenvalues(gpu_engine, cplx):
    vc.case_repeated(gpu_engine, cplx)


@pytest.mark.parametrize("cplx", [False, True])
def test_zero_eigenvalue(gpu_engine, cplx):
    vc.case_zero(gpu_engine, cplx)


def test_argument_errors(gpu_engine):
    vc.case_errors(gpu_engine)


@pytest.mark.parametrize("cplx", [False, True])
def test_several_chunks(gpu_engine, cplx):
    vc.case_chunks(gpu_engine, cplx)


def test_rescaled_columns(gpu_engine):
    vc.case_rescale(gpu_engine)


@pytest.mark.parametrize("cplx", [False, True])
def test_partial_schur(gpu_engine, cplx):
    vc.case_partial(gpu_engine, cplx)


def _device_problem(eng, n, p, cplx, seed):
    """pschur_dev on bench factors kept on the device; returns (kept A, T, Z, values, schurindex)"""
    import torch

    dt = np.complex128 if cplx else np.float64
    As = pt.bench_factors(n, p, seed=seed, dtype=dt)
    dA = torch.from_numpy(pt.pack(As, dt)).to("cuda:0")
    A0 = dA.clone()
    dZ = torch.zeros_like(dA)
    torch.cuda.synchronize()
    fn = eng.zpschur_dev if cplx else eng.pschur_dev
    lam, si, _, _ = fn(dA.data_ptr(), n, p, "L", dZ_ptr=dZ.data_ptr())
    return A0, dA, dZ, lam, si


def _device_ratio(A0, Vs, lam):
    """max over l, k of ||A_l v_l - mu v_{l+1}|| / (||A_l||_F ||v_l||) by torch on the device (A_l = A0[l].T)"""
    import torch

    p = A0.shape[0]
    mu = torch.as_tensor(np.asarray(lam, dtype=np.complex128) ** (1.0 / p), device=A0.device)
    worst = 0.0
    for l in range(p):
        A = A0[l].transpose(0, 1).to(torch.complex128)
        res = A @ Vs[l] - Vs[(l + 1) % p] * mu[None, :]
        r = torch.linalg.vector_norm(res, dim=0) / (torch.linalg.matrix_norm(A) * torch.linalg.vector_norm(Vs[l], dim=0))
        worst = max(worst, r.max().item())
    return worst


@pytest.mark.parametrize("cplx", [False, True])
def test_all_vectors_512x16_device_resident(gpu_engine, cplx):
    n, p = 512, 16
    A0, dT, dZ, lam, si = _device_problem(gpu_engine, n, p, cplx, seed=71 + cplx)
    T0, Z0 = dT.clone(), dZ.clone()
    Vs = gpu_engine.eigvecs_dev(dT, dZ, lam, [True] * n, lr="L", schurindex=si)
    st = gpu_engine.eigvecs_stats
    assert st.nvec == n and st.nzero == 0
    assert len(Vs) == p and tuple(Vs[0].shape) == (n, n)
    r = _device_ratio(A0, Vs, lam)
    print(f"512x16 {'ComplexF64' if cplx else 'Float64'}: worst relation ratio {r:.2e}, {st.ms_kernels:.1f} ms")
    assert r <= vc.GATE, r
    assert bool((dT == T0).all()) and bool((dZ == Z0).all())  # the factors are not modified
    V1 = gpu_engine.eigvecs_dev(dT, dZ, lam, [True] * n, lr="L", schurindex=si, shifted=False)
    assert len(V1) == 1 and bool((V1[0] == Vs[0]).all())


def test_bit_identical_runs(gpu_engine):
    n, p = 256, 8
    _, dT, dZ, lam, si = _device_problem(gpu_engine, n, p, False, seed=81)
    sel = [i % 3 != 1 for i in range(n)]
    a = gpu_engine.eigvecs_dev(dT, dZ, lam, sel, lr="L", schurindex=si)
    b = gpu_engine.eigvecs_dev(dT, dZ, lam, sel, lr="L", schurindex=si)
    for x, y in zip(a, b):
        assert bool((x == y).all())

