"""GPU tier (MI355X): partial_pschur on sparse (CSR) factors — the SpMV kernel at every group width, the driver cases of
the simulated tier, the device-resident entry with torch sparse-CSR tensors (structure check on the device included),
run-to-run bit identity, and an order no dense factor could be stored at."""
import numpy as np
import pytest

import csr_cases as cc
import krylov_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def problem_300():
    """(300, 4, 8) real: CSR factors and dense copies, shared and left unchanged."""
    return cc.sparse_dominant(300, 4, 8, False, seed=312, dense=True)


def _torch_csr(Ss):
    import torch

    return [torch.sparse_csr_tensor(torch.from_numpy(np.asarray(s.indptr)),
                                    torch.from_numpy(np.asarray(s.indices, dtype=np.int64)),
                                    torch.from_numpy(np.asarray(s.data)), size=(s.n, s.n)).cuda() for s in Ss]


@pytest.mark.parametrize("cplx", [False, True])
def test_matvec_every_group_width(gpu_engine, cplx):
    for i, (name, csr) in enumerate(cc.matvec_cases(cplx)):
        worst = cc.check_matvec(gpu_engine, csr, cplx, seed=i)
        print(f"{name} cplx={cplx}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("shape", [(300, 4, 8, False), (300, 4, 8, True), (257, 3, 2, False)],
                         ids=["n300_p4_k8_d", "n300_p4_k8_z", "n257_p3_k2_d"])
def test_driver(gpu_engine, shape):
    n, p, k, cplx = shape
    Ss, Ds = cc.sparse_dominant(n, p, k, cplx, seed=n + p + k, dense=True)
    P, h = gpu_engine.partial_pschur(Ss, cc.NEV, "LM", **cc.DRIVER_KW)
    nconv = P.Z[0].shape[1]
    print(shape, h)
    assert nconv >= (cc.NEV >> 1), h  # (the acceptance rule of test/krylov.jl:58-117, as kc.pkstest)
    assert h.nconverged == nconv and h.nev == cc.NEV and h.converged == (nconv >= cc.NEV)
    assert h.mvproducts % p == 0 and h.mvproducts > 0
    kc.check(P, Ds, 1e-10)
    kc.check_values(P, kc.full_values(Ds), "LM", cc.NEV)
    kc.ev_check(gpu_engine, P, Ds)


def test_bit_identical_runs(gpu_engine, problem_300):
    Ss, _ = problem_300
    kc.same_bits(*gpu_engine.partial_pschur(Ss, cc.NEV, "LM", **cc.DRIVER_KW),
                 *gpu_engine.partial_pschur(Ss, cc.NEV, "LM", **cc.DRIVER_KW))


def test_device_resident_matches_host_entry(gpu_engine, problem_300):
    import torch

    Ss, Ds = problem_300
    Ph, hh = gpu_engine.partial_pschur(Ss, cc.NEV, "LM", **cc.DRIVER_KW)
    Pd, hd = gpu_engine.partial_pschur(_torch_csr(Ss), cc.NEV, "LM", **cc.DRIVER_KW)
    assert isinstance(Pd.Z[0], torch.Tensor) and Pd.Z[0].is_cuda
    kc.same_bits(Ph, hh, Pd, hd)
    kc.check(Ph, Ds, 1e-10)


def test_device_side_validation(gpu_engine, problem_300):
    """A column index equal to n through the `_dev` entry: the structure-check kernel (which reads rowptr and colind and
    gathers through neither) reports it, and no product is launched."""
    Ss, _ = problem_300
    ci = np.array(Ss[2].indices)
    ci[11] = Ss[2].n
    bad = _torch_csr(Ss[:2] + [Ss[2]._replace(indices=ci)] + Ss[3:])
    with pytest.raises(ValueError, match="column index"):
        gpu_engine.partial_pschur(bad, cc.NEV, "LM", **cc.DRIVER_KW)
    ip = np.array(Ss[1].indptr)
    ip[20], ip[21] = ip[21], ip[20]
    bad = _torch_csr([Ss[0], Ss[1]._replace(indptr=ip)] + Ss[2:])
    with pytest.raises(ValueError, match="row pointers"):
        gpu_engine.partial_pschur(bad, cc.NEV, "LM", **cc.DRIVER_KW)


def test_n200000_beyond_dense_storage(gpu_engine):
    """n = 200 000, p = 4, 16 entries per row beside the diagonal: the dense factors would take 1.3 TB.  Relation
    residuals and orthonormality as kc.check, with csr_matmat for the products and the Frobenius norm of the stored
    values as the bound of the 2-norm (as test_gpu_krylov.test_real_8192x8_device_resident)."""
    n, p, k, nev = 200000, 4, 16, 4
    Ss = cc.sparse_dominant(n, p, k, False, seed=77)
    P, h = gpu_engine.partial_pschur(Ss, nev, "LM", tol=1e-10, restarts=100, seed=4)
    print(h, P.stats.asdict())
    assert h.nconverged >= 2, h
    kk = P.Z[0].shape[1]
    lmax = float(np.max(np.abs(P.values)))
    for l in range(p):
        Zl, Zn = P.Z[l], P.Z[(l + 1) % p]
        res = float(np.max(np.linalg.norm(cc.csr_matmat(Ss[l], Zl) - Zn @ P.Ts[l], axis=0)))
        an = float(np.linalg.norm(Ss[l].data))
        bound = 1e3 * n * kc.EPS * an + (100 * 1e-10 * lmax if l == p - 1 else 0.0)
        assert res <= bound, (l, res, bound)
        orth = float(np.linalg.norm(Zl.T @ Zl - np.eye(kk)))
        assert orth < 100 * n * kc.EPS, (l, orth)
