"""GPU tier (MI355X): the dense Krylov kernels (csrc/psd_krylov.h) one by one through the diagnostic entries
psd_?_dense_matvec / psd_?_kr_orth / psd_?_kr_basis, against extended-precision numpy references (krylov_kernel_cases):
odd orders, tile and chunk edges, subspaces wider than a workgroup, and a factor pointer that is only 8-byte aligned."""
import numpy as np
import pytest

import krylov_kernel_cases as kk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cplx", [False, True])
def test_matvec_orders(gpu_engine, cplx):
    geoms, worst = [], 0.0
    for n in kk.MATVEC_ORDERS:
        w, g = kk.check_matvec(gpu_engine, n, cplx)
        geoms.append((n, g))
        worst = max(worst, w)
    # real: even orders ran psd_kr_mv<false, 2>, odd orders psd_kr_mv<false, 1> (asserted per order from the reported rp)
    kk.matvec_coverage(geoms, (1,) if cplx else (1, 2))
    print(f"matvec cplx={cplx}: worst err / bound = {worst:.3g}")


@pytest.mark.parametrize("n", [514, 1026])
def test_matvec_unaligned_device_pointer(gpu_engine, n):
    """The factor as psd_d_partial_pschur_dev may receive it: a view into a torch buffer at an odd element offset, 8-byte
    but not 16-byte aligned.  The entry must take the one-row body (the two-row body loads 16 bytes at a time), and the
    aligned view of the same matrix the two-row body; both meet the bound."""
    import torch

    A, x = kk.matvec_problem(n, False)
    ref, bound = kk.matvec_bound(A, x)
    buf = torch.zeros(n * n + 1, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    for shift, rp in ((0, 2), (1, 1)):
        store = buf[shift: shift + n * n].view(n, n)  # row-major storage of A^T = column-major A
        store.copy_(torch.from_numpy(np.ascontiguousarray(A.T)))
        dA = store.t()
        assert dA.data_ptr() % 16 == 8 * shift
        y, geom = gpu_engine.dense_matvec(dA, x)
        w = kk.check_matvec_result(y, geom, n, False, ref, bound, rp)
        print(f"matvec n={n} offset={shift}: rp={geom['rp']} worst err / bound = {w:.3g}")


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n,ncols", kk.ORTH_SHAPES)
def test_orth(gpu_engine, n, ncols, cplx):
    worst = {kind: kk.check_orth(gpu_engine, n, ncols, cplx, kind) for kind in kk.ORTH_KINDS}
    print(f"orth n={n} ncols={ncols} cplx={cplx}: worst err / bound = " + ", ".join(f"{k} {w:.3g}" for k, w in worst.items()))


@pytest.mark.parametrize("n,m,cplx", kk.BASIS_SHAPES)
def test_basis(gpu_engine, n, m, cplx):
    print(f"basis n={n} m={m} cplx={cplx}: worst err / bound = {kk.check_basis(gpu_engine, n, m, cplx):.3g}")
