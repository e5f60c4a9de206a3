"""CPU tier: the dense Krylov kernels (csrc/psd_krylov.h) one by one on the TEST-ONLY serial simulation, through the
diagnostic entries psd_?_dense_matvec / psd_?_kr_orth / psd_?_kr_basis, against extended-precision numpy references
(krylov_kernel_cases).  The simulation runs the lanes of a workgroup serially: it checks the index arithmetic, the guards
and the launch geometry of every case; the strided and barriered execution is the GPU tier's part."""
import ctypes as C

import numpy as np
import pytest

import krylov_kernel_cases as kk


def test_product_ld_matches_numpy():
    """The sliced extended-precision product agrees with numpy's longdouble product to the latter's own rounding."""
    rng = np.random.default_rng(0)
    for cplx in (False, True):
        V, Q = kk.randn(rng, (37, 300), cplx), kk.randn(rng, (300, 41), cplx)
        V[3] *= 1e-9
        V[4] = 0
        Q[:, 5] *= 1e12
        d = np.abs(kk.product_ld(V, Q) - kk.ld(V) @ kk.ld(Q))
        assert np.all(d <= 2.0 ** -58 * (np.abs(V) @ np.abs(Q)))


@pytest.mark.parametrize("cplx", [False, True])
def test_matvec_orders(sim_engine, cplx):
    geoms, worst = [], 0.0
    for n in kk.MATVEC_ORDERS:
        w, g = kk.check_matvec(sim_engine, n, cplx)
        geoms.append((n, g))
        worst = max(worst, w)
    # real: even orders ran psd_kr_mv<false, 2>, odd orders psd_kr_mv<false, 1> (asserted per order from the reported rp)
    kk.matvec_coverage(geoms, (1,) if cplx else (1, 2))
    print(f"matvec cplx={cplx}: worst err / bound = {worst:.3g}")


def test_matvec_in_place_alignment(sim_engine):
    """A factor read in place (device-pointer semantics; host memory is device memory here): a 16-byte aligned base
    takes the two-row body, the same matrix one element further the one-row body."""
    n = 514
    A, x = kk.matvec_problem(n, False)
    ref, bound = kk.matvec_bound(A, x)
    buf = np.zeros(n * n + 3)
    off = (-buf.ctypes.data // 8) % 2  # first 16-byte aligned element
    for shift, rp in ((0, 2), (1, 1)):
        view = buf[off + shift: off + shift + n * n].reshape((n, n), order="F")
        view[...] = A
        assert view.ctypes.data % 16 == 8 * shift
        y, geom = sim_engine.dense_matvec(view, x, in_place=True)
        kk.check_matvec_result(y, geom, n, False, ref, bound, rp)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n,ncols", kk.ORTH_SHAPES)
def test_orth(sim_engine, n, ncols, cplx):
    worst = {kind: kk.check_orth(sim_engine, n, ncols, cplx, kind) for kind in kk.ORTH_KINDS}
    print(f"orth n={n} ncols={ncols} cplx={cplx}: worst err / bound = " + ", ".join(f"{k} {w:.3g}" for k, w in worst.items()))


@pytest.mark.parametrize("n,m,cplx", kk.BASIS_SHAPES)
def test_basis(sim_engine, n, m, cplx):
    print(f"basis n={n} m={m} cplx={cplx}: worst err / bound = {kk.check_basis(sim_engine, n, m, cplx):.3g}")


def test_argument_codes(sim_engine):
    """The negative info values of the diagnostic entries, as listed in psd_mi355x.h."""
    eng = sim_engine
    lib, ctx = eng.lib, eng.ctx
    dp = C.POINTER(C.c_double)
    n = 4
    a, x, y = np.eye(n, order="F"), np.ones(n), np.zeros(n)
    pa, px, py = a.ctypes.data, x.ctypes.data_as(dp), y.ctypes.data_as(dp)
    info = C.c_int(0)

    def mv(ctx=ctx, n=n, A=pa, a_dev=0, x=px, y=py):
        rc = lib.psd_d_dense_matvec(ctx, n, A, a_dev, x, y, None, C.byref(info))
        assert rc == info.value
        return rc

    assert [mv(), mv(ctx=None), mv(n=0), mv(A=None), mv(a_dev=2), mv(x=None), mv(y=None)] == [0, -1, -2, -4, -8, -9, -17]
    assert np.array_equal(y, x)

    U, h, un = np.eye(n, 2, order="F"), np.zeros(2), np.zeros(n)
    hjj, st = C.c_double(0), (C.c_int32 * 4)()
    pu, ph, pn = U.ctypes.data_as(dp), h.ctypes.data_as(dp), un.ctypes.data_as(dp)

    def orth(ctx=ctx, n=n, ncols=2, U=pu, v=px, h=ph, hjj=C.byref(hjj), unew=pn, state=st):
        rc = lib.psd_d_kr_orth(ctx, n, ncols, U, v, h, hjj, unew, state, C.byref(info))
        assert rc == info.value
        return rc

    assert [orth(), orth(ctx=None), orth(n=0), orth(ncols=-1), orth(ncols=2049), orth(U=None), orth(v=None), orth(h=None),
            orth(hjj=None), orth(unew=None), orth(state=None)] == [0, -1, -2, -3, -3, -4, -5, -6, -7, -8, -9]
    assert orth(ncols=0, U=None, h=None) == 0

    V, Q, R = np.ones((n, 3), order="F"), np.eye(2, order="F"), C.c_int32(0)
    pv, pq = V.ctypes.data_as(dp), Q.ctypes.data_as(dp)

    def basis(ctx=ctx, n=n, p=1, cols=3, a0=1, m=2, V=pv, Q=pq):
        rc = lib.psd_d_kr_basis(ctx, n, p, cols, a0, m, V, Q, C.byref(R), C.byref(info))
        assert rc == info.value
        return rc

    assert [basis(), basis(ctx=None), basis(n=0), basis(p=0), basis(cols=0), basis(a0=-1), basis(m=0), basis(m=2049),
            basis(a0=2), basis(V=None), basis(Q=None)] == [0, -1, -2, -3, -4, -5, -6, -6, -6, -7, -8]
    assert R.value == 64
