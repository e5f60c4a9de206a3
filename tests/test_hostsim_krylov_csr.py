"""CPU tier: partial_pschur on sparse (CSR) factors, on the TEST-ONLY serial simulation of the device code
(tests/hostsim): the SpMV kernel of psd_csr.h pinned at every group width, the structure check, and the Krylov driver
through the CSR entry points against dense copies of the same factors and the CPU oracle's full spectrum."""
import ctypes as C

import numpy as np
import pytest

import csr_cases as cc
import krylov_cases as kc
import psd_amd


@pytest.fixture(scope="module")
def problems():
    """(n, p, k, cplx) -> (CSR factors, dense copies, full spectrum of the dense copies), built once and left unchanged."""
    out = {}
    for shape in cc.DRIVER_SHAPES:
        n, p, k, cplx = shape
        Ss, Ds = cc.sparse_dominant(n, p, k, cplx, seed=n + p + k, dense=True)
        out[shape] = (Ss, Ds, kc.full_values(Ds))
    return out


@pytest.mark.parametrize("cplx", [False, True])
def test_matvec_every_group_width(sim_engine, cplx):
    for i, (name, csr) in enumerate(cc.matvec_cases(cplx)):
        worst = cc.check_matvec(sim_engine, csr, cplx, seed=i)
        print(f"{name} cplx={cplx}: worst error / bound = {worst:.3f}")


def test_matvec_argument_codes(sim_engine):
    csr = cc.random_rows(9, 2, False, 1)
    x = np.ones(9)
    for g in (3, 128, -1):
        with pytest.raises(ValueError, match="group"):
            sim_engine.csr_matvec(csr, x, group=g)
    with pytest.raises(psd_amd.DimensionMismatch):
        sim_engine.csr_matvec(csr, np.ones(8))
    bad = csr._replace(indices=np.where(np.arange(18) == 7, 9, csr.indices).astype(np.int32))
    with pytest.raises(ValueError, match="column index"):
        sim_engine.csr_matvec(bad, x)


@pytest.mark.parametrize("shape", cc.DRIVER_SHAPES, ids=lambda s: "n%d_p%d_k%d_%s" % (s[0], s[1], s[2], "z" if s[3] else "d"))
def test_driver(sim_engine, problems, shape):
    Ss, Ds, vfull = problems[shape]
    P, h = sim_engine.partial_pschur(Ss, cc.NEV, "LM", **cc.DRIVER_KW)
    nconv = P.Z[0].shape[1]
    print(shape, h)
    assert nconv >= (cc.NEV >> 1), h  # (the acceptance rule of test/krylov.jl:58-117, as kc.pkstest)
    assert h.nconverged == nconv and h.nev == cc.NEV and h.converged == (nconv >= cc.NEV)
    assert h.mvproducts % len(Ss) == 0 and h.mvproducts > 0 and P.stats.nprods == h.mvproducts
    assert len(P.values) == nconv and P.schurindex == len(Ss) and P.orientation == "L"
    kc.check(P, Ds, 1e-10)
    kc.check_values(P, vfull, "LM", cc.NEV)
    kc.ev_check(sim_engine, P, Ds)


@pytest.mark.parametrize("shape", [cc.DRIVER_SHAPES[0], cc.DRIVER_SHAPES[1]], ids=["real", "complex"])
def test_sparse_and_dense_paths_agree(sim_engine, problems, shape):
    """The same problem and start vector through both operators: converged values are accurate to tol |lambda|, so they
    agree to 1e-8 relative; the bits differ (the sums are ordered differently)."""
    Ss, Ds, _ = problems[shape]
    n, cplx = shape[0], shape[3]
    rng = np.random.default_rng(8)
    u1 = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
    kw = dict(cc.DRIVER_KW, u1=u1)
    Ps, hs = sim_engine.partial_pschur(Ss, cc.NEV, "LM", **kw)
    Pd, hd = sim_engine.partial_pschur(Ds, cc.NEV, "LM", **kw)
    kc.check(Ps, Ds, 1e-10)
    kc.check(Pd, Ds, 1e-10)
    m = min(len(Ps.values), len(Pd.values))
    assert m >= (cc.NEV >> 1)
    for lam in Ps.values[:m]:
        assert np.min(np.abs(Pd.values - lam)) <= 1e-8 * abs(lam), (lam, Pd.values)


@pytest.mark.parametrize("which", ["LM", "SR"])
def test_full_csr_of_reference_problem(sim_engine, which):
    """test/krylov.jl's own problem with every entry stored."""
    As = kc.mkmats1(30, 3, seed=11)
    Ss = [cc.full_csr(a) for a in As]
    P, h = sim_engine.partial_pschur(Ss, 4, which, mindim=6, maxdim=12, tol=1e-10, restarts=60)
    assert P.Z[0].shape[1] >= 2, h
    kc.check(P, As, 1e-10)
    kc.check_values(P, kc.full_values(As), which, 4)


def test_bit_identical_runs(sim_engine, problems):
    Ss = problems[cc.DRIVER_SHAPES[2]][0]
    a = sim_engine.partial_pschur(Ss, cc.NEV, "LM", **cc.DRIVER_KW)
    b = sim_engine.partial_pschur(Ss, cc.NEV, "LM", **cc.DRIVER_KW)
    kc.same_bits(*a, *b)


def test_input_forms_and_errors(sim_engine, problems):
    Ss, Ds, _ = problems[cc.DRIVER_SHAPES[2]]
    eng = sim_engine
    ref = eng.partial_pschur(Ss, cc.NEV, "LM", **cc.DRIVER_KW)
    bare = [(s.indptr, s.indices.astype(np.int64), s.data) for s in Ss]  # bare triples, wide indices
    kc.same_bits(*ref, *eng.partial_pschur(bare, cc.NEV, "LM", **cc.DRIVER_KW))
    with pytest.raises(TypeError):
        eng.partial_pschur([Ss[0], Ds[1], Ss[2]], cc.NEV)
    small = cc.random_rows(5, 2, False, 0)
    with pytest.raises(psd_amd.DimensionMismatch, match="same \\(square\\) size"):
        eng.partial_pschur([Ss[0], small, Ss[2]], cc.NEV)
    n = Ss[0].n

    def broken(**kw):
        return [Ss[0], Ss[1]._replace(**kw), Ss[2]]

    ip = np.array(Ss[1].indptr)
    ip[4], ip[5] = ip[5], ip[4]
    with pytest.raises(ValueError, match="row pointers"):
        eng.partial_pschur(broken(indptr=ip), cc.NEV)
    ip = np.array(Ss[1].indptr)
    ip[0] = 1
    with pytest.raises(ValueError, match="row pointers"):
        eng.partial_pschur(broken(indptr=ip), cc.NEV)
    for badcol in (n, -1):
        ci = np.array(Ss[1].indices)
        ci[7] = badcol
        with pytest.raises(ValueError, match="column index"):
            eng.partial_pschur(broken(indices=ci), cc.NEV)


def _abi_csr(eng, n, p, nev=2, which=b"M", mindim=4, maxdim=6, u1=None, tol=1e-8, tol1=1e-14, restarts=10,
             purgebuffer=2, A="ok", T="ok", Z="ok", wr="ok", nconv="ok", dev=False, edit=None):
    """psd_d_partial_pschur_csr (or _csr_dev: in the simulation device memory is host memory) on p diagonal factors."""
    rps = [np.arange(n + 1, dtype=np.int64) for _ in range(p)]
    cis = [np.arange(max(n, 1), dtype=np.int32) for _ in range(p)]
    vls = [1.0 + np.arange(max(n, 1)) / max(n, 1) for _ in range(p)]
    if edit:
        edit(rps, cis, vls)
    Ts = [np.zeros((maxdim, maxdim)) for _ in range(p)]
    Zs = [np.zeros((n, maxdim)) for _ in range(p)] if not dev else [np.zeros((p, n, maxdim))]
    w = np.zeros(max(maxdim, 1))
    dp = C.POINTER(C.c_double)
    info, k = C.c_int(0), C.c_int(0)
    up = u1.ctypes.data_as(dp) if u1 is not None else None
    arrs = [eng._ptrs(x) for x in (rps, cis, vls)]
    if A == "null-array":
        arrs[1] = None
    elif A == "null-element":
        arrs[2][p - 1] = None
    elif A is None:
        arrs = [None, None, None]
    zarg = (C.c_void_p(Zs[0].ctypes.data) if dev else eng._ptrs(Zs)) if Z == "ok" else None
    st = psd_amd.KrylovStats()
    fn = eng.lib.psd_d_partial_pschur_csr_dev if dev else eng.lib.psd_d_partial_pschur_csr
    rc = fn(eng.ctx, n, p, *arrs, nev, which, mindim, maxdim, up, 0, tol, tol1, restarts, purgebuffer,
            C.byref(k) if nconv == "ok" else None, eng._ptrs(Ts) if T == "ok" else None, zarg,
            w.ctypes.data_as(dp) if wr == "ok" else None, w.ctypes.data_as(dp), C.byref(st), C.byref(info))
    assert rc == info.value
    return rc, st


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_abi_argument_codes(sim_engine, dev):
    """Every code of the dense entry (test_hostsim_krylov.test_abi_argument_codes) through the CSR entries, the NULL
    forms of -4, and the structure codes -19 / -20 (in the `_dev` entry from the check kernel, before any product)."""
    eng = sim_engine
    n, p = 8, 2

    def call(*a, **kw):
        return _abi_csr(eng, *a, dev=dev, **kw)[0]

    assert call(n, p) == 0
    assert call(0, p) == -2
    assert call(n, 0) == -3
    assert call(n, p, A=None) == -4
    assert call(n, p, A="null-array") == -4
    assert call(n, p, A="null-element") == -4
    assert call(n, p, nev=0) == -5
    assert call(n, p, which=b"X") == -6
    assert call(n, p, nev=5, mindim=4) == -7
    assert call(n, p, mindim=7, maxdim=6) == -7
    assert call(n, p, maxdim=17) == -7
    assert call(3000, 2, maxdim=2049) == -8
    assert call(n, p, u1=np.zeros(n)) == -9
    assert call(n, p, tol=0.0) == -11
    assert call(n, p, tol1=-1.0) == -12
    assert call(n, p, restarts=-1) == -13
    assert call(n, p, purgebuffer=-1) == -14
    assert call(n, p, nconv=None) == -15
    assert call(n, p, T=None) == -16
    assert call(n, p, Z=None) == -17
    assert call(n, p, wr=None) == -18

    def edit(which, i, v):
        def f(rps, cis, vls):
            (rps if which == "r" else cis)[1][i] = v
        return f

    for e, code in ((edit("r", 0, 1), -19), (edit("r", 3, 5), -19), (edit("r", n, -1), -19),
                    (edit("r", n, 2 ** 41), -19), (edit("c", 5, n), -20), (edit("c", 5, -1), -20)):
        rc, st = _abi_csr(eng, n, p, dev=dev, edit=e)
        assert rc == code, (rc, code)
        assert st.nprods == 0 and st.ms_arnoldi == 0.0  # no Krylov work


def test_scipy_objects(sim_engine, problems):
    sp = pytest.importorskip("scipy.sparse")
    Ss = problems[cc.DRIVER_SHAPES[2]][0]
    ref = sim_engine.partial_pschur(Ss, cc.NEV, "LM", **cc.DRIVER_KW)
    n = Ss[0].n
    forms = {"csr_matrix": [sp.csr_matrix((s.data, s.indices, s.indptr), shape=(n, n)) for s in Ss],
             "csr_array": [sp.csr_array((s.data, s.indices, s.indptr), shape=(n, n)) for s in Ss]}
    for name, As in forms.items():
        kc.same_bits(*ref, *sim_engine.partial_pschur(As, cc.NEV, "LM", **cc.DRIVER_KW))
    # csc -> .tocsr() sums repeated entries and sorts the columns: compare with the triple form of that same matrix
    csc = [sp.csc_matrix(a) for a in forms["csr_matrix"]]
    back = [a.tocsr() for a in csc]
    trip = [cc.CSR(n, a.indptr, a.indices, a.data) for a in back]
    kc.same_bits(*sim_engine.partial_pschur(trip, cc.NEV, "LM", **cc.DRIVER_KW),
                 *sim_engine.partial_pschur(csc, cc.NEV, "LM", **cc.DRIVER_KW))
