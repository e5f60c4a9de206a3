"""Cases for the ComplexF64 batched entries (Engine.zphessenberg_batch_ / zpschur_batch_ / zpschur_batch /
zpschur_hess_batch_): many small complex problems of one shape in one call.  Each case takes an engine;
tests/test_hostsim_zpschur_batch.py runs them on the serial simulation, tests/test_gpu_zpschur_batch.py on the device.
Factors come from pt.bench_factors(..., dtype=complex128)."""
import ctypes as C

import numpy as np
import pytest

import engine_cases as ec
import psd_amd
import psdtest as pt

# (nb, n, p) and the edge of the kernels each one covers
SHAPES = [
    (3, 1, 3),    # n = 1: no sweep at all
    (4, 2, 2),    # smallest window
    (3, 5, 1),    # p = 1: H_{m-1} is H_m
    (5, 12, 3),   # one window, n < W
    (3, 40, 4),   # n > W = 32: several windows per sweep, off-window roles on all three sides
    (2, 30, 22),  # p >= 20: zero-shift pass first (st.ziter = -1), W = 20 < n
    (2, 14, 70),  # W = 10, window image ~ 123 KB: the LDS limit path
    (300, 3, 2),  # more workgroups than compute units
    (6, 20, 3),   # the group loop under PSD_BATCH_GROUP=4
]

_cache = {}
_refs = {}


def problems(nb, n, p):
    """The factors of a shape: built once, shared, never written to."""
    key = (nb, n, p)
    if key not in _cache:
        probs = [pt.bench_factors(n, p, seed=9000 + 131 * q + 7 * n + p, dtype=np.complex128) for q in range(nb)]
        for A in probs:
            for a in A:
                a.setflags(write=False)
        _cache[key] = probs
    return _cache[key]


def reference(shape, q, lr):
    """(||P||_2, numpy's eigenvalues of the product, the oracle's eigenvalues) of problem q: computed once."""
    key = (shape, q, lr)
    if key not in _refs:
        A = problems(*shape)[q]
        P = pt.product(A, lr == "L")
        po = pt.oracle_zpschur(work(A), lr)
        assert po.info == 0
        _refs[key] = (np.linalg.norm(P, 2), np.linalg.eigvals(P), po.values.copy())
    return _refs[key]


def work(A):
    return [np.array(a, dtype=np.complex128, order="F", copy=True) for a in A]


def shape_id(s):
    return "nb%d_n%d_p%d" % s


# ------------------------------------------------------------------------------------------------
# 1. reduction
def case_reduction_bits(eng, shape):
    """zphessenberg_batch_ against phessenberg_ problem by problem: the same bodies in the same order, so the packed H
    (reflectors below the diagonal included) and tau are equal bit for bit."""
    nb, n, p = shape
    probs = problems(*shape)
    Wb = [work(A) for A in probs]
    out, st = eng.zphessenberg_batch_(Wb)
    assert len(out) == nb
    for q in range(nb):
        W1 = work(probs[q])
        H1, tau1, _ = eng.phessenberg_(W1)
        for j in range(p):
            assert np.array_equal(W1[j], Wb[q][j]), (shape, q, j)
            assert np.array_equal(H1[j], out[q][0][j]), (shape, q, j)
        assert np.array_equal(tau1, out[q][1]), (shape, q)


def _q_from_reflectors(Apacked, tau, first):
    """Q = H_1 ... H_{n-1} from LAPACK-style storage, H_c = I - tau_c v v' (householder.jl:190-205): the reflector of
    column c acts on rows c + first ... n - 1 (first = 1 for the Hessenberg factor, 0 for the triangular ones).  A
    complex reflector of a single row is not the identity."""
    n = Apacked.shape[0]
    Q = np.eye(n, dtype=np.complex128)
    for c in range(n - 2, -1, -1):
        r0 = c + first
        if r0 > n - 1:
            continue
        v = np.zeros(n, dtype=np.complex128)
        v[r0] = 1.0
        v[r0 + 1:] = Apacked[r0 + 1:, c]
        Q -= tau[c] * np.outer(v, v.conj() @ Q)
    return Q


def case_reduction_close(eng, shape):
    """For shapes whose single call rounds differently (look-ahead form, p >= 3 on the device): the checks and bounds of
    batch_cases.case_reduction_close with conjugate transposes — triu parts equal to 1e-13 ||A||, the Q_j of the batched
    reduction unitary to 10 eps n, and Q_j' A_j Q_{j+1} = H_j to 10 n eps ||A_j||_F."""
    nb, n, p = shape
    probs = problems(*shape)
    Wb = [work(A) for A in probs]
    out, st = eng.zphessenberg_batch_(Wb)
    for q in range(nb):
        A = probs[q]
        W1 = work(A)
        H1, tau1, _ = eng.phessenberg_(W1)
        anorm = max(np.linalg.norm(a, 2) for a in A)
        Hb, taub = out[q]
        for j in range(p):
            d = np.abs(Hb[j] - H1[j]).max()
            print(f"{shape} q={q} j={j}: |H_batch - H_single| = {d:.3e} (bound {1e-13 * anorm:.3e})")
            assert d <= 1e-13 * anorm, (shape, q, j, d)
        Qs = [_q_from_reflectors(Wb[q][j], taub[j], 1 if j == 0 else 0) for j in range(p)]
        for j in range(p):
            orth = np.linalg.norm(Qs[j].conj().T @ Qs[j] - np.eye(n))
            assert orth < 10 * pt.EPS * n, (shape, q, j, orth)
            res = np.linalg.norm(Qs[j].conj().T @ A[j] @ Qs[(j + 1) % p] - Hb[j])
            assert res < 10 * n * pt.EPS * np.linalg.norm(A[j]), (shape, q, j, res)


# ------------------------------------------------------------------------------------------------
# 2. full decomposition
def check_problem(shape, q, ps, lr, A=None, refs=True):
    nb, n, p = shape
    A = problems(*shape)[q] if A is None else A
    assert ps.orientation == lr and ps.schurindex == (p if lr == "L" else 1)
    pt.pschur_check(A, ps, tol=100 * max(1.0, np.sqrt(n / 32)), check_lam=False, real=False)
    if refs:
        sc, lam_np, lam_or = reference(shape, q, lr)
        e_np, e_or = pt.match_eigs(lam_np, ps.values), pt.match_eigs(lam_or, ps.values)
        print(f"{shape} {lr} q={q}: |lam - numpy| = {e_np:.3e}, |lam - oracle| = {e_or:.3e} (bound {1e-10 * sc:.3e})")
        assert e_np <= 1e-10 * sc, (shape, lr, q, e_np)
        assert e_or <= 1e-10 * sc, (shape, lr, q, e_or)
    for j, T in enumerate(ps.Ts):
        if j != ps.schurindex - 1:
            assert np.all(np.diag(T).imag == 0) and np.all(np.diag(T).real >= 0), (shape, lr, q, j)


def case_full(eng, shape, lr):
    nb, n, p = shape
    probs = problems(*shape)
    batch = eng.zpschur_batch(probs, lr)
    assert len(batch) == nb
    for q in range(nb):
        check_problem(shape, q, batch[q], lr)
    # nothing is shared between the problems of a batch: alone in a batch of one a problem gives the same bits
    for q in sorted({0, nb - 2, nb - 1} & set(range(nb))):
        alone = eng.zpschur_batch([probs[q]], lr)[0]
        assert np.array_equal(alone.values, batch[q].values), (shape, lr, q)
        for j in range(p):
            assert np.array_equal(alone.Ts[j], batch[q].Ts[j]), (shape, lr, q, j)
            assert np.array_equal(alone.Z[j], batch[q].Z[j]), (shape, lr, q, j)
    assert all(not a.flags.writeable for A in probs for a in A)  # (the copying form left its input alone)


# ------------------------------------------------------------------------------------------------
# 3. iteration against the single call (simulation: built with -ffp-contract=off, the same bodies give the same bits)
def case_iteration_bits(eng, single_eng, shape):
    """zpschur_hess_batch_ on the reduced problems against zpschur_hess_ with the trains off, problem by problem: T, Z,
    the values and the sweep, zero-shift and Case-II counts.

    single_eng: the engine of the single calls, created with PSD_C3=0.  The batched kernel chases a window with the
    one-wave chain (psd_zq_sweep_window without the rotation table), factor after factor; the single call's default is
    the scan chase of psd_zchase3.h, which forms the rotations of all factors of a position from a chain of 2 x 2
    products and agrees with the one-wave chain to rounding only.  With the scan chase off the single call runs the
    same bodies as the batched kernel, and the bits are equal."""
    nb, n, p = shape
    probs = problems(*shape)
    reduced = []
    for A in probs:
        Hs, _, _ = eng.phessenberg_(work(A))
        reduced.append([np.asfortranarray(h) for h in Hs])
    keep = single_eng.get_train_z()
    single_eng.set_train_z(0)
    try:
        singles = [single_eng.zpschur_hess_(work(H)[0], work(H)[1:]) for H in reduced]
    finally:
        single_eng.set_train_z(keep)
    Wb = [work(H) for H in reduced]
    batch = eng.zpschur_hess_batch_([(W[0], W[1:]) for W in Wb])
    for q in range(nb):
        assert np.array_equal(singles[q].values, batch[q].values, equal_nan=True), (shape, q)
        for j in range(p):
            assert np.array_equal(singles[q].Ts[j], batch[q].Ts[j]), (shape, q, j)
            assert np.array_equal(singles[q].Z[j], batch[q].Z[j]), (shape, q, j)
    st = batch[0].stats
    for name in ("nsweeps", "nrqpass", "ndefl2", "ndefl1", "nwindows"):
        assert getattr(st, name) == sum(getattr(s.stats, name) for s in singles), (shape, name)


# ------------------------------------------------------------------------------------------------
# 4. holes (Case II)
HOLES = [(5, 3, 2, 3), (32, 4, 2, 3), (40, 4, 3, 20)]  # (n, p, factor, index)


def case_holes(eng, hole):
    """An exact zero on the diagonal of a triangular factor (engine_cases.case_zholes), in a batch between two untouched
    problems of the same shape."""
    n, p, fac, idx = hole

    def make(seed):
        A = ec.zhess_ut(n, p, seed)
        if n > 32:
            A = [np.asfortranarray(a + 2 * np.eye(n)) if k > 0 else a for k, a in enumerate(A)]
        return A

    probs = [make(80 + p + n + 1000), make(80 + p + n), make(80 + p + n + 2000)]
    probs[1][fac - 1][idx - 1, idx - 1] = 0
    Wb = [work(A) for A in probs]
    out = eng.zpschur_hess_batch_([(W[0], W[1:]) for W in Wb])
    case2 = 0
    for q in range(3):
        pt.gpschur_check(probs[q], [True] * p, out[q], tol=100 * max(1, n / 32))
        po = pt.oracle_zpschur_hess(probs[q][0], probs[q][1:], [True] * p)
        fin = np.isfinite(po.values)
        err = pt.match_eigs(po.values[fin], out[q].values[fin])
        print(f"{hole} q={q}: |lam - oracle| = {err:.3e} (bound {1e-10 * abs(po.values[fin]).max():.3e})")
        assert err <= 1e-10 * abs(po.values[fin]).max(), (hole, q, err)
        nq = int((po.sweeplog[:, 0] == 2).sum())
        if q == 1:
            assert nq == 1, (hole, nq)  # (the oracle's count at the holed problem)
        case2 += nq
    # the call's stats are sums over its problems: the holed problem's count is what the untouched ones leave of it
    assert out[0].stats.ndefl2 == case2, (hole, out[0].stats.ndefl2, case2)


# ------------------------------------------------------------------------------------------------
# 5. one failing problem
ONE_FAILS_SHAPE = (4, 24, 3)


def one_fails_problems(n=24, p=3):
    """The complex analogue of batch_cases.one_fails_problems: three problems whose product needs a handful of sweeps —
    triangular factors with one 3 x 3 block in A_1 — around one full random problem."""
    def easy(seed):
        A = [np.triu(a) for a in pt.bench_factors(n, p, seed=seed, dtype=np.complex128)]
        full = pt.bench_factors(n, 1, seed=seed + 977, dtype=np.complex128)[0]
        for k in (9, 10):
            A[0][k + 1, k] = full[k + 1, k]
        return [np.asfortranarray(a) for a in A]
    return [easy(41), pt.bench_factors(n, p, seed=42, dtype=np.complex128), easy(43), easy(44)]


def case_one_fails(eng):
    """maxitfac = 2: the full problem exhausts its budget and ends alone (the oracle: codes (0, 15, 0, 0) after 34, 48, 32
    and 33 of 48 iterations); the other three are complete and correct."""
    probs = one_fails_problems()
    infos = []
    out = eng.zpschur_batch(probs, "R", maxitfac=2, infos_out=infos)
    assert len(infos) == 4 and infos[0] == 0 and infos[2] == 0 and infos[3] == 0, infos
    assert psd_amd.INFO_NOCONV <= infos[1] < psd_amd.INFO_NOTIMPL, infos
    for q in (0, 2, 3):
        check_problem(ONE_FAILS_SHAPE, q, out[q], "R", A=probs[q], refs=False)
        P = pt.product(probs[q])
        sc = np.linalg.norm(P, 2)
        po = pt.oracle_zpschur(work(probs[q]), "R")
        assert pt.match_eigs(np.linalg.eigvals(P), out[q].values) <= 1e-10 * sc
        assert pt.match_eigs(po.values, out[q].values) <= 1e-10 * sc
    Ws = [work(A) for A in probs]
    with pytest.raises(psd_amd.ConvergenceError):  # raised after all four have run
        eng.zpschur_batch_(Ws, "R", maxitfac=2)
    for q in (0, 2, 3):  # ... so the in-place factors of the others are their T factors
        assert np.all(np.tril(Ws[q][0], -1) == 0) and all(np.all(np.tril(w, -1) == 0) for w in Ws[q][1:])
        assert np.array_equal(Ws[q][0], out[q].Ts[0])


# ------------------------------------------------------------------------------------------------
# 6. flags
def case_flags(eng, shape=(5, 12, 3)):
    nb, n, p = shape
    probs = problems(*shape)
    for lr in ("R", "L"):
        full = eng.zpschur_batch(probs, lr)
        noz = eng.zpschur_batch(probs, lr, wantZ=False)
        not_ = eng.zpschur_batch(probs, lr, wantZ=False, wantT=False)
        for q in range(nb):
            sc = reference(shape, q, lr)[0]
            assert noz[q].Z == [] and not_[q].Z == []
            assert pt.match_eigs(full[q].values, noz[q].values) <= 1e-10 * sc
            assert pt.match_eigs(full[q].values, not_[q].values) <= 1e-10 * sc
            for ps in (full[q], noz[q], not_[q]):
                assert ps.schurindex == (1 if lr == "R" else p) and ps.orientation == lr
        W = work(probs[0])
        b1 = eng.zpschur_batch_([W], lr)
        assert b1[0].Ts[0] is W[0]  # in place


# ------------------------------------------------------------------------------------------------
# 7. argument errors
def case_argument_errors(eng):
    A = problems(3, 5, 1)
    B = problems(4, 2, 2)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zpschur_batch([A[0], B[0][:1]])  # unequal order
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zpschur_batch([B[0], B[1][:1]])  # unequal period
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zphessenberg_batch_([work(B[0]), work(A[0])])
    with pytest.raises(psd_amd.DimensionMismatch):
        W = [work(B[0]), work(A[0])]
        eng.zpschur_hess_batch_([(w[0], w[1:]) for w in W])
    with pytest.raises(TypeError):
        eng.zpschur_batch_([[np.ascontiguousarray(a) for a in B[0]]])  # in place needs Fortran order
    with pytest.raises(ValueError):
        eng.zpschur_batch(A, "X")
    real = [[np.asfortranarray(a.real.copy()) for a in A[0]]]
    with pytest.raises(TypeError):
        eng.zpschur_batch(real)
    with pytest.raises(TypeError):
        eng.zpschur_batch_(real)
    with pytest.raises(TypeError):
        eng.zphessenberg_batch_(real)
    with pytest.raises(TypeError):
        eng.zpschur_hess_batch_([(real[0][0], real[0][1:])])
    assert eng.zpschur_batch([]) == [] and eng.zpschur_batch_([], "L") == [] and eng.zpschur_hess_batch_([]) == []
    assert eng.zphessenberg_batch_([])[0] == []
    infos = [7]
    assert eng.zpschur_batch([], infos_out=infos) == [] and infos == []
    # the real family still refuses complex input
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.pschur_batch([A[0]])
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.pschur_batch_([work(A[0])])


def case_abi_codes(eng, shape=(5, 12, 3)):
    """The argument codes of the four C entries (in the simulation device memory is host memory), as
    batch_cases.case_dev_abi; and psd_z_pschur_batch_dev on packed blocks gives the host entry's bits."""
    nb, n, p = shape
    probs = problems(*shape)
    dp = C.POINTER(C.c_double)
    i32p = C.POINTER(C.c_int32)
    lib, ctx = eng.lib, eng.ctx
    for lr in ("R", "L"):
        host = eng.zpschur_batch(probs, lr)
        dA = np.ascontiguousarray(np.array([pt.pack(A, np.complex128) for A in probs]))
        dZ = np.zeros_like(dA)
        alpha, beta = np.zeros((nb, n), dtype=np.complex128), np.zeros((nb, n))
        sc = np.zeros((nb, n), dtype=np.int32)
        infos = (C.c_int * nb)()
        si, info = C.c_int(0), C.c_int(0)
        st = psd_amd.Stats()
        rc = lib.psd_z_pschur_batch_dev(ctx, nb, n, p, C.c_void_p(dA.ctypes.data), lr.encode(), 1, 1, 30,
                                        C.c_void_p(dZ.ctypes.data), alpha.view(np.float64).ctypes.data_as(dp),
                                        beta.ctypes.data_as(dp), sc.ctypes.data_as(i32p), infos, C.byref(si),
                                        C.byref(st), C.byref(info))
        assert rc == 0 and info.value == 0 and si.value == (p if lr == "L" else 1) and not any(infos)
        assert st.ms_total >= st.ms_hess >= 0 and st.nsweeps > 0
        for q in range(nb):
            assert np.array_equal(pt.gvalues(alpha[q], beta[q], sc[q]), host[q].values)
            for j in range(p):
                assert np.array_equal(dA[q, j].T, host[q].Ts[j]) and np.array_equal(dZ[q, j].T, host[q].Z[j])
    A = work(probs[0])
    ptrs = eng._ptrs(A)
    tau = np.zeros((p, n), dtype=np.complex128)
    al, be, sc1 = np.zeros(n, dtype=np.complex128), np.zeros(n), np.zeros(n, dtype=np.int32)
    ap, bp, sp = al.view(np.float64).ctypes.data_as(dp), be.ctypes.data_as(dp), sc1.ctypes.data_as(i32p)
    tp = tau.view(np.float64).ctypes.data_as(dp)
    buf = C.c_void_p(dA.ctypes.data)

    def hess(nb_=1, n_=n, p_=p, A_=ptrs, tau_=tp):
        return lib.psd_z_phessenberg_batch(ctx, nb_, n_, p_, A_, tau_, None, None)

    def host_(nb_=1, n_=n, p_=p, A_=ptrs, o=b"R", mi=30, wz=0, Z_=None, al_=ap, sc_=sp):
        return lib.psd_z_pschur_batch(ctx, nb_, n_, p_, A_, o, 1, wz, mi, Z_, al_, bp, sc_, None, None, None, None)

    def dev_(nb_=1, n_=n, p_=p, A_=buf, o=b"R", mi=30, wz=0, Z_=None, al_=ap, sc_=sp):
        return lib.psd_z_pschur_batch_dev(ctx, nb_, n_, p_, A_, o, 1, wz, mi, Z_, al_, bp, sc_, None, None, None, None)

    def hb_(nb_=1, n_=n, p_=p, H_=ptrs, mi=30, wz=0, Q_=None, al_=ap, sc_=sp):
        return lib.psd_z_pschur_hess_batch(ctx, nb_, n_, p_, H_, Q_, 1, wz, mi, al_, bp, sc_, None, None, None)

    assert hess(nb_=0) == -2 and hess(n_=0) == -3 and hess(p_=0) == -4 and hess(A_=None) == -5 and hess(tau_=None) == -6
    for f in (host_, dev_):
        assert f(nb_=0) == -2 and f(n_=0) == -3 and f(p_=0) == -4 and f(A_=None) == -5 and f(o=b"X") == -6
        assert f(mi=0) == -9 and f(wz=1) == -10 and f(al_=None) == -11 and f(sc_=None) == -11
    assert hb_(nb_=0) == -2 and hb_(n_=0) == -3 and hb_(p_=0) == -4 and hb_(H_=None) == -5 and hb_(wz=1) == -6
    assert hb_(mi=0) == -9 and hb_(al_=None) == -10 and hb_(sc_=None) == -10
    assert lib.psd_z_phessenberg_batch(None, 1, n, p, ptrs, tp, None, None) == -1
    assert lib.psd_z_pschur_batch(None, 1, n, p, ptrs, b"R", 1, 0, 30, None, ap, bp, sp, None, None, None, None) == -1
    assert lib.psd_z_pschur_batch_dev(None, 1, n, p, buf, b"R", 1, 0, 30, None, ap, bp, sp, None, None, None, None) == -1
    assert lib.psd_z_pschur_hess_batch(None, 1, n, p, ptrs, None, 1, 0, 30, ap, bp, sp, None, None, None) == -1


# ------------------------------------------------------------------------------------------------
# 8. groups
def case_groups(make_engine, shape=(6, 20, 3)):
    """A host entry whose batch does not fit the device at once works through it in groups (PSD_BATCH_GROUP lowers the
    group size): the same results as in one group, problem by problem."""
    nb, n, p = shape
    probs = problems(*shape)
    ref = make_engine({})
    eng = make_engine({"PSD_BATCH_GROUP": "4"})
    whole = ref.zpschur_batch(probs, "L")
    parts = eng.zpschur_batch(probs, "L")
    for q in range(nb):
        assert np.array_equal(whole[q].values, parts[q].values)
        for j in range(p):
            assert np.array_equal(whole[q].Ts[j], parts[q].Ts[j]) and np.array_equal(whole[q].Z[j], parts[q].Z[j])
    Wb, Wp = [work(A) for A in probs], [work(A) for A in probs]
    ob, _ = ref.zphessenberg_batch_(Wb)
    op, _ = eng.zphessenberg_batch_(Wp)
    for q in range(nb):
        assert np.array_equal(ob[q][1], op[q][1]) and all(np.array_equal(Wb[q][j], Wp[q][j]) for j in range(p))
    Hb, Hp = [work(o[0]) for o in ob], [work(o[0]) for o in op]
    hb = ref.zpschur_hess_batch_([(H[0], H[1:]) for H in Hb])
    hp = eng.zpschur_hess_batch_([(H[0], H[1:]) for H in Hp])
    for q in range(nb):
        assert np.array_equal(hb[q].values, hp[q].values)
        assert all(np.array_equal(Hb[q][j], Hp[q][j]) and np.array_equal(hb[q].Z[j], hp[q].Z[j]) for j in range(p))


# ------------------------------------------------------------------------------------------------
# 9. device-resident entry
def case_device_resident(eng, shape=(5, 12, 3)):
    """One torch complex128 [nb, p, n, n] tensor through psd_z_pschur_batch_dev: T, Z and the values equal the host
    entry's to 1e-12 relative (the same kernels on the same data; the entries differ in the copies alone)."""
    import torch

    nb, n, p = shape
    probs = problems(*shape)
    for lr in ("R", "L"):
        host = eng.zpschur_batch(probs, lr)
        dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in probs])).cuda()
        assert dA.dtype == torch.complex128
        keep = dA.clone()
        T, Z, values, st = eng.zpschur_batch(dA, lr)
        assert isinstance(T, torch.Tensor) and T.is_cuda and Z.is_cuda and tuple(T.shape) == (nb, p, n, n)
        assert torch.equal(dA, keep)  # the input stays as it was
        Th, Zh = T.cpu().numpy(), Z.cpu().numpy()
        for q in range(nb):
            sc = max(np.linalg.norm(a, 2) for a in probs[q])
            assert np.abs(values[q] - host[q].values).max() <= 1e-12 * np.abs(host[q].values).max()
            for j in range(p):
                assert np.abs(Th[q, j] - host[q].Ts[j]).max() <= 1e-12 * sc, (lr, q, j)
                assert np.abs(Zh[q, j] - host[q].Z[j]).max() <= 1e-12, (lr, q, j)
            ps = psd_amd.PeriodicSchur([np.asfortranarray(Th[q, j]) for j in range(p)],
                                       [np.asfortranarray(Zh[q, j]) for j in range(p)], values[q], lr,
                                       p if lr == "L" else 1)
            check_problem(shape, q, ps, lr)
    Tn, Zn, vn, _ = eng.zpschur_batch(dA, "R", wantZ=False)
    assert Zn is None
    for q in range(nb):
        assert pt.match_eigs(reference(shape, q, "R")[2], vn[q]) <= 1e-10 * reference(shape, q, "R")[0]
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zpschur_batch(dA[:, :, :, :5])
    with pytest.raises(TypeError):
        eng.zpschur_batch(dA.real.contiguous())
