"""Cases for the ComplexF64 SIGNED batched entries (Engine.zgphessenberg_batch_ / zgpschur_batch_ / zgpschur_batch /
zgpschur_hess_batch_ / gpschur_batch, and zpschur_batch(..., S=...)): many small complex problems of one shape and one
signature in one call.  Each case takes an engine; tests/test_hostsim_zgpschur_batch.py runs them on the serial
simulation, tests/test_gpu_zgpschur_batch.py on the device.  Factors come from pt.bench_factors(..., dtype=complex128),
I + G / (2 sqrt(n)): every factor is safely invertible, so every eigenvalue of the signed product is finite."""
import ctypes as C

import numpy as np
import pytest

import engine_cases as ec
import psd_amd
import psdtest as pt

T, F = True, False


def _sig22():
    return tuple([T] + [bool((5 * q + 1) % 3) for q in range(1, 22)])


# (nb, n, p, S for 'R') and the edge of the kernels each one covers; for 'L' the signature is reversed (true entry last)
SHAPES = [
    (3, 1, 3, (T, F, T)),       # n = 1: no sweep at all
    (4, 2, 2, (T, F)),          # smallest window, a pencil
    (5, 12, 3, (T, F, T)),      # one window
    (3, 40, 4, (T, F, F, T)),   # n > W; adjacent negative factors: both neighbour sides of stage 1, with and without the flip
    (3, 33, 4, (T, T, F, T)),   # a non-flipped factor with a flipped neighbour
    (2, 30, 22, _sig22()),      # p >= 20: zero-shift pass first
    (2, 14, 70, tuple(q % 2 == 0 for q in range(70))),  # W = 10: the LDS limit path
    (300, 3, 2, (T, F)),        # more workgroups than compute units
    (6, 20, 3, (T, T, F)),      # the group loop under PSD_BATCH_GROUP=4
]

_cache = {}
_refs = {}


def sig(shape, lr):
    S = list(shape[3])
    return S[::-1] if lr == "L" else S


def problems(shape):
    """The factors of a shape: built once, shared, never written to."""
    nb, n, p = shape[:3]
    key = (nb, n, p)
    if key not in _cache:
        probs = [pt.bench_factors(n, p, seed=7000 + 131 * q + 7 * n + p, dtype=np.complex128) for q in range(nb)]
        for A in probs:
            for a in A:
                a.setflags(write=False)
        _cache[key] = probs
    return _cache[key]


def reference(shape, q, lr):
    """The oracle's decomposition of problem q: computed once."""
    key = (shape, q, lr)
    if key not in _refs:
        po = pt.oracle_gpschur(work(problems(shape)[q]), sig(shape, lr), lr)
        assert po.info == 0
        _refs[key] = po
    return _refs[key]


def work(A):
    return [np.array(a, dtype=np.complex128, order="F", copy=True) for a in A]


def shape_id(s):
    return "nb%d_n%d_p%d" % s[:3]


def same_bits(a, b, p, what):
    assert np.array_equal(a.values, b.values, equal_nan=True), what
    for j in range(p):
        assert np.array_equal(a.Ts[j], b.Ts[j]), (what, j)
        if a.Z or b.Z:
            assert np.array_equal(a.Z[j], b.Z[j]), (what, j)


# ------------------------------------------------------------------------------------------------
# 1. reduction
def case_reduction(eng, shape):
    """zgphessenberg_batch_: pt.sg_hess_check per problem with the bounds of engine_cases.case_zg_phessenberg for the
    order (20 max(1, n/8) and 10 max(1, n/16))."""
    nb, n, p = shape[:3]
    S = sig(shape, "R")
    probs = problems(shape)
    Wb = [work(A) for A in probs]
    out, st = eng.zgphessenberg_batch_(Wb, S)
    assert len(out) == nb
    for q in range(nb):
        Hs, Qs = out[q]
        assert all(Hs[j] is Wb[q][j] for j in range(p))  # in place
        pt.sg_hess_check(probs[q], S, Hs, Qs, tol=20 * max(1, n / 8), qtol=10 * max(1, n / 16))
    noq, _ = eng.zgphessenberg_batch_([work(A) for A in probs], S, wantQ=False)
    for q in range(nb):
        assert noq[q][1] == [] and all(np.array_equal(noq[q][0][j], out[q][0][j]) for j in range(p))


def case_reduction_bits(eng, single_eng, shape):
    """Simulation: the batched reduction against gphessenberg_ with the serial stage 2 (PSD_HESS_SERIAL=1 in the
    environment of the single call): the same bodies in the same order, so H and Q are equal bit for bit."""
    nb, n, p = shape[:3]
    S = sig(shape, "R")
    probs = problems(shape)
    out, st = eng.zgphessenberg_batch_([work(A) for A in probs], S)
    for q in range(nb):
        H1, Q1 = single_eng.gphessenberg_(work(probs[q]), S)
        for j in range(p):
            assert np.array_equal(H1[j], out[q][0][j]), (shape_id(shape), q, j)
            assert np.array_equal(Q1[j], out[q][1][j]), (shape_id(shape), q, j)


# ------------------------------------------------------------------------------------------------
# 2. full decomposition
def check_problem(shape, q, ps, lr, A=None, S=None, ref=True):
    nb, n, p = shape[:3]
    A = problems(shape)[q] if A is None else A
    S = sig(shape, lr) if S is None else S
    assert ps.orientation == lr and ps.schurindex == (p if lr == "L" else 1) and ps.S == list(S)
    out = pt.gpschur_check(A, S, ps, tol=100 * max(1.0, np.sqrt(n / 32)), qtol=10 * max(1.0, np.sqrt(n / 32)))
    if ref:
        po = reference(shape, q, lr)
        err = pt.match_eigs(po.values, ps.values)
        bound = 1e-8 * max(1.0, abs(po.values).max())
        print(f"{shape_id(shape)} {lr} q={q}: resid {max(out['resid']):.2f} eps n, orth {max(out['orth']):.2f} eps n, "
              f"|lam - oracle| = {err:.3e} (bound {bound:.3e})")
        assert err < bound, (shape_id(shape), lr, q, err)


def case_full(eng, shape, lr):
    nb, n, p = shape[:3]
    S = sig(shape, lr)
    probs = problems(shape)
    batch = eng.zgpschur_batch(probs, S, lr)
    assert len(batch) == nb
    for q in range(nb):
        check_problem(shape, q, batch[q], lr)
    # nothing is shared between the problems of a batch: alone in a batch of one a problem gives the same bits
    for q in sorted({0, nb - 2, nb - 1} & set(range(nb))):
        alone = eng.zgpschur_batch([probs[q]], S, lr)[0]
        same_bits(alone, batch[q], p, (shape_id(shape), lr, q))
    assert all(not a.flags.writeable for A in probs for a in A)  # (the copying form left its input alone)


def case_above_cap(eng, n):
    """order cap + 1 (nb = 2, p = 2): the single call's reduction and iteration, problem by problem on the batch buffer"""
    shape = (2, n, 2, (T, F))
    case_full(eng, shape, "R")


# ------------------------------------------------------------------------------------------------
# 3. iteration against the single call (simulation: built without contraction, the same bodies give the same bits)
def case_iteration_bits(eng, single_eng, shape):
    """zgpschur_hess_batch_ on the reduced problems against zpschur_hess_(..., S) with the signed trains off, problem by
    problem: T, Z, the values and the sweep, zero-shift, Case II and Case III counts."""
    nb, n, p = shape[:3]
    S = sig(shape, "R")
    probs = problems(shape)
    red, _ = eng.zgphessenberg_batch_([work(A) for A in probs], S)
    reduced = [work(H) for H, _ in red]
    assert single_eng.get_train_g() == 0
    singles = [single_eng.zpschur_hess_(work(H)[0], work(H)[1:], S) for H in reduced]
    Wb = [work(H) for H in reduced]
    batch = eng.zgpschur_hess_batch_([(W[0], W[1:]) for W in Wb], S)
    for q in range(nb):
        same_bits(singles[q], batch[q], p, (shape_id(shape), q))
        assert batch[q].S == list(S)
    st = batch[0].stats
    for name in ("nsweeps", "nrqpass", "ndefl2", "ndefl1", "nwindows", "reserved", "niter"):
        assert getattr(st, name) == sum(getattr(s.stats, name) for s in singles), (shape_id(shape), name)
    assert st.nsweeps > 0 or n == 1
    if p >= 20:
        assert st.nrqpass > 0  # (the zero-shift pass came first)


def case_all_true(eng, shape=(5, 12, 3, (T, T, T))):
    """An all-true signature takes the path of zpschur_batch: the same bits, through every entry."""
    nb, n, p = shape[:3]
    probs = problems(shape)
    for lr in ("R", "L"):
        ref = eng.zpschur_batch(probs, lr)
        for got in (eng.zgpschur_batch(probs, [True] * p, lr), eng.zpschur_batch(probs, lr, S=[True] * p)):
            for q in range(nb):
                same_bits(ref[q], got[q], p, (lr, q))
    red, _ = eng.zphessenberg_batch_([work(A) for A in probs])
    Ha, Hb = [work(H) for H, _ in red], [work(H) for H, _ in red]
    a = eng.zpschur_hess_batch_([(H[0], H[1:]) for H in Ha])
    b = eng.zgpschur_hess_batch_([(H[0], H[1:]) for H in Hb], [True] * p)
    for q in range(nb):
        same_bits(a[q], b[q], p, ("hess", q))
    # and S dispatches to the signed path when it has a negative entry
    S = [True, False, True]
    g = eng.zpschur_batch(probs, "R", S=S)
    h = eng.zgpschur_batch(probs, S, "R")
    for q in range(nb):
        assert isinstance(g[q], psd_amd.GeneralizedPeriodicSchur) and g[q].S == S
        same_bits(g[q], h[q], p, ("dispatch", q))


# ------------------------------------------------------------------------------------------------
# 4. gpschur_batch
def _pairs(nb, n, ph, seed):
    As = [pt.bench_factors(n, ph, seed=seed + 17 * q, dtype=np.complex128) for q in range(nb)]
    Bs = [pt.bench_factors(n, ph, seed=seed + 17 * q + 5000, dtype=np.complex128) for q in range(nb)]
    return As, Bs


def case_gpschur_batch(eng):
    """One pair: the QZ problem of the pencil (A, B), against numpy's eigenvalues of B^-1 A at n = 6.  Bound
    1e-10 max(1, |lambda|max): both methods are backward stable (errors of a few n eps in A and B), B = I + G / (2 sqrt n)
    has a condition number below 10 and the eigenvalues of such a pencil condition numbers of order 10, so the
    difference is of order 1e-13; three digits are left for an unlucky draw.  Three pairs: against Engine.gpschur
    problem by problem within 1e-8 max(1, |lambda|max), the bound of engine_cases.case_zg_full (the single call runs
    trains and the pipelined stage 2, so it rounds differently)."""
    n = 6
    As, Bs = _pairs(4, n, 1, 300)
    out = eng.gpschur_batch(As, Bs)
    assert len(out) == 4
    for q in range(4):
        lam = np.linalg.eigvals(np.linalg.solve(Bs[q][0], As[q][0]))
        err = pt.match_eigs(lam, out[q].values)
        print(f"pencil q={q}: |lam - numpy| = {err:.3e} (bound {1e-10 * max(1.0, abs(lam).max()):.3e})")
        assert err < 1e-10 * max(1.0, abs(lam).max()), (q, err)
        assert out[q].S == [True, False] and out[q].period == 2
    As, Bs = _pairs(3, n, 3, 400)
    out = eng.gpschur_batch(As, Bs)
    for q in range(3):
        one = eng.gpschur(As[q], Bs[q])
        err = pt.match_eigs(one.values, out[q].values)
        print(f"three pairs q={q}: |lam - gpschur| = {err:.3e}")
        assert err < 1e-8 * max(1.0, abs(one.values).max()), (q, err)
        assert out[q].S == one.S and out[q].period == 6
        # the interleaving is gpschur's: the factors decompose the same sequence
        Cs = [As[q][2], Bs[q][1], As[q][1], Bs[q][0], As[q][0], Bs[q][2]]
        pt.gpschur_check(Cs, out[q].S, out[q])
    assert eng.gpschur_batch([], []) == []
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.gpschur_batch(As, Bs[:2])
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.gpschur_batch([As[0], As[1][:2]], [Bs[0], Bs[1][:2]])


# ------------------------------------------------------------------------------------------------
# 5. holes (Cases II and III)
HOLES = [(5, 5, tuple(S), l, j) for (S, l, j) in ec.RG_HOLES] + [(32, 4, (T, F, T, F), 2, 3), (40, 4, (T, T, F, T), 3, 30)]


def hole_id(h):
    return "n%d_p%d_%s_f%d_i%d" % (h[0], h[1], "".join("T" if s else "F" for s in h[2]), h[3], h[4])


def case_holes(eng, hole):
    """An exact zero on the diagonal of a triangular factor — of a +1 factor (Case II, a zero eigenvalue) or of a -1
    factor (Case III, an infinite one: beta == 0) — built as engine_cases.case_zg_holes builds it, in a batch between two
    untouched problems of the same shape.  The counts of finite values and of Cases II / III equal the oracle's, and the
    call's stats are the sums over the three problems."""
    n, p, S, fac, idx = hole
    S = list(S)
    seed = 1900 if n == 5 else 140 + n + p

    def make(sd):
        A = ec.zhess_ut(n, p, sd)
        if n > 5:
            A = [np.asfortranarray(a + 2 * np.eye(n)) if k > 0 else a for k, a in enumerate(A)]
        return A

    probs = [make(seed + 1000), make(seed), make(seed + 2000)]
    probs[1][fac - 1][idx - 1, idx - 1] = 0.0
    Wb = [work(A) for A in probs]
    out = eng.zgpschur_hess_batch_([(W[0], W[1:]) for W in Wb], S)
    c2 = c3 = 0
    for q in range(3):
        pt.gpschur_check(probs[q], S, out[q], tol=100 * max(1, n / 32))
        po = pt.oracle_zpschur_hess(probs[q][0], probs[q][1:], S)
        assert po.info == 0
        fin, gfin = np.isfinite(po.values), np.isfinite(out[q].values)
        assert fin.sum() == gfin.sum(), (hole, q)
        rtol = 1e-9 if n == 5 else 1e-8
        err = pt.match_eigs(po.values[fin], out[q].values[gfin])
        print(f"{hole_id(hole)} q={q}: finite {fin.sum()}/{n}, |lam - oracle| = {err:.3e} "
              f"(bound {rtol * max(1.0, abs(po.values[fin]).max()):.3e})")
        assert err < rtol * max(1.0, abs(po.values[fin]).max()), (hole, q, err)
        n2, n3 = int((po.sweeplog[:, 0] == 2).sum()), int((po.sweeplog[:, 0] == 3).sum())
        if q == 1:
            assert n2 + n3 >= 1, hole
            if S[fac - 1]:  # a zero in a +1 factor: a zero eigenvalue
                assert n2 >= 1 and np.any(out[q].values == 0), hole
            else:           # a zero in a -1 factor: an infinite eigenvalue
                assert n3 >= 1 and (out[q].beta == 0).sum() >= 1 and gfin.sum() < n, hole
        c2 += n2
        c3 += n3
    st = out[0].stats
    assert (st.reserved % 1000, st.reserved // 1000) == (c2, c3), (hole, st.reserved, c2, c3)
    assert st.ndefl2 == c2


# ------------------------------------------------------------------------------------------------
# 6. one failing problem
ONE_FAILS_SHAPE = (4, 24, 3, (T, F, T))


def one_fails_problems(n=24, p=3):
    """Three problems whose product needs a handful of sweeps — triangular factors with one 3 x 3 block in A_1 — around
    one full random problem (zbatch_cases.one_fails_problems with a signature)."""
    def easy(seed):
        A = [np.triu(a) for a in pt.bench_factors(n, p, seed=seed, dtype=np.complex128)]
        full = pt.bench_factors(n, 1, seed=seed + 977, dtype=np.complex128)[0]
        for k in (9, 10):
            A[0][k + 1, k] = full[k + 1, k]
        return [np.asfortranarray(a) for a in A]
    return [easy(41), pt.bench_factors(n, p, seed=42, dtype=np.complex128), easy(43), easy(44)]


def case_one_fails(eng):
    """maxitfac = 2, S = (T, F, T): the full problem exhausts its budget of 48 iterations and ends alone — the oracle's
    codes on these four inputs are (0, 16, 0, 0), after 36, 48, 32 and 33 iterations —; the other three are complete
    and correct."""
    S = list(ONE_FAILS_SHAPE[3])
    probs = one_fails_problems()
    infos = []
    out = eng.zgpschur_batch(probs, S, "R", maxitfac=2, infos_out=infos)
    assert len(infos) == 4 and infos[0] == 0 and infos[2] == 0 and infos[3] == 0, infos
    assert psd_amd.INFO_NOCONV <= infos[1] < psd_amd.INFO_NOTIMPL, infos
    for q in (0, 2, 3):
        check_problem(ONE_FAILS_SHAPE, q, out[q], "R", A=probs[q], S=S, ref=False)
        po = pt.oracle_gpschur(work(probs[q]), S, "R")
        assert po.info == 0
        assert pt.match_eigs(po.values, out[q].values) < 1e-8 * max(1.0, abs(po.values).max())
    Ws = [work(A) for A in probs]
    with pytest.raises(psd_amd.ConvergenceError):  # raised after all four have run
        eng.zgpschur_batch_(Ws, S, "R", maxitfac=2)
    for q in (0, 2, 3):  # ... so the in-place factors of the others are their T factors
        assert all(np.all(np.tril(w, -1) == 0) for w in Ws[q])
        assert all(np.array_equal(Ws[q][j], out[q].Ts[j]) for j in range(3))


# ------------------------------------------------------------------------------------------------
# 7. flags
def case_flags(eng, shape=SHAPES[2]):
    nb, n, p = shape[:3]
    probs = problems(shape)
    for lr in ("R", "L"):
        S = sig(shape, lr)
        full = eng.zgpschur_batch(probs, S, lr)
        noz = eng.zgpschur_batch(probs, S, lr, wantZ=False)
        not_ = eng.zgpschur_batch(probs, S, lr, wantZ=False, wantT=False)
        for q in range(nb):
            sc = max(1.0, abs(reference(shape, q, lr).values).max())
            assert noz[q].Z == [] and not_[q].Z == []
            assert pt.match_eigs(full[q].values, noz[q].values) < 1e-8 * sc
            assert pt.match_eigs(full[q].values, not_[q].values) < 1e-8 * sc
            for ps in (full[q], noz[q], not_[q]):
                assert ps.schurindex == (1 if lr == "R" else p) and ps.orientation == lr and ps.S == S
            for j in range(p):  # (without Z the factors still are the T factors)
                assert np.all(np.tril(noz[q].Ts[j], -1) == 0)
        W = work(probs[0])
        b1 = eng.zgpschur_batch_([W], S, lr)
        assert b1[0].Ts[0] is W[0]  # in place


# ------------------------------------------------------------------------------------------------
# 8. argument errors
def case_argument_errors(eng):
    A = problems(SHAPES[2])   # n = 12, p = 3
    B = problems(SHAPES[1])   # n = 2, p = 2
    S3, S2 = [T, F, T], [T, F]
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zgpschur_batch([A[0], B[0] + B[0][:1]], S3)  # unequal order
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zgpschur_batch([B[0], B[1][:1]], S2)  # unequal period
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zgpschur_batch(A, S2)  # one entry of S per factor
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zgphessenberg_batch_([work(a) for a in A], S2)
    with pytest.raises(psd_amd.DimensionMismatch):
        W = [work(a) for a in A]
        eng.zgpschur_hess_batch_([(w[0], w[1:]) for w in W], S2)
    with pytest.raises(ValueError):
        eng.zgpschur_batch(A, [F, T, T], "R")  # the leftmost entry must be true
    with pytest.raises(ValueError):
        eng.zgpschur_batch(A, [T, T, F], "L")
    with pytest.raises(ValueError):
        eng.zgphessenberg_batch_([work(a) for a in A], [F, T, T])
    with pytest.raises(ValueError):
        W = [work(a) for a in A]
        eng.zgpschur_hess_batch_([(w[0], w[1:]) for w in W], [F, T, T])
    with pytest.raises(ValueError):
        eng.zpschur_batch(A, "R", S=[F, T, T])
    with pytest.raises(TypeError):
        eng.zgpschur_batch_([[np.ascontiguousarray(a) for a in A[0]]], S3)  # in place needs Fortran order
    with pytest.raises(ValueError):
        eng.zgpschur_batch(A, S3, "X")
    real = [[np.asfortranarray(a.real.copy()) for a in A[0]]]
    with pytest.raises(TypeError):
        eng.zgpschur_batch(real, S3)
    with pytest.raises(TypeError):
        eng.zgpschur_batch_(real, S3)
    with pytest.raises(TypeError):
        eng.zgphessenberg_batch_(real, S3)
    with pytest.raises(TypeError):
        eng.zgpschur_hess_batch_([(real[0][0], real[0][1:])], S3)
    assert eng.zgpschur_batch([], S3) == [] and eng.zgpschur_batch_([], S3, "L") == []
    assert eng.zgpschur_hess_batch_([], S3) == [] and eng.zgphessenberg_batch_([], S3)[0] == []
    infos = [7]
    assert eng.zgpschur_batch([], S3, infos_out=infos) == [] and infos == []


def case_abi_codes(eng, shape=SHAPES[2]):
    """The argument codes of the four C entries (in the simulation device memory is host memory), and
    psd_z_gpschur_batch_dev on packed blocks against the host entry, bit for bit."""
    nb, n, p = shape[:3]
    probs = problems(shape)
    dp = C.POINTER(C.c_double)
    i32p = C.POINTER(C.c_int32)
    lib, ctx = eng.lib, eng.ctx

    def sarr(S):
        return (C.c_uint8 * len(S))(*[1 if x else 0 for x in S])

    for lr in ("R", "L"):
        S = sig(shape, lr)
        host = eng.zgpschur_batch(probs, S, lr)
        dA = np.ascontiguousarray(np.array([pt.pack(A, np.complex128) for A in probs]))
        dZ = np.zeros_like(dA)
        alpha, beta = np.zeros((nb, n), dtype=np.complex128), np.zeros((nb, n))
        sc = np.zeros((nb, n), dtype=np.int32)
        infos = (C.c_int * nb)()
        si, info = C.c_int(0), C.c_int(0)
        st = psd_amd.Stats()
        rc = lib.psd_z_gpschur_batch_dev(ctx, nb, n, p, C.c_void_p(dA.ctypes.data), sarr(S), lr.encode(), 1, 1, 30,
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
    al, be, sc1 = np.zeros(n, dtype=np.complex128), np.zeros(n), np.zeros(n, dtype=np.int32)
    ap, bp, sp = al.view(np.float64).ctypes.data_as(dp), be.ctypes.data_as(dp), sc1.ctypes.data_as(i32p)
    buf = C.c_void_p(dA.ctypes.data)
    SR, SL = sarr([T, F, T]), sarr([F, T, T])  # SL: leftmost in working order true for 'L' only

    def hess(nb_=1, n_=n, p_=p, A_=ptrs, S_=SR):
        return lib.psd_z_gphessenberg_batch(ctx, nb_, n_, p_, A_, S_, None, None, None)

    def host_(nb_=1, n_=n, p_=p, A_=ptrs, S_=SR, o=b"R", mi=30, wz=0, Z_=None, al_=ap, sc_=sp):
        return lib.psd_z_gpschur_batch(ctx, nb_, n_, p_, A_, S_, o, 1, wz, mi, Z_, al_, bp, sc_, None, None, None, None)

    def dev_(nb_=1, n_=n, p_=p, A_=buf, S_=SR, o=b"R", mi=30, wz=0, Z_=None, al_=ap, sc_=sp):
        return lib.psd_z_gpschur_batch_dev(ctx, nb_, n_, p_, A_, S_, o, 1, wz, mi, Z_, al_, bp, sc_, None, None, None, None)

    def hb_(nb_=1, n_=n, p_=p, H_=ptrs, S_=SR, mi=30, wz=0, Q_=None, al_=ap, sc_=sp):
        return lib.psd_z_gpschur_hess_batch(ctx, nb_, n_, p_, H_, S_, Q_, 1, wz, mi, al_, bp, sc_, None, None, None)

    assert hess(nb_=0) == -2 and hess(n_=0) == -3 and hess(p_=0) == -4 and hess(A_=None) == -5 and hess(S_=SL) == -7
    for f in (host_, dev_):
        assert f(nb_=0) == -2 and f(n_=0) == -3 and f(p_=0) == -4 and f(A_=None) == -5 and f(o=b"X") == -6
        assert f(S_=SL) == -7 and f(S_=SR, o=b"L") == 0 and f(S_=sarr([T, T, F]), o=b"L") == -7
        assert f(mi=0) == -9 and f(wz=1) == -10 and f(al_=None) == -11 and f(sc_=None) == -11
    assert hb_(nb_=0) == -2 and hb_(n_=0) == -3 and hb_(p_=0) == -4 and hb_(H_=None) == -5 and hb_(wz=1) == -6
    assert hb_(S_=SL) == -7 and hb_(mi=0) == -9 and hb_(al_=None) == -11 and hb_(sc_=None) == -11
    assert lib.psd_z_gphessenberg_batch(None, 1, n, p, ptrs, SR, None, None, None) == -1
    assert lib.psd_z_gpschur_batch(None, 1, n, p, ptrs, SR, b"R", 1, 0, 30, None, ap, bp, sp, None, None, None, None) == -1
    assert lib.psd_z_gpschur_batch_dev(None, 1, n, p, buf, SR, b"R", 1, 0, 30, None, ap, bp, sp, None, None, None, None) == -1
    assert lib.psd_z_gpschur_hess_batch(None, 1, n, p, ptrs, SR, None, 1, 0, 30, ap, bp, sp, None, None, None) == -1


# ------------------------------------------------------------------------------------------------
# 9. groups
def case_groups(make_engine, shape=SHAPES[8]):
    """A host entry whose batch does not fit the device at once works through it in groups (PSD_BATCH_GROUP lowers the
    group size): the same bits as in one group, problem by problem."""
    nb, n, p = shape[:3]
    probs = problems(shape)
    ref = make_engine({})
    eng = make_engine({"PSD_BATCH_GROUP": "4"})
    S = sig(shape, "L")
    whole = ref.zgpschur_batch(probs, S, "L")
    parts = eng.zgpschur_batch(probs, S, "L")
    for q in range(nb):
        same_bits(whole[q], parts[q], p, q)
    for name in ("nsweeps", "nwindows", "ndefl1", "niter"):
        assert getattr(whole[0].stats, name) == getattr(parts[0].stats, name), name
    S = sig(shape, "R")
    ob, _ = ref.zgphessenberg_batch_([work(A) for A in probs], S)
    op, _ = eng.zgphessenberg_batch_([work(A) for A in probs], S)
    for q in range(nb):
        assert all(np.array_equal(ob[q][0][j], op[q][0][j]) and np.array_equal(ob[q][1][j], op[q][1][j]) for j in range(p))
    Hb, Hp = [work(o[0]) for o in ob], [work(o[0]) for o in op]
    hb = ref.zgpschur_hess_batch_([(H[0], H[1:]) for H in Hb], S)
    hp = eng.zgpschur_hess_batch_([(H[0], H[1:]) for H in Hp], S)
    for q in range(nb):
        same_bits(hb[q], hp[q], p, ("hess", q))


# ------------------------------------------------------------------------------------------------
# 10. device-resident entry
def case_device_resident(eng, shape=SHAPES[2]):
    """One torch complex128 [nb, p, n, n] tensor through psd_z_gpschur_batch_dev: T, Z and the values equal the host
    entry's bit for bit (the same kernels on the same data; the entries differ in the copies alone)."""
    import torch

    nb, n, p = shape[:3]
    probs = problems(shape)
    for lr in ("R", "L"):
        S = sig(shape, lr)
        host = eng.zgpschur_batch(probs, S, lr)
        dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in probs])).cuda()
        assert dA.dtype == torch.complex128
        keep = dA.clone()
        Tt, Zt, values, st = eng.zgpschur_batch(dA, S, lr)
        assert isinstance(Tt, torch.Tensor) and Tt.is_cuda and Zt.is_cuda and tuple(Tt.shape) == (nb, p, n, n)
        assert torch.equal(dA, keep)  # the input stays as it was
        Th, Zh = Tt.cpu().numpy(), Zt.cpu().numpy()
        for q in range(nb):
            assert np.array_equal(values[q], host[q].values), (lr, q)
            for j in range(p):
                assert np.array_equal(Th[q, j], host[q].Ts[j]), (lr, q, j)
                assert np.array_equal(Zh[q, j], host[q].Z[j]), (lr, q, j)
    Tn, Zn, vn, _ = eng.zpschur_batch(dA, "R", wantZ=False, S=sig(shape, "R"))
    assert Zn is None
    for q in range(nb):
        po = reference(shape, q, "R")
        assert pt.match_eigs(po.values, vn[q]) < 1e-8 * max(1.0, abs(po.values).max())
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zgpschur_batch(dA[:, :, :, :5], sig(shape, "R"))
    with pytest.raises(TypeError):
        eng.zgpschur_batch(dA.real.contiguous(), sig(shape, "R"))
