"""Cases for the Float64 SIGNED batched entries (Engine.dgphessenberg_batch_ / dgpschur_batch_ / dgpschur_batch /
dgpschur_hess_batch_, and gpschur_batch(..., real=True)): many small real problems of one shape and one signature in
one call.  Each case takes an engine; tests/test_hostsim_dgpschur_batch.py runs them on the serial simulation,
tests/test_gpu_dgpschur_batch.py on the device.  Factors come from pt.bench_factors (Float64), I + G / (2 sqrt(n)): every
factor is safely invertible, so every eigenvalue of the signed product is finite, and random real factors give both real
eigenvalues and conjugate pairs."""
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
    (4, 2, 2, (T, F)),          # the smallest problem: a single 2 x 2 block of a pencil
    (5, 12, 3, (T, F, T)),      # one window
    (3, 40, 4, (T, F, F, T)),   # n > W; adjacent negative factors: both neighbour sides of stage 1, with and without the flip
    (3, 33, 4, (T, T, F, T)),   # a non-flipped factor with a flipped neighbour, odd order
    (2, 30, 22, _sig22()),      # p >= 20: zero-shift pass first, window below 32
    (2, 20, 70, tuple(q % 2 == 0 for q in range(70))),  # W = 16 for 8-byte elements: the LDS limit path, n above it
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
        probs = [pt.bench_factors(n, p, seed=9000 + 131 * q + 7 * n + p) for q in range(nb)]
        for A in probs:
            for a in A:
                a.setflags(write=False)
        _cache[key] = probs
    return _cache[key]


def reference(shape, q, lr, S=None):
    """The oracle's decomposition of problem q: computed once."""
    S = sig(shape, lr) if S is None else list(S)
    key = (shape[:3], tuple(S), q, lr)
    if key not in _refs:
        po = pt.oracle_gpschur(work(problems(shape)[q]), S, lr)
        assert po.info == 0
        _refs[key] = po
    return _refs[key]


def work(A):
    return [np.array(a, dtype=np.float64, order="F", copy=True) for a in A]


def shape_id(s):
    return "nb%d_n%d_p%d" % s[:3]


def same_bits(a, b, p, what):
    """T, Z, alpha, beta and the scaling of two decompositions, bit for bit"""
    assert np.array_equal(a.alpha, b.alpha, equal_nan=True), what
    assert np.array_equal(a.beta, b.beta, equal_nan=True), what
    assert np.array_equal(a.alphascale, b.alphascale), what
    assert np.array_equal(a.values, b.values, equal_nan=True), what
    for j in range(p):
        assert np.array_equal(a.Ts[j], b.Ts[j]), (what, j)
        if a.Z or b.Z:
            assert np.array_equal(a.Z[j], b.Z[j]), (what, j)


def real_form(ps, what):
    """What the real entries promise beyond the complex ones: real Ts and Z, T at schurindex quasi-triangular with a zero
    sub-diagonal wherever the eigenvalue is real, the others triangular, the values of a 2 x 2 block exact conjugates."""
    n = ps.Ts[0].shape[0]
    assert all(t.dtype == np.float64 for t in ps.Ts) and all(z.dtype == np.float64 for z in ps.Z), what
    assert isinstance(ps, psd_amd.GeneralizedPeriodicSchur), what
    js = ps.schurindex - 1
    for l, t in enumerate(ps.Ts):
        assert np.all(np.tril(t, -2 if l == js else -1) == 0), (what, l)
    sub = np.diag(ps.Ts[js], -1) if n > 1 else np.zeros(0)
    i = 0
    while i < n:
        if i + 1 < n and sub[i] != 0:
            assert i + 2 >= n or sub[i + 1] == 0, (what, i)  # (blocks do not overlap)
            assert ps.values[i].imag != 0 and ps.values[i + 1] == np.conj(ps.values[i]), (what, i, ps.values[i:i + 2])
            i += 2
        else:
            assert ps.values[i].imag == 0 or not np.isfinite(ps.values[i]), (what, i, ps.values[i])
            i += 1


# ------------------------------------------------------------------------------------------------
# 1. reduction
def case_reduction(eng, shape):
    """dgphessenberg_batch_: pt.sg_hess_check per problem with the bounds of engine_cases.case_rg_phessenberg for the
    order (20 max(1, n/8) and 10 max(1, n/16)); wantQ=False gives the same H."""
    nb, n, p = shape[:3]
    S = sig(shape, "R")
    probs = problems(shape)
    Wb = [work(A) for A in probs]
    out, st = eng.dgphessenberg_batch_(Wb, S)
    assert len(out) == nb
    for q in range(nb):
        Hs, Qs = out[q]
        assert all(Hs[j] is Wb[q][j] for j in range(p))  # in place
        assert all(h.dtype == np.float64 for h in Hs) and all(x.dtype == np.float64 for x in Qs)
        pt.sg_hess_check(probs[q], S, Hs, Qs, tol=20 * max(1, n / 8), qtol=10 * max(1, n / 16))
    noq, _ = eng.dgphessenberg_batch_([work(A) for A in probs], S, wantQ=False)
    for q in range(nb):
        assert noq[q][1] == [] and all(np.array_equal(noq[q][0][j], out[q][0][j]) for j in range(p))


def case_reduction_bits(eng, single_eng, shape):
    """Simulation: the batched reduction against gphessenberg_ with the serial stage 2 (PSD_HESS_SERIAL=1 in the
    environment of the single call): the same bodies in the same order, so H and Q are equal bit for bit."""
    nb, n, p = shape[:3]
    S = sig(shape, "R")
    probs = problems(shape)
    out, st = eng.dgphessenberg_batch_([work(A) for A in probs], S)
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
    what = (shape_id(shape), lr, q)
    assert ps.orientation == lr and ps.schurindex == (p if lr == "L" else 1) and ps.S == list(S), what
    pt.rgpschur_check(A, S, ps, tol=100 * max(1.0, np.sqrt(n / 32)), qtol=10 * max(1.0, np.sqrt(n / 32)))
    real_form(ps, what)
    if ref:
        po = reference(shape, q, lr, S)
        err = pt.match_eigs(po.values, ps.values)
        bound = 1e-8 * max(1.0, abs(po.values).max())
        print(f"{shape_id(shape)} {lr} q={q}: |lam - oracle| = {err:.3e} (bound {bound:.3e}), "
              f"{int((ps.values.imag > 0).sum())} pairs")
        assert err < bound, (what, err)


def case_full(eng, shape, lr):
    nb, n, p = shape[:3]
    S = sig(shape, lr)
    probs = problems(shape)
    batch = eng.dgpschur_batch(probs, S, lr)
    assert len(batch) == nb
    for q in range(nb):
        check_problem(shape, q, batch[q], lr)
    assert all(not a.flags.writeable for A in probs for a in A)  # (the copying form left its input alone)


def case_above_cap(eng, n):
    """an order above the cap (nb = 2, p = 2): the single call's reduction and iteration, problem by problem on the batch
    buffer"""
    shape = (2, n, 2, (T, F))
    case_full(eng, shape, "R")
    case_reduction(eng, shape)


# ------------------------------------------------------------------------------------------------
# 3. against the single call (simulation: built without contraction, the same bodies give the same bits)
def case_iteration_bits(eng, single_eng, shape):
    """dgpschur_hess_batch_ on the reduced problems against gpschur_hess_ with the signed trains off and the single-wave
    sweep, problem by problem: T, Z, alpha, beta, the scaling, and the sums of the counters."""
    nb, n, p = shape[:3]
    S = sig(shape, "R")
    probs = problems(shape)
    red, _ = eng.dgphessenberg_batch_([work(A) for A in probs], S)
    reduced = [work(H) for H, _ in red]
    assert single_eng.get_train_g() == 0
    singles = [single_eng.gpschur_hess_(work(H)[0], work(H)[1:], S) for H in reduced]
    Wb = [work(H) for H in reduced]
    batch = eng.dgpschur_hess_batch_([(W[0], W[1:]) for W in Wb], S)
    for q in range(nb):
        same_bits(singles[q], batch[q], p, (shape_id(shape), q))
        assert batch[q].S == list(S)
    st = batch[0].stats
    for name in ("nsweeps", "nrqpass", "ndefl2", "ndefl1", "nwindows", "reserved", "niter"):
        assert getattr(st, name) == sum(getattr(s.stats, name) for s in singles), (shape_id(shape), name)
    assert st.nsweeps > 0 or n <= 2
    if p >= 20:
        assert st.nrqpass > 0  # (the zero-shift pass came first)


def case_full_bits(eng, single_eng, shape, lr):
    """dgpschur_batch against pschur_(..., S=S) in the same form (trains off, serial stage 2, single-wave sweep)"""
    nb, n, p = shape[:3]
    S = sig(shape, lr)
    probs = problems(shape)
    batch = eng.dgpschur_batch(probs, S, lr)
    for q in range(nb):
        one = single_eng.pschur_(work(probs[q]), lr, S=S)
        same_bits(one, batch[q], p, (shape_id(shape), lr, q))


# ------------------------------------------------------------------------------------------------
# 4. place independence
def case_places(eng, shape):
    """Nothing is shared between the problems of a batch: one problem at several positions of one batch, and in batches
    of other sizes, gives the same bits."""
    nb, n, p = shape[:3]
    probs = problems(shape)
    A, B = probs[0], probs[nb - 1]
    for lr in ("R", "L"):
        S = sig(shape, lr)
        alone = eng.dgpschur_batch([A], S, lr)[0]
        mixed = eng.dgpschur_batch([A, B, A, B, B, A], S, lr)
        for q in (0, 2, 5):
            same_bits(alone, mixed[q], p, (shape_id(shape), lr, q))
        for q in (3, 4):
            same_bits(mixed[1], mixed[q], p, (shape_id(shape), lr, q))
        pair = eng.dgpschur_batch([B, A], S, lr)
        same_bits(alone, pair[1], p, (shape_id(shape), lr, "pair"))
        same_bits(mixed[1], pair[0], p, (shape_id(shape), lr, "pair"))


# ------------------------------------------------------------------------------------------------
# 5. all-true and NULL signatures, flags
def case_all_true(eng, shape=(5, 12, 3, (T, T, T))):
    """An all-true signature and none at all run the signed kernels: GeneralizedPeriodicSchur in the real form, the checks
    of case_full; both spellings give the same bits, through every entry."""
    nb, n, p = shape[:3]
    probs = problems(shape)
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for lr in ("R", "L"):
        a = eng.dgpschur_batch(probs, [True] * p, lr)
        b = eng.dgpschur_batch(probs, None, lr)
        for q in range(nb):
            check_problem(shape, q, a[q], lr)
            same_bits(a[q], b[q], p, (lr, q))
        # a NULL S at the C entry
        Wb = [work(A) for A in probs]
        flat = [w for W in Wb for w in W]
        Z = [np.zeros((n, n), order="F") for _ in range(nb * p)]
        al, be, sc = np.zeros((nb, n), dtype=np.complex128), np.zeros((nb, n)), np.zeros((nb, n), dtype=np.int32)
        si, info = C.c_int(0), C.c_int(0)
        rc = eng.lib.psd_d_gpschur_batch(eng.ctx, nb, n, p, eng._ptrs(flat), None, lr.encode(), 1, 1, 120, eng._ptrs(Z),
                                         al.view(np.float64).ctypes.data_as(dp), be.ctypes.data_as(dp),
                                         sc.ctypes.data_as(i32p), None, C.byref(si), None, C.byref(info))
        assert rc == 0 and info.value == 0 and si.value == (p if lr == "L" else 1)
        for q in range(nb):
            assert np.array_equal(al[q], a[q].alpha) and np.array_equal(be[q], a[q].beta)
            assert all(np.array_equal(Wb[q][j], a[q].Ts[j]) and np.array_equal(Z[q * p + j], a[q].Z[j]) for j in range(p))
    red, _ = eng.dgphessenberg_batch_([work(A) for A in probs], None)
    red2, _ = eng.dgphessenberg_batch_([work(A) for A in probs], [True] * p)
    Ha, Hb = [work(H) for H, _ in red], [work(H) for H, _ in red2]
    x = eng.dgpschur_hess_batch_([(H[0], H[1:]) for H in Ha], None)
    y = eng.dgpschur_hess_batch_([(H[0], H[1:]) for H in Hb], [True] * p)
    for q in range(nb):
        same_bits(x[q], y[q], p, ("hess", q))
        assert x[q].S == [True] * p


def case_flags(eng, shape=SHAPES[2]):
    """wantZ=False and wantT=False, wantZ=False against the full run: the eigenvalues within 1e-9 |lambda|max, the bound of
    engine_cases.case_rg_fast_paths"""
    nb, n, p = shape[:3]
    probs = problems(shape)
    for lr in ("R", "L"):
        S = sig(shape, lr)
        full = eng.dgpschur_batch(probs, S, lr)
        noz = eng.dgpschur_batch(probs, S, lr, wantZ=False)
        not_ = eng.dgpschur_batch(probs, S, lr, wantZ=False, wantT=False)
        for q in range(nb):
            sc = abs(full[q].values).max()
            assert noz[q].Z == [] and not_[q].Z == []
            e1, e2 = pt.match_eigs(full[q].values, noz[q].values), pt.match_eigs(full[q].values, not_[q].values)
            print(f"flags {lr} q={q}: {e1:.3e}, {e2:.3e} (bound {1e-9 * sc:.3e})")
            assert e1 < 1e-9 * sc and e2 < 1e-9 * sc
            for ps in (full[q], noz[q], not_[q]):
                assert ps.schurindex == (1 if lr == "R" else p) and ps.orientation == lr and ps.S == S
            js = full[q].schurindex - 1
            for j in range(p):  # (without Z the factors still are the T factors)
                assert np.all(np.tril(noz[q].Ts[j], -2 if j == js else -1) == 0)
        W = work(probs[0])
        b1 = eng.dgpschur_batch_([W], S, lr)
        assert b1[0].Ts[0] is W[0]  # in place


# ------------------------------------------------------------------------------------------------
# 6. holes (Cases II and III)
HOLES = [(tuple(S), l, j) for (S, l, j) in ec.RG_HOLES]


def hole_id(h):
    return "%s_f%d_i%d" % ("".join("T" if s else "F" for s in h[0]), h[1], h[2])


def case_holes(eng, hole):
    """An exact zero on the diagonal of a triangular factor — of a +1 factor (Case II) or of a -1 factor (Case III) — in
    Hessenberg-triangular inputs as engine_cases.rg_hess_ut makes them (n = p = 5, the RG_HOLES table), in a batch
    between two hole-free problems.  Finite eigenvalues match pt.oracle_gpschur_hess within 1e-9 max(1, |lambda|max)
    (engine_cases._rg_match_oracle) and as many are infinite; `reserved` is the sum of the oracle's Case II and III counts;
    the hole-free neighbours give the bits they give in a batch without the hole."""
    S, fac, idx = hole
    S = list(S)
    n = p = 5
    probs = [ec.rg_hess_ut(n, p, 1900), ec.rg_hess_ut(n, p, 900), ec.rg_hess_ut(n, p, 2900)]
    probs[1][fac - 1][idx - 1, idx - 1] = 0.0
    Wb = [work(A) for A in probs]
    out = eng.dgpschur_hess_batch_([(W[0], W[1:]) for W in Wb], S)
    c2 = c3 = 0
    for q in range(3):
        pt.rgpschur_check(probs[q], S, out[q])
        real_form(out[q], (hole_id(hole), q))
        po = pt.oracle_gpschur_hess(probs[q][0], probs[q][1:], S)
        assert po.info == 0
        fin, gfin = np.isfinite(po.values), np.isfinite(out[q].values)
        assert fin.sum() == gfin.sum(), (hole, q)
        err = pt.match_eigs(po.values[fin], out[q].values[gfin])
        bound = 1e-9 * max(1.0, abs(po.values[fin]).max())
        print(f"{hole_id(hole)} q={q}: finite {fin.sum()}/{n}, |lam - oracle| = {err:.3e} (bound {bound:.3e})")
        assert err < bound, (hole, q, err)
        if q == 1:
            assert po.counters["case2"] + po.counters["case3"] >= 1, hole
        c2 += po.counters["case2"]
        c3 += po.counters["case3"]
    st = out[0].stats
    assert (st.reserved % 1000, st.reserved // 1000) == (c2, c3), (hole, st.reserved, c2, c3)
    Wc = [work(probs[0]), work(probs[2])]
    clean = eng.dgpschur_hess_batch_([(W[0], W[1:]) for W in Wc], S)
    same_bits(clean[0], out[0], p, (hole_id(hole), "left neighbour"))
    same_bits(clean[1], out[2], p, (hole_id(hole), "right neighbour"))


# ------------------------------------------------------------------------------------------------
# 7. one failing problem
ONE_FAILS_SHAPE = (4, 24, 3, (T, F, T))
ONE_FAILS_MAXITFAC = 2


def one_fails_problems(n=24, p=3):
    """Three problems whose product needs a handful of sweeps — triangular factors with one 3 x 3 block in A_1 — around
    one full random problem (zgbatch_cases.one_fails_problems in Float64)."""
    def easy(seed):
        A = [np.triu(a) for a in pt.bench_factors(n, p, seed=seed)]
        full = pt.bench_factors(n, 1, seed=seed + 977)[0]
        for k in (9, 10):
            A[0][k + 1, k] = full[k + 1, k]
        return [np.asfortranarray(a) for a in A]
    return [easy(41), pt.bench_factors(n, p, seed=42), easy(43), easy(44)]


def case_one_fails(eng):
    """maxitfac = 2, S = (T, F, T): the full problem cannot deflate 24 eigenvalues within its budget of 48 iterations and
    ends alone; the three nearly triangular ones are complete and correct.  The reference does the same on these inputs:
    the oracle's codes with this maxitfac are non-zero for the second problem alone (asserted here)."""
    S = list(ONE_FAILS_SHAPE[3])
    probs = one_fails_problems()
    codes = [pt.oracle_gpschur(work(A), S, "R", maxitfac=ONE_FAILS_MAXITFAC).info for A in probs]
    assert codes[1] != 0 and codes[0] == codes[2] == codes[3] == 0, codes
    infos = []
    out = eng.dgpschur_batch(probs, S, "R", maxitfac=ONE_FAILS_MAXITFAC, infos_out=infos)
    assert len(infos) == 4 and infos[0] == 0 and infos[2] == 0 and infos[3] == 0, infos
    assert psd_amd.INFO_NOCONV < infos[1] <= psd_amd.INFO_NOCONV + 24, infos  # PSD_INFO_NOCONV + level
    for q in (0, 2, 3):
        check_problem(ONE_FAILS_SHAPE, q, out[q], "R", A=probs[q], S=S, ref=False)
        po = pt.oracle_gpschur(work(probs[q]), S, "R")
        assert po.info == 0
        assert pt.match_eigs(po.values, out[q].values) < 1e-8 * max(1.0, abs(po.values).max())
    Ws = [work(A) for A in probs]
    with pytest.raises(psd_amd.ConvergenceError):  # raised after all four have run
        eng.dgpschur_batch_(Ws, S, "R", maxitfac=ONE_FAILS_MAXITFAC)
    for q in (0, 2, 3):  # ... so the in-place factors of the others are their T factors
        assert all(np.array_equal(Ws[q][j], out[q].Ts[j]) for j in range(3))


# ------------------------------------------------------------------------------------------------
# 8. gpschur_batch(real=True)
def _pairs(nb, n, ph, seed):
    As = [pt.bench_factors(n, ph, seed=seed + 17 * q) for q in range(nb)]
    Bs = [pt.bench_factors(n, ph, seed=seed + 17 * q + 5000) for q in range(nb)]
    return As, Bs


def case_gpschur_batch_real(eng):
    """real=True against the loop of Engine.gpschur per pair: real output, eigenvalues within 1e-8 max(1, |lambda|max) (the
    bound of engine_cases.case_rg_full_sizes: the single call runs trains and the pipelined stage 2, so it rounds
    differently); the factors decompose gpschur's interleaving.  The default stays the ComplexF64 path."""
    n = 6
    for nb, ph, seed in ((4, 1, 300), (3, 3, 400)):
        As, Bs = _pairs(nb, n, ph, seed)
        out = eng.gpschur_batch(As, Bs, real=True)
        assert len(out) == nb
        for q in range(nb):
            one = eng.gpschur(As[q], Bs[q])
            err = pt.match_eigs(one.values, out[q].values)
            print(f"{ph} pairs q={q}: |lam - gpschur| = {err:.3e}")
            assert err < 1e-8 * max(1.0, abs(one.values).max()), (q, err)
            assert out[q].S == one.S == [True, False] * ph and out[q].period == 2 * ph
            real_form(out[q], (ph, q))
            if ph == 1:
                Cs = [As[q][0], Bs[q][0]]
            else:
                Cs = [As[q][2], Bs[q][1], As[q][1], Bs[q][0], As[q][0], Bs[q][2]]
            pt.rgpschur_check(Cs, out[q].S, out[q])
    dflt = eng.gpschur_batch(As, Bs)
    assert all(t.dtype == np.complex128 for t in dflt[0].Ts)  # (the default is untouched)
    assert eng.gpschur_batch([], [], real=True) == []
    with pytest.raises(TypeError):
        eng.gpschur_batch([[a.astype(np.complex128) for a in As[0]]], [Bs[0]], real=True)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.gpschur_batch(As, Bs[:2], real=True)


# ------------------------------------------------------------------------------------------------
# 9. argument errors and ABI codes
def case_argument_errors(eng):
    A = problems(SHAPES[2])   # n = 12, p = 3
    B = problems(SHAPES[1])   # n = 2, p = 2
    S3, S2 = [T, F, T], [T, F]
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgpschur_batch([A[0], B[0] + B[0][:1]], S3)  # unequal order
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgpschur_batch([B[0], B[1][:1]], S2)  # unequal period
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgpschur_batch(A, S2)  # one entry of S per factor
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgphessenberg_batch_([work(a) for a in A], S2)
    with pytest.raises(psd_amd.DimensionMismatch):
        W = [work(a) for a in A]
        eng.dgpschur_hess_batch_([(w[0], w[1:]) for w in W], S2)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgpschur_batch([[a[:, :5] for a in A[0]]], S3)  # not square
    with pytest.raises(ValueError):
        eng.dgpschur_batch(A, [F, T, T], "R")  # the leftmost entry must be true
    with pytest.raises(ValueError):
        eng.dgpschur_batch(A, [T, T, F], "L")
    with pytest.raises(ValueError):
        eng.dgphessenberg_batch_([work(a) for a in A], [F, T, T])
    with pytest.raises(ValueError):
        W = [work(a) for a in A]
        eng.dgpschur_hess_batch_([(w[0], w[1:]) for w in W], [F, T, T])
    with pytest.raises(TypeError):
        eng.dgpschur_batch_([[np.ascontiguousarray(a) for a in A[0]]], S3)  # in place needs Fortran order
    with pytest.raises(ValueError):
        eng.dgpschur_batch(A, S3, "X")
    cplx = [[np.asfortranarray(a.astype(np.complex128)) for a in A[0]]]
    with pytest.raises(TypeError, match="Float64 only"):  # the wrong family
        eng.dgpschur_batch(cplx, S3)
    with pytest.raises(TypeError, match="Float64 only"):
        eng.dgpschur_batch_(cplx, S3)
    with pytest.raises(TypeError, match="Float64 only"):
        eng.dgphessenberg_batch_(cplx, S3)
    with pytest.raises(TypeError, match="Float64 only"):
        eng.dgpschur_hess_batch_([(cplx[0][0], cplx[0][1:])], S3)
    assert eng.dgpschur_batch([], S3) == [] and eng.dgpschur_batch_([], S3, "L") == []
    assert eng.dgpschur_hess_batch_([], S3) == [] and eng.dgphessenberg_batch_([], S3)[0] == []
    infos = [7]
    assert eng.dgpschur_batch([], S3, infos_out=infos) == [] and infos == []


def case_abi_codes(eng, shape=SHAPES[2], devbuf=None):
    """The argument codes of the four C entries, and (simulation, where device memory is host memory: `devbuf` None)
    psd_d_gpschur_batch_dev on packed blocks against the host entry, bit for bit.  `devbuf`: the address of one packed
    problem in device memory for the calls of the device entry that go through."""
    nb, n, p = shape[:3]
    probs = problems(shape)
    dp = C.POINTER(C.c_double)
    i32p = C.POINTER(C.c_int32)
    lib, ctx = eng.lib, eng.ctx

    def sarr(S):
        return (C.c_uint8 * len(S))(*[1 if x else 0 for x in S])

    for lr in ("R", "L") if devbuf is None else ():
        S = sig(shape, lr)
        host = eng.dgpschur_batch(probs, S, lr)
        dA = np.ascontiguousarray(np.array([pt.pack(A, np.float64) for A in probs]))
        dZ = np.zeros_like(dA)
        alpha, beta = np.zeros((nb, n), dtype=np.complex128), np.zeros((nb, n))
        sc = np.zeros((nb, n), dtype=np.int32)
        infos = (C.c_int * nb)()
        si, info = C.c_int(0), C.c_int(0)
        st = psd_amd.Stats()
        rc = lib.psd_d_gpschur_batch_dev(ctx, nb, n, p, C.c_void_p(dA.ctypes.data), sarr(S), lr.encode(), 1, 1, 120,
                                         C.c_void_p(dZ.ctypes.data), alpha.view(np.float64).ctypes.data_as(dp),
                                         beta.ctypes.data_as(dp), sc.ctypes.data_as(i32p), infos, C.byref(si),
                                         C.byref(st), C.byref(info))
        assert rc == 0 and info.value == 0 and si.value == (p if lr == "L" else 1) and not any(infos)
        assert st.ms_total >= st.ms_hess >= 0 and st.nsweeps > 0
        for q in range(nb):
            assert np.array_equal(alpha[q], host[q].alpha) and np.array_equal(beta[q], host[q].beta)
            assert np.array_equal(sc[q], host[q].alphascale)
            for j in range(p):
                assert np.array_equal(dA[q, j].T, host[q].Ts[j]) and np.array_equal(dZ[q, j].T, host[q].Z[j])
    A = work(probs[0])
    ptrs = eng._ptrs(A)
    al, be, sc1 = np.zeros(n, dtype=np.complex128), np.zeros(n), np.zeros(n, dtype=np.int32)
    ap, bp, sp = al.view(np.float64).ctypes.data_as(dp), be.ctypes.data_as(dp), sc1.ctypes.data_as(i32p)
    buf = C.c_void_p(dA.ctypes.data if devbuf is None else devbuf)
    SR, SL = sarr([T, F, T]), sarr([F, T, T])  # SL: leftmost in working order true for 'L' only

    def hess(nb_=1, n_=n, p_=p, A_=ptrs, S_=SR):
        return lib.psd_d_gphessenberg_batch(ctx, nb_, n_, p_, A_, S_, None, None, None)

    def host_(nb_=1, n_=n, p_=p, A_=ptrs, S_=SR, o=b"R", mi=120, wz=0, Z_=None, al_=ap, be_=bp, sc_=sp):
        return lib.psd_d_gpschur_batch(ctx, nb_, n_, p_, A_, S_, o, 1, wz, mi, Z_, al_, be_, sc_, None, None, None, None)

    def dev_(nb_=1, n_=n, p_=p, A_=buf, S_=SR, o=b"R", mi=120, wz=0, Z_=None, al_=ap, be_=bp, sc_=sp):
        return lib.psd_d_gpschur_batch_dev(ctx, nb_, n_, p_, A_, S_, o, 1, wz, mi, Z_, al_, be_, sc_, None, None, None, None)

    def hb_(nb_=1, n_=n, p_=p, H_=ptrs, S_=SR, mi=120, wz=0, Q_=None, al_=ap, be_=bp, sc_=sp):
        return lib.psd_d_gpschur_hess_batch(ctx, nb_, n_, p_, H_, S_, Q_, 1, wz, mi, al_, be_, sc_, None, None, None)

    assert hess(nb_=0) == -2 and hess(n_=0) == -3 and hess(p_=0) == -4 and hess(A_=None) == -5 and hess(S_=SL) == -7
    assert hess() == 0 and hess(S_=None) == 0
    for f in (host_, dev_):
        assert f(nb_=0) == -2 and f(n_=0) == -3 and f(p_=0) == -4 and f(A_=None) == -5 and f(o=b"X") == -6
        assert f(S_=SL) == -7 and f(S_=SR, o=b"L") == 0 and f(S_=sarr([T, T, F]), o=b"L") == -7
        assert f(mi=0) == -9 and f(wz=1) == -10 and f(al_=None) == -11 and f(be_=None) == -11 and f(sc_=None) == -11
        assert f() == 0 and f(S_=None) == 0
    assert hb_(nb_=0) == -2 and hb_(n_=0) == -3 and hb_(p_=0) == -4 and hb_(H_=None) == -5 and hb_(wz=1) == -6
    assert hb_(S_=SL) == -7 and hb_(mi=0) == -9 and hb_(al_=None) == -11 and hb_(be_=None) == -11 and hb_(sc_=None) == -11
    assert lib.psd_d_gphessenberg_batch(None, 1, n, p, ptrs, SR, None, None, None) == -1
    assert lib.psd_d_gpschur_batch(None, 1, n, p, ptrs, SR, b"R", 1, 0, 120, None, ap, bp, sp, None, None, None, None) == -1
    assert lib.psd_d_gpschur_batch_dev(None, 1, n, p, buf, SR, b"R", 1, 0, 120, None, ap, bp, sp, None, None, None, None) == -1
    assert lib.psd_d_gpschur_hess_batch(None, 1, n, p, ptrs, SR, None, 1, 0, 120, ap, bp, sp, None, None, None) == -1


def case_abi_codes_gpu(eng, shape=SHAPES[2]):
    """case_abi_codes with the device entry's problem in device memory"""
    import torch

    dA = torch.from_numpy(np.ascontiguousarray(pt.pack(problems(shape)[0], np.float64))).cuda()
    torch.cuda.synchronize()
    case_abi_codes(eng, shape, devbuf=dA.data_ptr())


# ------------------------------------------------------------------------------------------------
# 10. groups
def case_groups(make_engine, shape=SHAPES[8]):
    """A host entry whose batch does not fit the device at once works through it in groups (PSD_BATCH_GROUP lowers the
    group size): the same bits as in one group, problem by problem."""
    nb, n, p = shape[:3]
    probs = problems(shape)
    ref = make_engine({})
    eng = make_engine({"PSD_BATCH_GROUP": "4"})
    S = sig(shape, "L")
    whole = ref.dgpschur_batch(probs, S, "L")
    parts = eng.dgpschur_batch(probs, S, "L")
    for q in range(nb):
        same_bits(whole[q], parts[q], p, q)
    for name in ("nsweeps", "nwindows", "ndefl1", "ndefl2", "niter"):
        assert getattr(whole[0].stats, name) == getattr(parts[0].stats, name), name
    S = sig(shape, "R")
    ob, _ = ref.dgphessenberg_batch_([work(A) for A in probs], S)
    op, _ = eng.dgphessenberg_batch_([work(A) for A in probs], S)
    for q in range(nb):
        assert all(np.array_equal(ob[q][0][j], op[q][0][j]) and np.array_equal(ob[q][1][j], op[q][1][j]) for j in range(p))
    Hb, Hp = [work(o[0]) for o in ob], [work(o[0]) for o in op]
    hb = ref.dgpschur_hess_batch_([(H[0], H[1:]) for H in Hb], S)
    hp = eng.dgpschur_hess_batch_([(H[0], H[1:]) for H in Hp], S)
    for q in range(nb):
        same_bits(hb[q], hp[q], p, ("hess", q))


# ------------------------------------------------------------------------------------------------
# the device-resident entry (GPU)
def case_device_resident(eng, shape=SHAPES[2]):
    """One torch float64 [nb, p, n, n] tensor through psd_d_gpschur_batch_dev: T, Z and the values equal the host entry's
    bit for bit (the same kernels on the same data; the entries differ in the copies alone)."""
    import torch

    nb, n, p = shape[:3]
    probs = problems(shape)
    for lr in ("R", "L"):
        S = sig(shape, lr)
        host = eng.dgpschur_batch(probs, S, lr)
        dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in probs])).cuda()
        assert dA.dtype == torch.float64
        keep = dA.clone()
        Tt, Zt, values, st = eng.dgpschur_batch(dA, S, lr)
        assert isinstance(Tt, torch.Tensor) and Tt.is_cuda and Zt.is_cuda and tuple(Tt.shape) == (nb, p, n, n)
        assert Tt.dtype == Zt.dtype == torch.float64
        assert torch.equal(dA, keep)  # the input stays as it was
        Th, Zh = Tt.cpu().numpy(), Zt.cpu().numpy()
        for q in range(nb):
            assert np.array_equal(values[q], host[q].values), (lr, q)
            for j in range(p):
                assert np.array_equal(Th[q, j], host[q].Ts[j]), (lr, q, j)
                assert np.array_equal(Zh[q, j], host[q].Z[j]), (lr, q, j)
    Tn, Zn, vn, _ = eng.dgpschur_batch_(dA, sig(shape, "R"), "R", wantZ=False)
    assert Zn is None
    for q in range(nb):
        po = reference(shape, q, "R")
        assert pt.match_eigs(po.values, vn[q]) < 1e-8 * max(1.0, abs(po.values).max())
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgpschur_batch(dA[:, :, :, :5], sig(shape, "R"))
    with pytest.raises(TypeError, match="Float64 only"):
        eng.dgpschur_batch(dA.to(torch.complex128), sig(shape, "R"))
    empty = torch.zeros((0, 2, 3, 3), dtype=torch.float64, device="cuda")
    infos = [7]
    Te, Ze, ve, ste = eng.dgpschur_batch_(empty, [True, False], infos_out=infos)
    assert tuple(Te.shape) == (0, 2, 3, 3) and ve.shape == (0, 3) and infos == [] and ste.niter == 0
