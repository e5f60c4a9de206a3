"""Engine.zgordschur_batch_ / zgordschur_batch (psd_z_gordschur_batch / psd_z_gordschur_batch_dev, csrc/psd_zgbord.h): many
small signed ComplexF64 periodic Schur forms reordered in one call — the cases shared by the simulated tier
(test_hostsim_zgordschur_batch.py) and the device tier (test_gpu_zgordschur_batch.py), the signed counterparts of
zord_batch_cases.  Inputs are zgpschur_batch results of pt.bench_factors(..., dtype=complex128) with one signature per
shape (reversed for 'L') and the eigenvalues at or below the median modulus selected; the checks and bounds of
engine_cases.case_gordschur_windows are applied to every problem of a batch.  pt.oracle_gordschur accepts every swap of
the first six problems of every shape (asserted)."""
import ctypes as C

import numpy as np
import pytest

import psd_amd
import psdtest as pt
from batch_common import SIG22, shape_id, sig
from zord_batch_cases import bits_differ, median_select, select_for

T, F = True, False

# (nb, n, p, S for 'R') and what each covers; for 'L' the signature is reversed (true entry last)
WINDOW_SHAPES = [
    (3, 48, 3, (T, F, T)),       # W = 32 < n: several windows, all three off-window roles
    (2, 40, 22, SIG22),          # W = 20
    (2, 30, 70, tuple(q % 2 == 0 for q in range(70))),  # W = 10, window image near the LDS limit
    (33, 12, 3, (T, F, T)),      # more problems than a 32-wide chunk, n < W
    (3, 5, 2, (T, F)),           # a pencil
    (4, 2, 2, (T, F)),           # smallest window; row 2 alone is selected
    (3, 1, 3, (T, F, T)),        # n = 1: no swap
    (3, 33, 4, (T, T, F, T)),    # signature class: a positive factor beside a negative one
    (3, 20, 4, (T, F, F, T)),    # signature class: adjacent negative factors
]
NARROW_SHAPE = (3, 20, 3, (T, F, T))  # with PSD_BORD_W=6: several narrow windows
GROUP_SHAPE = (6, 20, 3, (T, T, F))   # the group loop under PSD_BATCH_GROUP=4
CAP_SHAPE = (2, 20, 3, (T, F, T))
CHAIN_SHAPE = (5, 12, 3, (T, F, T))
NORACLE = 6  # the oracle runs on the first six problems of a shape

_cache = {}


def expected_window(n, p):
    """zgordschur_dev's candidates under zgord_lds_bytes (csrc/psd_engine.cpp), narrowed to the smallest that holds the
    whole problem."""
    W = 0
    for w in (32, 24, 20, 16, 12, 10, 8, 6, 4):
        b = p * w * (w + 1) * 16 + 15 * p * 16 + (p + 2) * 8 + p * 4 + 64
        if (b + 15) // 16 * 16 > 155 * 1024:
            continue
        if W == 0 or w >= n:
            W = w
    return W


def gclone(ps):
    return psd_amd.GeneralizedPeriodicSchur(list(ps.S), [t.copy(order="F") for t in ps.Ts], [z.copy(order="F") for z in ps.Z],
                                            ps.alpha.copy(), ps.beta.copy(), ps.alphascale.copy(), ps.orientation,
                                            ps.schurindex)


def factors(shape):
    """The factors of a shape: built once, shared, never written to."""
    nb, n, p = shape[:3]
    key = ("A", nb, n, p)
    if key not in _cache:
        probs = [pt.bench_factors(n, p, seed=9700 + 131 * q + 7 * n + p, dtype=np.complex128) for q in range(nb)]
        for A in probs:
            for a in A:
                a.setflags(write=False)
        _cache[key] = probs
    return _cache[key]


def inputs(eng, shape, lr):
    """(factors, decompositions, selections) of a shape and orientation: computed once per library (the engines of a tier
    differ in the knobs of the reordering only) and only cloned."""
    key = (eng.lib._name, shape, lr)
    if key not in _cache:
        probs = factors(shape)
        ps0 = eng.zgpschur_batch(probs, sig(shape, lr), lr)
        sels = np.array([select_for(shape, ps.values) for ps in ps0])
        _cache[key] = (probs, ps0, sels)
    return _cache[key]


def single(eng, shape, lr, q):
    """ordschur_ of problem q on `eng` (the serial or the default single driver): computed once, never written to."""
    key = ("single", id(eng), shape, lr, q)
    if key not in _cache:
        probs, ps0, sels = inputs(eng, shape, lr)
        _cache[key] = (eng.ordschur_(gclone(ps0[q]), sels[q]), eng)
    return _cache[key][0]


def oracle(ps0, select):
    po0 = pt.GPSD(ps0.S, [t.copy() for t in ps0.Ts], [z.copy() for z in ps0.Z], ps0.alpha, ps0.beta, ps0.alphascale,
                  ps0.orientation, ps0.schurindex)
    return pt.oracle_gordschur(po0, select)


def check_problem(A, ps0, ps1, select, oracle_run=True, nswaps=None):
    """The checks of engine_cases.case_gordschur_windows with its bounds, for one problem; returns the swap count."""
    n = A[0].shape[0]
    lam0 = ps0.values
    assert ps1.S == ps0.S
    pt.gpschur_check(A, ps0.S, ps1, tol=100 * max(1.0, np.sqrt(n / 32)), qtol=10 * max(1.0, np.sqrt(n / 32)))
    for t in ps1.Ts:
        assert np.all(np.tril(t, -1) == 0)  # (every factor stays triangular)
    assert np.array_equal(ps1.values, pt.gvalues(ps1.alpha, ps1.beta, ps1.alphascale))
    m = int(select.sum())
    sc = abs(lam0).max()
    assert pt.match_eigs(lam0[select], ps1.values[:m]) < 1e-9 * sc
    assert pt.match_eigs(lam0[~select], ps1.values[m:]) < 1e-9 * sc
    # the order inside the selected / unselected groups is preserved (stable bubbling)
    assert np.allclose(ps1.values[:m], lam0[select], rtol=1e-7, atol=1e-9 * sc)
    assert np.allclose(ps1.values[m:], lam0[~select], rtol=1e-7, atol=1e-9 * sc)
    if oracle_run:
        po = oracle(ps0, select)
        assert po.info == 0 and ps1.stats.nsweeps == po.nswaps, (ps1.stats.nsweeps, po.nswaps)
    if nswaps is not None:
        assert ps1.stats.nsweeps == nswaps
    return ps1.stats.nsweeps


# ------------------------------------------------------------------------------------------------
# 1. reference shape
def case_reference(eng, lr):
    """engine_cases.case_gordschur_reference per problem of a batch: (nb, n, p) = (4, 7, 5), spectrum 4^j."""
    nb, n, p, nsel = 4, 7, 5, 2
    S = [True] * p
    for l in range(0, p - 1, 2):
        S[l] = False
    probs = [pt.gord_test_factors(n, p, S, seed=31 + 37 * q, cplx=True) for q in range(nb)]
    if lr == "R":
        probs, S = [A[::-1] for A in probs], S[::-1]
    ps0 = eng.zgpschur_batch(probs, S, lr)
    for q in range(nb):
        pt.gpschur_check(probs[q], S, ps0[q])
    for which in ("smallest", "largest"):
        sels, idxs = [], []
        for ps in ps0:
            idx = np.argsort(np.abs(ps.values))
            if which == "largest":
                idx = idx[::-1]
            s = np.zeros(n, dtype=bool)
            s[idx[:nsel]] = True
            sels.append(s)
            idxs.append(idx)
        out = eng.zgordschur_batch_([gclone(ps) for ps in ps0], np.array(sels))
        assert eng.zgordschur_batch_stats.nlaunch_step == 1
        for q in range(nb):
            pt.gpschur_check(probs[q], S, out[q])
            for j in range(nsel):
                assert np.any(np.isclose(out[q].values[:nsel], ps0[q].values[idxs[q][j]], rtol=1e-8))
            po = oracle(ps0[q], sels[q])
            assert po.info == 0 and out[q].stats.nsweeps == po.nswaps
            assert pt.match_eigs(po.values, out[q].values) < 1e-9 * abs(po.values).max()


# ------------------------------------------------------------------------------------------------
# 2. windows
def case_windows(eng, shape, lr, expect_window=None):
    nb, n, p = shape[:3]
    probs, ps0, sels = inputs(eng, shape, lr)
    out = eng.zgordschur_batch_([gclone(ps) for ps in ps0], sels)
    st = eng.zgordschur_batch_stats
    assert len(out) == nb and st.nlaunch_step == 1 and st.nsweeps == sum(ps.stats.nsweeps for ps in out)
    assert list(eng.zgordschur_batch_nswaps) == [ps.stats.nsweeps for ps in out]
    if expect_window is not None:
        assert st.window == expect_window and st.nwindows > nb  # (several windows per problem)
    else:
        assert st.window == expected_window(n, p), (st.window, expected_window(n, p))
    noz = eng.zgordschur_batch_([gclone(ps) for ps in ps0], sels, wantZ=False)
    for q in range(nb):
        one = single(eng, shape, lr, q)
        nsw = check_problem(probs[q], ps0[q], out[q], sels[q], oracle_run=q < NORACLE, nswaps=one.stats.nsweeps)
        assert (nsw > 0) == (n > 1)
        sc = abs(ps0[q].values).max()
        # wantZ = false leaves Z untouched and gives the same T
        assert all(np.array_equal(a, b) for a, b in zip(noz[q].Z, ps0[q].Z))
        assert max(np.abs(a - b).max() for a, b in zip(noz[q].Ts, out[q].Ts)) < 1e-12 * sc


# ------------------------------------------------------------------------------------------------
# 3. against the serial single driver
def _same(a, b):
    return (np.array_equal(a.values, b.values) and np.array_equal(a.alpha, b.alpha) and np.array_equal(a.beta, b.beta)
            and np.array_equal(a.alphascale, b.alphascale) and all(np.array_equal(x, y) for x, y in zip(a.Ts, b.Ts))
            and all(np.array_equal(x, y) for x, y in zip(a.Z, b.Z)))


def case_against_serial(make_engine, shape, lr, exact):
    """The single driver with PSD_ORD_PIPE=0 (psd_z_gordschur) moves one eigenvalue at a time through the same windows
    with the same arithmetic as the batched kernel; the roles of a window touch disjoint entries, so the order of the
    items cannot matter.  exact: bit for bit (the simulation is built with -ffp-contract=off); otherwise 1e-12 * scale
    (contraction may differ between kernels: the bound of the all-true sister kernel, which runs the same kind of
    bodies).  Returns the number of entries whose bits differ."""
    nb, n, p = shape[:3]
    ser = make_engine({"PSD_ORD_PIPE": "0"})
    probs, ps0, sels = inputs(ser, shape, lr)
    out = ser.zgordschur_batch_([gclone(ps) for ps in ps0], sels)
    differ = 0
    for q in range(nb):
        one = single(ser, shape, lr, q)
        assert one.stats.nsweeps == out[q].stats.nsweeps
        differ += bits_differ(one, out[q])
        sc = abs(ps0[q].values).max()
        print("against serial %s %s q=%d: entries with other bits %d, max |dT| %.3e, max |dZ| %.3e, max |dlam| %.3e (scale %.3e)"
              % (shape_id(shape), lr, q, bits_differ(one, out[q]),
                 max(np.abs(a - b).max() for a, b in zip(one.Ts, out[q].Ts)),
                 max(np.abs(a - b).max() for a, b in zip(one.Z, out[q].Z)), np.abs(one.values - out[q].values).max(), sc))
        if exact:
            assert _same(one, out[q]), (shape_id(shape), lr, q)
        else:
            assert max(np.abs(a - b).max() for a, b in zip(one.Ts, out[q].Ts)) <= 1e-12 * sc
            assert max(np.abs(a - b).max() for a, b in zip(one.Z, out[q].Z)) <= 1e-12 * sc
            assert np.abs(one.values - out[q].values).max() <= 1e-12 * sc
    return differ


# ------------------------------------------------------------------------------------------------
# 4. independence
def case_independence(eng, shape, lr="R"):
    """A problem alone in a batch of one gets, bit for bit, what it gets inside the batch."""
    nb, n, p = shape[:3]
    probs, ps0, sels = inputs(eng, shape, lr)
    out = eng.zgordschur_batch_([gclone(ps) for ps in ps0], sels)
    for q in sorted({0, nb - 2, nb - 1} & set(range(nb))):
        alone = eng.zgordschur_batch_([gclone(ps0[q])], sels[q:q + 1])
        assert _same(alone[0], out[q]), (shape_id(shape), q)


def case_groups(make_engine, shape=GROUP_SHAPE):
    """PSD_BATCH_GROUP=4: a batch worked through in two groups equals one group bit for bit."""
    nb, n, p = shape[:3]
    ref = make_engine({})
    eng = make_engine({"PSD_BATCH_GROUP": "4"})
    probs, ps0, sels = inputs(ref, shape, "L")
    whole = ref.zgordschur_batch_([gclone(ps) for ps in ps0], sels)
    assert ref.zgordschur_batch_stats.nlaunch_step == 1
    parts = eng.zgordschur_batch_([gclone(ps) for ps in ps0], sels)
    assert eng.zgordschur_batch_stats.nlaunch_step == 2
    for q in range(nb):
        assert _same(whole[q], parts[q]), q
        assert whole[q].stats.nsweeps == parts[q].stats.nsweeps > 0


# ------------------------------------------------------------------------------------------------
# 5. all-true signature
def case_all_true(eng, shape=CHAIN_SHAPE):
    """A null or all-true S is the call of zordschur_batch_: the same bits, through the C entry and the Python method."""
    nb, n, p = shape[:3]
    probs = factors(shape)
    for lr in "RL":
        ps0 = eng.zpschur_batch(probs, lr)
        sels = np.array([median_select(ps.values) for ps in ps0])

        def plain():
            return [psd_amd.PeriodicSchur([t.copy(order="F") for t in ps.Ts], [z.copy(order="F") for z in ps.Z],
                                          ps.values.copy(), lr, ps.schurindex) for ps in ps0]
        ref = eng.zordschur_batch_(plain(), sels)
        rst = eng.zordschur_batch_stats
        assert rst.nsweeps > 0
        gen = [psd_amd.GeneralizedPeriodicSchur([True] * p, ps.Ts, ps.Z, ps.values.copy(), np.ones(n),
                                                np.zeros(n, dtype=np.int32), lr, ps.schurindex) for ps in plain()]
        out = eng.zgordschur_batch_(gen, sels)
        st = eng.zgordschur_batch_stats
        assert st.nsweeps == rst.nsweeps and st.window == rst.window and st.nlaunch_step == rst.nlaunch_step
        for q in range(nb):
            assert bits_differ(ref[q], out[q]) == 0 and out[q].stats.nsweeps == ref[q].stats.nsweeps
            assert np.array_equal(out[q].values, pt.gvalues(out[q].alpha, out[q].beta, out[q].alphascale))
        for Sarr in (None, (C.c_uint8 * p)(*[1] * p)):
            work = plain()
            flatT, flatZ = [t for ps in work for t in ps.Ts], [z for ps in work for z in ps.Z]
            alpha, beta = np.zeros((nb, n), dtype=np.complex128), np.zeros((nb, n))
            sc = np.zeros((nb, n), dtype=np.int32)
            nsw = (C.c_int * nb)()
            rc = raw(eng, eng.lib.psd_z_gordschur_batch, nb, n, p, eng._ptrs(flatT), eng._ptrs(flatZ), Sarr, lr.encode(),
                     ps0[0].schurindex, np.ascontiguousarray(sels, dtype=np.uint8), 1, alpha, beta, sc, None, nsw)
            assert rc == 0
            for q in range(nb):
                assert nsw[q] == ref[q].stats.nsweeps
                assert np.array_equal(pt.gvalues(alpha[q], beta[q], sc[q]), ref[q].values)
                assert all(np.array_equal(a, b) for a, b in zip(work[q].Ts + work[q].Z, ref[q].Ts + ref[q].Z))


# ------------------------------------------------------------------------------------------------
# 6. per-problem selections
def case_selections(eng):
    """all-false, all-true and the median rule side by side in one batch; one row for every problem"""
    shape = (1, 8, 3, (T, F, T))
    n = shape[1]
    probs, ps0, _ = inputs(eng, shape, "R")
    A, ps0 = probs[0], ps0[0]
    sels = np.zeros((3, n), dtype=bool)
    sels[1] = True
    sels[2] = median_select(ps0.values)
    out = eng.zgordschur_batch_([gclone(ps0) for _ in range(3)], sels)
    assert out[0].stats.nsweeps == 0 and out[1].stats.nsweeps == 0
    for o in out[:2]:
        assert all(np.array_equal(a, b) for a, b in zip(o.Ts + o.Z, ps0.Ts + ps0.Z))  # untouched bit for bit
        assert np.allclose(o.values, ps0.values, rtol=1e-13, atol=0)  # (recomputed from the same diagonals)
    assert check_problem(A, ps0, out[2], sels[2]) > 0
    one = eng.zgordschur_batch_([gclone(ps0) for _ in range(3)], sels[2])  # one row for every problem
    assert all(_same(o, out[2]) for o in one)


# ------------------------------------------------------------------------------------------------
# 7. one problem fails
def singular_problem(seed=0):
    """n = 4, p = 2, S = (T, F), 'R': random complex upper-triangular factors plus 3 I with rows 1 and 2 of the diagonal
    of the Schur factor exactly zero, which makes an exactly zero row of the generalized periodic Sylvester system of
    the swap (1, 2).  (Equal eigenvalues would not do: under a signed S the cyclic system of such a pair is singular but
    can be consistent, and the swap is then accepted or rejected depending on rounding.)"""
    n, p = 4, 2
    rng = np.random.default_rng(seed)
    Ts = [np.asfortranarray(np.triu(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) + 3 * np.eye(n))
          for _ in range(p)]
    Ts[0][0, 0] = Ts[0][1, 1] = 0
    Z = [np.asfortranarray(np.eye(n, dtype=np.complex128)) for _ in range(p)]
    alpha = np.diag(Ts[0]) / np.diag(Ts[1])
    return psd_amd.GeneralizedPeriodicSchur([True, False], Ts, Z, alpha, np.ones(n), np.zeros(n, dtype=np.int32), "R", 1)


def one_fails_inputs(eng):
    shape = (3, 4, 2, (T, F))
    good, ps0, gsel = inputs(eng, shape, "R")
    bad = singular_problem()
    probs = [good[0], [t.copy() for t in bad.Ts], good[1], good[2]]
    work = [ps0[0], bad, ps0[1], ps0[2]]
    sels = np.array([gsel[0], [False, True, False, False], gsel[1], gsel[2]])
    return probs, work, sels


def case_one_fails(eng):
    probs, work, sels = one_fails_inputs(eng)
    with pytest.raises((psd_amd.SingularException, psd_amd.IllConditionedException)):
        eng.ordschur_(gclone(work[1]), sels[1])  # (the single call on the same engine rejects it: the yardstick)
    infos = []
    out = eng.zgordschur_batch_([gclone(ps) for ps in work], sels, infos_out=infos)
    assert len(infos) == 4 and infos[0] == 0 and infos[2] == 0 and infos[3] == 0, infos
    assert infos[1] == 3000 or 2000 <= infos[1] < 3000, infos
    for q in (0, 2, 3):
        check_problem(probs[q], work[q], out[q], sels[q])
    # the failed problem is still a decomposition of its product, with its old values
    pt.gpschur_check(probs[1], work[1].S, out[1])
    assert np.array_equal(out[1].values, work[1].values) and np.array_equal(out[1].alpha, work[1].alpha)
    again = [gclone(ps) for ps in work]
    with pytest.raises((psd_amd.SingularException, psd_amd.IllConditionedException)):  # raised after all four have run
        eng.zgordschur_batch_(again, sels)
    for q in (0, 2, 3):
        assert _same(again[q], out[q])


# ------------------------------------------------------------------------------------------------
# 8. fallback above the cap
def case_above_cap(make_engine, shape=CAP_SHAPE):
    """PSD_BORD_NMAX=16 at order 20: the single driver problem by problem on the batch buffers — the single calls' bits."""
    nb, n, p = shape[:3]
    eng = make_engine({"PSD_BORD_NMAX": "16"})
    for lr in "RL":
        probs, ps0, sels = inputs(eng, shape, lr)
        out = eng.zgordschur_batch_([gclone(ps) for ps in ps0], sels)
        assert eng.zgordschur_batch_stats.nlaunch_step > 1
        for q in range(nb):
            one = eng.ordschur_(gclone(ps0[q]), sels[q])
            assert _same(one, out[q]) and one.stats.nsweeps == out[q].stats.nsweeps > 0


# ------------------------------------------------------------------------------------------------
# 9. C ABI and arguments
def raw(eng, fn, nb, n, p, Tp, Zp, S, orient, si, sel, wantZ, alpha, beta, sc, infos=None, nsw=None, st=None):
    info = C.c_int(0)
    dp = C.POINTER(C.c_double)
    rc = fn(eng.ctx, nb, n, p, Tp, Zp, S, orient, si, sel.ctypes.data_as(C.POINTER(C.c_uint8)) if sel is not None else None,
            wantZ, alpha.view(np.float64).ctypes.data_as(dp) if alpha is not None else None,
            beta.ctypes.data_as(dp) if beta is not None else None,
            sc.ctypes.data_as(C.POINTER(C.c_int32)) if sc is not None else None,
            infos, nsw, C.byref(st) if st is not None else None, C.byref(info))
    assert rc == info.value
    return rc


def case_argument_codes(eng, shape=CHAIN_SHAPE):
    nb, n, p = shape[:3]
    probs, ps0, sels = inputs(eng, shape, "R")
    w = gclone(ps0[0])
    Tp, Zp = eng._ptrs(w.Ts), eng._ptrs(w.Z)
    buf = np.zeros((p, n, n), dtype=np.complex128)
    sel = np.ascontiguousarray(sels[0], dtype=np.uint8)
    alpha, beta, sc = np.zeros(n, dtype=np.complex128), np.zeros(n), np.zeros(n, dtype=np.int32)
    Sok = (C.c_uint8 * p)(*[1 if x else 0 for x in sig(shape, "R")])  # (T, F, T)
    Sbad = (C.c_uint8 * p)(0, 1, 1)
    Slast = (C.c_uint8 * p)(1, 1, 0)
    for fn, Tq, Zq in ((eng.lib.psd_z_gordschur_batch, Tp, Zp),
                       (eng.lib.psd_z_gordschur_batch_dev, C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data))):
        def f(nb_=1, n_=n, p_=p, T_=Tq, Z_=Zq, S_=Sok, o=b"R", si=1, sel_=sel, wz=1, a_=alpha, b_=beta, s_=sc):
            return raw(eng, fn, nb_, n_, p_, T_, Z_, S_, o, si, sel_, wz, a_, b_, s_)
        assert f(n_=0) == -2 and f(p_=0) == -3 and f(T_=None) == -4 and f(Z_=None) == -5 and f(o=b"X") == -6
        assert f(si=2) == -7 and f(si=0) == -7 and f(si=p + 1) == -7  # strictly inside, or outside, the period
        assert f(sel_=None) == -8 and f(a_=None) == -9 and f(b_=None) == -9 and f(s_=None) == -9 and f(nb_=-1) == -11
        # the entry of S that lands first in working order is that of the Schur factor: slot schurindex of the user's
        assert f(S_=Sbad) == -10 and f(S_=Sbad, o=b"L") == -10 and f(S_=Slast, si=p) == -10 and f(S_=Slast, o=b"L", si=p) == -10
        assert f(nb_=0) == 0 and f(nb_=0, T_=None) == 0 and f(nb_=0, S_=Sbad) == 0
        info = C.c_int(0)
        assert fn(None, 1, n, p, Tq, Zq, Sok, b"R", 1, sel.ctypes.data_as(C.POINTER(C.c_uint8)), 1, None, None, None, None,
                  None, None, C.byref(info)) == -1
    # a period-sharded context keeps a slice of Z: the batched entries refuse it (an engine of its own, let go afterwards)
    sharded = psd_amd.Engine(libpath=eng.lib._name)
    sharded.set_shard(0, 2)
    for fn, Tq, Zq in ((sharded.lib.psd_z_gordschur_batch, Tp, Zp),
                       (sharded.lib.psd_z_gordschur_batch_dev, C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data))):
        assert raw(sharded, fn, 1, n, p, Tq, Zq, Sok, b"R", 1, sel, 1, alpha, beta, sc) == psd_amd.INFO_NOTIMPL
        assert raw(sharded, fn, 0, n, p, Tq, Zq, Sok, b"R", 1, sel, 1, alpha, beta, sc) == 0
    with pytest.raises(psd_amd.NotImplementedPSD):
        sharded.zgordschur_batch_([gclone(ps0[0])], sels[:1])
    sharded.set_shard(0, 1)
    assert sharded.zgordschur_batch_([gclone(ps0[0])], sels[:1])[0].stats.nsweeps > 0  # (whole again: accepted)
    # (no refused call touched anything)
    assert _same(w, ps0[0]) and not buf.any() and not alpha.any() and not beta.any() and not sc.any()


def case_python_errors(eng):
    nb, n, p, S = CHAIN_SHAPE
    probs, ps0, sels = inputs(eng, CHAIN_SHAPE, "R")
    other = eng.pschur_(pt.bench_factors(9, p, seed=3, dtype=np.complex128), "R", S=list(S))
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zgordschur_batch([ps0[0], other], np.zeros(n, dtype=bool))  # unequal order
    left = eng.pschur_(pt.bench_factors(n, p, seed=4, dtype=np.complex128), "L", S=list(S))
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zgordschur_batch([ps0[0], left], sels[:2])  # unequal orientation
    otherS = eng.pschur_(pt.bench_factors(n, p, seed=5, dtype=np.complex128), "R", S=[True, True, False])
    with pytest.raises(psd_amd.DimensionMismatch, match="signatures"):
        eng.zgordschur_batch([ps0[0], otherS], sels[:2])  # unequal S
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zgordschur_batch(ps0[:2], np.zeros((2, n - 1), dtype=bool))  # select rows of the wrong length
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zgordschur_batch(ps0[:2], np.zeros((3, n), dtype=bool))  # ... or the wrong number of them
    # the entries without a signature keep refusing signed problems
    for fn in (eng.zordschur_batch, eng.zordschur_batch_):
        with pytest.raises(psd_amd.NotImplementedPSD, match="use ordschur_ per problem"):
            fn([gclone(ps0[0])], sels[:1])
    rl = eng.pschur_(pt.bench_factors(n, p, seed=3), "R", S=list(S))
    assert not np.iscomplexobj(rl.Ts[0])
    for fn in (eng.zgordschur_batch, eng.zgordschur_batch_):
        with pytest.raises(psd_amd.NotImplementedPSD, match="ComplexF64 only"):
            fn([rl], sels[:1])
    notf = gclone(ps0[0])
    notf.Ts[1] = np.ascontiguousarray(notf.Ts[1])
    with pytest.raises(TypeError):
        eng.zgordschur_batch_([notf], sels[:1])  # in place needs Fortran order
    ro = gclone(ps0[0])
    ro.Z[0].setflags(write=False)
    with pytest.raises(TypeError):
        eng.zgordschur_batch_([ro], sels[:1])  # ... and writable arrays
    mid = gclone(ps0[0])
    mid.schurindex = 2
    with pytest.raises(ValueError):
        eng.zgordschur_batch_([mid], sels[:1])  # interior schurindex (ordschur.jl:32)
    neg = gclone(ps0[0])
    neg.S = [False, True, True]
    with pytest.raises(ValueError):
        eng.zgordschur_batch_([neg], sels[:1])  # the Schur factor's entry of S is false
    assert eng.zgordschur_batch_([], sels) == [] and eng.zgordschur_batch([], sels[0]) == []
    infos = [7]
    assert eng.zgordschur_batch_([], sels, infos_out=infos) == [] and infos == []
    keep = gclone(ps0[0])
    got = eng.zgordschur_batch([ps0[0]], sels[:1])  # the copying form leaves its input alone
    assert _same(keep, ps0[0]) and got[0].stats.nsweeps > 0 and got[0].S == list(S)


# ------------------------------------------------------------------------------------------------
# 10. device entry through the C ABI
def case_dev_abi(eng, shape=CHAIN_SHAPE, launches=1, device=False):
    """psd_z_gordschur_batch_dev through the C ABI on packed [nb][p][n][n] column-major blocks — numpy arrays in the
    simulation, where device memory is host memory, torch CUDA tensors through data_ptr() on the GPU (device=True): the
    same bits as the host entry, for both alignments of each orientation.
    `launches`: the groups the engine's PSD_BATCH_GROUP cuts the batch into (the shifted alignments are then gathered a
    group at a time as well)."""
    nb, n, p = shape[:3]
    for lr in "RL":
        probs, ps0, sels = inputs(eng, shape, lr)
        si0 = ps0[0].schurindex
        for si in (si0, p + 1 - si0):
            # (the other alignment of the same orientation: the same factors and signature written shifted by one slot.
            #  Only the bits matter here.)
            shift = si != si0

            def placed(ps):
                q = gclone(ps)
                if shift:  # the triangular Schur factor goes from the first slot to the last, or back
                    rot = (lambda x: x[1:] + x[:1]) if si == p else (lambda x: x[-1:] + x[:-1])
                    q.Ts, q.Z, q.S = rot(q.Ts), rot(q.Z), rot(q.S)
                    q.schurindex = si
                return q
            host = eng.zgordschur_batch_([placed(ps) for ps in ps0], sels)
            hst = eng.zgordschur_batch_stats
            src = [placed(ps) for ps in ps0]
            Sarr = (C.c_uint8 * p)(*[1 if x else 0 for x in src[0].S])
            dT = np.ascontiguousarray(np.array([pt.pack(ps.Ts, np.complex128) for ps in src]))
            dZ = np.ascontiguousarray(np.array([pt.pack(ps.Z, np.complex128) for ps in src]))
            if device:
                import torch

                gT, gZ = torch.from_numpy(dT).cuda(), torch.from_numpy(dZ).cuda()
                assert gT.is_contiguous() and gZ.is_contiguous()
                torch.cuda.synchronize()
                pT, pZ = C.c_void_p(gT.data_ptr()), C.c_void_p(gZ.data_ptr())
            else:
                pT, pZ = C.c_void_p(dT.ctypes.data), C.c_void_p(dZ.ctypes.data)
            alpha, beta = np.zeros((nb, n), dtype=np.complex128), np.zeros((nb, n))
            sc = np.zeros((nb, n), dtype=np.int32)
            infos, nsw = (C.c_int * nb)(), (C.c_int * nb)()
            st = psd_amd.Stats()
            sel = np.ascontiguousarray(sels, dtype=np.uint8)
            rc = raw(eng, eng.lib.psd_z_gordschur_batch_dev, nb, n, p, pT, pZ, Sarr, lr.encode(), si, sel, 1, alpha, beta,
                     sc, infos, nsw, st)
            if device:  # (the entry returns with its stream drained)
                dT, dZ = gT.cpu().numpy(), gZ.cpu().numpy()
            assert rc == 0 and not any(infos) and st.nlaunch_step == hst.nlaunch_step == launches and st.window == hst.window
            assert st.nsweeps == hst.nsweeps == sum(nsw) > 0 and st.ms_total >= 0
            for q in range(nb):
                assert nsw[q] == host[q].stats.nsweeps
                assert np.array_equal(pt.gvalues(alpha[q], beta[q], sc[q]), host[q].values)
                for j in range(p):
                    assert np.array_equal(dT[q, j].T, host[q].Ts[j]) and np.array_equal(dZ[q, j].T, host[q].Z[j]), (lr, si, q, j)


# ------------------------------------------------------------------------------------------------
# 11. device-resident chain (GPU tier)
def case_device_chain(eng, lr, shape=CHAIN_SHAPE):
    """zgpschur_batch_ -> zgordschur_batch_ without a matrix touching the host"""
    import torch

    nb, n, p = shape[:3]
    S = sig(shape, lr)
    probs = factors(shape)
    si = p if lr == "L" else 1
    dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in probs])).cuda()
    T, Z, values, _ = eng.zgpschur_batch_(dA, S, lr)
    sels = np.array([median_select(v) for v in values])
    ps0 = [psd_amd.GeneralizedPeriodicSchur(S, [np.asfortranarray(T[q, j].cpu().numpy()) for j in range(p)],
                                            [np.asfortranarray(Z[q, j].cpu().numpy()) for j in range(p)], values[q].copy(),
                                            np.ones(n), np.zeros(n, dtype=np.int32), lr, si) for q in range(nb)]
    host = eng.zgordschur_batch_([gclone(ps) for ps in ps0], sels)
    T1, Z1, values1, st = eng.zgordschur_batch_(T, Z, sels, S=S, lr=lr, schurindex=si)
    assert T1.data_ptr() == T.data_ptr() and Z1.data_ptr() == Z.data_ptr()  # in place
    assert T1.stride() == T.stride() and Z1.stride() == Z.stride()
    assert st.nlaunch_step == 1 and tuple(T1.shape) == (nb, p, n, n)
    Th, Zh = T1.cpu().numpy(), Z1.cpu().numpy()
    for q in range(nb):
        sc = max(np.linalg.norm(a, 2) for a in probs[q])
        assert np.abs(values1[q] - host[q].values).max() <= 1e-12 * np.abs(host[q].values).max()
        for j in range(p):
            assert np.abs(Th[q, j] - host[q].Ts[j]).max() <= 1e-12 * sc, (lr, q, j)
            assert np.abs(Zh[q, j] - host[q].Z[j]).max() <= 1e-12, (lr, q, j)
        ps1 = psd_amd.GeneralizedPeriodicSchur(S, [np.asfortranarray(Th[q, j]) for j in range(p)],
                                               [np.asfortranarray(Zh[q, j]) for j in range(p)], values1[q], np.ones(n),
                                               np.zeros(n, dtype=np.int32), lr, si)
        ps1.stats = psd_amd.Stats()
        ps1.stats.nsweeps = int(eng.zgordschur_batch_nswaps[q])
        check_problem(probs[q], ps0[q], ps1, sels[q], nswaps=host[q].stats.nsweeps)
    # any other layout is copied first: the input stays as it was
    Tc = T1.contiguous()
    keep = Tc.clone()
    T2, Z2, v2, _ = eng.zgordschur_batch_(Tc, Z1.contiguous(), np.ones((nb, n), dtype=bool), S=S, lr=lr, schurindex=si)
    assert T2.data_ptr() != Tc.data_ptr() and torch.equal(Tc, keep) and torch.equal(T2, Tc)
    Tn, Zn, vn, _ = eng.zgordschur_batch(T1, None, sels, S=S, lr=lr, schurindex=si, wantZ=False)  # copying form, no Z
    assert Zn is None and Tn.data_ptr() != T1.data_ptr() and torch.equal(T1.cpu(), torch.from_numpy(Th))
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zgordschur_batch_(T1[:, :, :, :5], None, sels, S=S, lr=lr, schurindex=si, wantZ=False)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zgordschur_batch_(T1, None, sels, S=S[:-1], lr=lr, schurindex=si, wantZ=False)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.zgordschur_batch_(T1.real.contiguous(), None, sels, S=S, lr=lr, schurindex=si, wantZ=False)
    with pytest.raises(ValueError):
        eng.zgordschur_batch_(T1, Z1, sels, S=S, lr=lr, schurindex=2)
    # an empty batch is returned as it is and describes itself like any other call
    infos = [7]
    T0, Z0, v0, st0 = eng.zgordschur_batch_(T1[:0], Z1[:0], sels[:0], S=S, lr=lr, schurindex=si, infos_out=infos)
    assert T0.shape[0] == 0 and v0.shape == (0, n) and infos == [] and st0.nlaunch_step == 0
    assert eng.zgordschur_batch_stats.nsweeps == 0 and len(eng.zgordschur_batch_nswaps) == 0
