"""Engine.dgordschur_batch_ / dgordschur_batch (psd_d_gordschur_batch / psd_d_gordschur_batch_dev, csrc/psd_gbord.h): many
small signed Float64 periodic Schur forms reordered in one call — the cases shared by the simulated tier
(test_hostsim_dgordschur_batch.py) and the device tier (test_gpu_dgordschur_batch.py), the real counterparts of
zgord_batch_cases and the signed counterparts of ord_batch_cases.  Inputs are dgpschur_batch results of the factors of
batch_cases.DG (pt.bench_factors(n, p, seed=9000 + 131 q + 7 n + p)) with one signature per shape (reversed for 'L') and
the eigenvalues at or below the median modulus selected (row 2 alone for n = 2).  Random real factors give real
eigenvalues and conjugate pairs side by side, so a batch contains the 1x1 and the 2x2 signed swaps; every problem of
(4, 2, 2) has a real spectrum.  pt.oracle_gordschur accepts every swap of the first six problems of every shape
(asserted).

Bounds: pt.rgpschur_check with those of engine_cases.case_gordschur_pairs_random (400 and 10 times max(1, sqrt(n / 32))
units of eps); the selected and unselected eigenvalue groups to 1e-8 max|lambda| (the same case); against the single call
1e-9 max|lambda| (the bound of the oracle comparisons of engine_cases.case_gordschur_pairs_reference)."""
import ctypes as C

import numpy as np
import pytest

import batch_cases as bc
import psd_amd
import psdtest as pt
from batch_cases import real_form
from batch_common import SIG22, shape_id, sig
from ord_batch_cases import median_select
from zgord_batch_cases import gclone, oracle, raw, select_for

T, F = True, False

# (nb, n, p, S for 'R') and what each covers; for 'L' the signature is reversed (true entry last)
WINDOW_SHAPES = [
    (3, 48, 3, (T, F, T)),       # W = 25 < n: several windows, all off-window roles on both sides
    (2, 40, 22, SIG22),          # W = 24
    (2, 30, 70, tuple(q % 2 == 0 for q in range(70))),  # W = 6: the per-factor scratch near the LDS limit
    (33, 12, 3, (T, F, T)),      # more problems than a 32-wide chunk, n < W
    (3, 5, 2, (T, F)),           # a pencil (problem 2 needs no swap in 'L')
    (4, 2, 2, (T, F)),           # smallest window; row 2 alone is selected; real spectra only
    (3, 1, 3, (T, F, T)),        # n = 1: no swap
    (3, 33, 4, (T, T, F, T)),    # signature class: a positive factor beside a negative one
    (3, 20, 4, (T, F, F, T)),    # signature class: adjacent negative factors
    (4, 7, 5, (T, F, T, F, T)),  # odd order, alternating signature
]
NARROW_SHAPE = (3, 20, 3, (T, F, T))  # with PSD_BORD_W=6: several narrow windows
GROUP_SHAPE = (6, 20, 3, (T, T, F))   # the group loop under PSD_BATCH_GROUP=4
CAP_SHAPE = (2, 20, 3, (T, F, T))
CHAIN_SHAPE = (5, 12, 3, (T, F, T))
NORACLE = 6  # the oracle runs on the first six problems of a shape

_cache = {}


def expected_window(n, p):
    """bord_real::window (csrc/psd_bord_host.inl): the candidates of choose_window_rord under rord_lds_bytes, the
    smallest that holds the whole problem if it fits, otherwise the widest that fits, and at most PSD_BORD_SPAN1 = 25."""
    W = 0
    for w in (32, 24, 20, 16, 12, 10, 8, 6):
        if _lds_bytes(p, w) > 155 * 1024:
            continue
        if W == 0 or w >= n:
            W = w
    return min(W, 25)


def _lds_bytes(p, w):
    """rord_lds_bytes (csrc/psd_engine.cpp) with psd_rord_tree_doubles (csrc/psd_rord.h)"""
    tree = (2 * p + 8) * 36 + 4 * 104 + 4 * 12 + (7 * p + 16 + 32 + 1) // 2 + 8
    b = (p * w * (w + 1) + p * (96 + 52) + 4 + 192 + tree) * 8 + p * 5 + 80
    return (b + 15) // 16 * 16


def closed_select(lam0, select):
    """the selection closed under conjugation, as the device closes it"""
    closed = np.array(select, dtype=bool).copy()
    for i in range(len(lam0) - 1):
        if lam0[i].imag > 0 and (select[i] or select[i + 1]):
            closed[i] = closed[i + 1] = True
    return closed


def inputs(eng, shape, lr):
    """(factors, decompositions, selections) of a shape and orientation: computed once per library (the engines of a tier
    differ in the knobs of the reordering only) and only cloned."""
    key = (eng.lib._name, shape, lr)
    if key not in _cache:
        probs = bc.problems(bc.DG, shape)
        ps0 = eng.dgpschur_batch(probs, sig(shape, lr), lr)
        sels = np.array([select_for(shape, ps.values) for ps in ps0])
        _cache[key] = (probs, ps0, sels)
    return _cache[key]


def single(eng, shape, lr, q):
    """ordschur_ of problem q on `eng`: computed once, never written to."""
    key = ("single", id(eng), shape, lr, q)
    if key not in _cache:
        probs, ps0, sels = inputs(eng, shape, lr)
        _cache[key] = (eng.ordschur_(gclone(ps0[q]), sels[q]), eng)
    return _cache[key][0]


def has_pair(ps):
    return bool(np.any(ps.values.imag != 0))


def check_problem(A, ps0, ps1, select, oracle_run=True, nswaps=None, one=None, what=None):
    """The checks of case 1 (windows) for one problem; returns the swap count."""
    n = A[0].shape[0]
    lam0 = ps0.values
    assert ps1.S == ps0.S
    pt.rgpschur_check(A, ps0.S, ps1, tol=400 * max(1.0, np.sqrt(n / 32)), qtol=10 * max(1.0, np.sqrt(n / 32)))
    real_form(ps1, what)
    assert np.array_equal(ps1.values, pt.gvalues(ps1.alpha, ps1.beta, ps1.alphascale))
    closed = closed_select(lam0, select)
    m = int(closed.sum())
    sc = abs(lam0).max()
    assert pt.match_eigs(lam0[closed], ps1.values[:m]) < 1e-8 * sc
    assert pt.match_eigs(lam0[~closed], ps1.values[m:]) < 1e-8 * sc
    if oracle_run:
        po = oracle(ps0, select)
        assert po.info == 0 and ps1.stats.nsweeps == po.nswaps, (what, ps1.stats.nsweeps, po.nswaps)
    if nswaps is not None:
        assert ps1.stats.nsweeps == nswaps, (what, ps1.stats.nsweeps, nswaps)
    if one is not None:
        err = pt.match_eigs(one.values, ps1.values)
        print(f"{what}: |lam - single call| = {err:.3e} (bound {1e-9 * sc:.3e}), {ps1.stats.nsweeps} swaps")
        assert err < 1e-9 * sc, (what, err)
    return ps1.stats.nsweeps


def _same(a, b):
    return (np.array_equal(a.values, b.values) and np.array_equal(a.alpha, b.alpha) and np.array_equal(a.beta, b.beta)
            and np.array_equal(a.alphascale, b.alphascale) and all(np.array_equal(x, y) for x, y in zip(a.Ts, b.Ts))
            and all(np.array_equal(x, y) for x, y in zip(a.Z, b.Z)))


# ------------------------------------------------------------------------------------------------
# 1. windows
def case_windows(eng, shape, lr, expect_window=None):
    nb, n, p = shape[:3]
    probs, ps0, sels = inputs(eng, shape, lr)
    out = eng.dgordschur_batch_([gclone(ps) for ps in ps0], sels)
    st = eng.dgordschur_batch_stats
    assert len(out) == nb and st.nlaunch_step == 1 and st.nsweeps == sum(ps.stats.nsweeps for ps in out)
    assert list(eng.dgordschur_batch_nswaps) == [ps.stats.nsweeps for ps in out]
    if expect_window is not None:
        assert st.window == expect_window and st.nwindows > nb  # (several windows per problem)
    else:
        assert st.window == expected_window(n, p), (st.window, expected_window(n, p))
    noz = eng.dgordschur_batch_([gclone(ps) for ps in ps0], sels, wantZ=False)
    total = 0
    for q in range(nb):
        one = single(eng, shape, lr, q)
        total += check_problem(probs[q], ps0[q], out[q], sels[q], oracle_run=q < NORACLE, nswaps=one.stats.nsweeps, one=one,
                               what=(shape_id(shape), lr, q))
        sc = abs(ps0[q].values).max()
        # wantZ = false leaves Z untouched and gives the same T
        assert all(np.array_equal(a, b) for a, b in zip(noz[q].Z, ps0[q].Z))
        assert max(np.abs(a - b).max() for a, b in zip(noz[q].Ts, out[q].Ts)) < 1e-12 * sc
    assert (total > 0) == (n > 1)  # (per shape: a problem may need no swap)
    if n == 2:
        assert not any(has_pair(ps) for ps in ps0)
    elif n > 2:  # real eigenvalues and pairs side by side: the 1x1 and the 2x2 signed swaps
        assert any(has_pair(ps) for ps in ps0) and any(np.any(ps.values.imag == 0) for ps in ps0)


# ------------------------------------------------------------------------------------------------
# 2. reference shapes
def case_reference(eng, lr):
    """engine_cases.case_gordschur_reference(cplx=False) per problem of a batch: (nb, n, p) = (4, 7, 5), spectrum 4^j."""
    nb, n, p, nsel = 4, 7, 5, 2
    S = [True] * p
    for l in range(0, p - 1, 2):
        S[l] = False
    probs = [pt.gord_test_factors(n, p, S, seed=31 + 37 * q, cplx=False) for q in range(nb)]
    if lr == "R":
        probs, S = [A[::-1] for A in probs], S[::-1]
    ps0 = eng.dgpschur_batch(probs, S, lr)
    for q in range(nb):
        pt.rgpschur_check(probs[q], S, ps0[q])
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
        out = eng.dgordschur_batch_([gclone(ps) for ps in ps0], np.array(sels))
        assert eng.dgordschur_batch_stats.nlaunch_step == 1
        for q in range(nb):
            pt.rgpschur_check(probs[q], S, out[q])
            real_form(out[q], (lr, which, q))
            for j in range(nsel):
                assert np.any(np.isclose(out[q].values[:nsel], ps0[q].values[idxs[q][j]], rtol=1e-8))
            po = oracle(ps0[q], sels[q])
            assert po.info == 0 and out[q].stats.nsweeps == po.nswaps
            assert pt.match_eigs(po.values, out[q].values) < 1e-9 * abs(po.values).max()


def case_pairs_reference(eng):
    """engine_cases.case_gordschur_pairs_reference as ONE batch: mkrps(7, 5, [3, 6], alt=True) with its six selection
    sets, against the oracle at its 1e-9."""
    n, p = 7, 5
    ps0, A = pt.mkrps(n, p, [3, 6], seed=905, alt=True)
    lam0 = ps0.values
    selsets = ([6, 7], [3, 4], [1, 2, 5], [1, 3, 4], [1, 2, 6, 7], [5])
    sels = np.zeros((len(selsets), n), dtype=bool)
    for q, ss in enumerate(selsets):
        sels[q, [j - 1 for j in ss]] = True
    work = [psd_amd.GeneralizedPeriodicSchur(ps0.S, [t.copy(order="F") for t in ps0.Ts], [z.copy(order="F") for z in ps0.Z],
                                             ps0.alpha.copy(), ps0.beta.copy(), ps0.ascale.copy(), "L", p) for _ in selsets]
    out = eng.dgordschur_batch_(work, sels)
    assert eng.dgordschur_batch_stats.nlaunch_step == 1
    for q, ss in enumerate(selsets):
        pt.rgpschur_check(A, ps0.S, out[q], tol=400)
        real_form(out[q], ss)
        for j in ss:
            assert np.any(np.isclose(out[q].values[:len(ss)], lam0[j - 1], rtol=1e-7)), (ss, out[q].values)
        po = pt.oracle_gordschur(ps0, sels[q])
        assert po.info == 0 and po.nswaps == out[q].stats.nsweeps
        assert pt.match_eigs(po.values, out[q].values) < 1e-9 * abs(po.values).max()


# ------------------------------------------------------------------------------------------------
# 3. independence and groups
def case_independence(eng, shape, lr="R"):
    """A problem alone in a batch of one gets, bit for bit, what it gets inside the batch."""
    nb, n, p = shape[:3]
    probs, ps0, sels = inputs(eng, shape, lr)
    out = eng.dgordschur_batch_([gclone(ps) for ps in ps0], sels)
    for q in sorted({0, nb - 2, nb - 1} & set(range(nb))):
        alone = eng.dgordschur_batch_([gclone(ps0[q])], sels[q:q + 1])
        assert _same(alone[0], out[q]), (shape_id(shape), q)


def case_groups(make_engine, shape=GROUP_SHAPE):
    """PSD_BATCH_GROUP=4: a batch worked through in two groups equals one group bit for bit."""
    nb, n, p = shape[:3]
    ref = make_engine({})
    eng = make_engine({"PSD_BATCH_GROUP": "4"})
    probs, ps0, sels = inputs(ref, shape, "L")
    whole = ref.dgordschur_batch_([gclone(ps) for ps in ps0], sels)
    assert ref.dgordschur_batch_stats.nlaunch_step == 1
    parts = eng.dgordschur_batch_([gclone(ps) for ps in ps0], sels)
    assert eng.dgordschur_batch_stats.nlaunch_step == 2
    for q in range(nb):
        assert _same(whole[q], parts[q]), q
        assert whole[q].stats.nsweeps == parts[q].stats.nsweeps > 0


# ------------------------------------------------------------------------------------------------
# 4. fallback above the cap
def case_above_cap(make_engine, shape=CAP_SHAPE):
    """PSD_BORD_NMAX=16 at order 20: the real signed single driver problem by problem on the batch buffers.  A problem
    that contains a pair gets the single call's bits; one with a real spectrum, which the single call promotes to the
    complex kernel, goes through the checks of case 1."""
    nb, n, p = shape[:3]
    eng = make_engine({"PSD_BORD_NMAX": "16"})
    for lr in "RL":
        probs, ps0, sels = inputs(eng, shape, lr)
        out = eng.dgordschur_batch_([gclone(ps) for ps in ps0], sels)
        assert eng.dgordschur_batch_stats.nlaunch_step > 1
        for q in range(nb):
            one = eng.ordschur_(gclone(ps0[q]), sels[q])
            check_problem(probs[q], ps0[q], out[q], sels[q], nswaps=one.stats.nsweeps, one=one, what=("cap", lr, q))
            assert out[q].stats.nsweeps > 0
            if has_pair(ps0[q]):
                assert _same(one, out[q]), (lr, q)


# ------------------------------------------------------------------------------------------------
# 5. all-true / NULL signature
def case_all_true(eng, shape=CHAIN_SHAPE):
    """A null or all-true S is accepted and stays on the signed kernels: the result is in the scaled form, with the swap
    counts of ordschur_batch_ on the same factors and its eigenvalues to 1e-9 * scale."""
    nb, n, p = shape[:3]
    probs = bc.problems(bc.DG, shape)
    for lr in "RL":
        ps0 = eng.dgpschur_batch(probs, None, lr)
        assert all(ps.S == [True] * p for ps in ps0)
        sels = np.array([median_select(ps.values) for ps in ps0])

        def plain():
            return [psd_amd.PeriodicSchur([t.copy(order="F") for t in ps.Ts], [z.copy(order="F") for z in ps.Z],
                                          ps.values.copy(), lr, ps.schurindex) for ps in ps0]
        ref = eng.ordschur_batch_(plain(), sels)
        assert eng.ordschur_batch_stats.nsweeps > 0
        out = eng.dgordschur_batch_([gclone(ps) for ps in ps0], sels)
        assert eng.dgordschur_batch_stats.nsweeps == eng.ordschur_batch_stats.nsweeps
        for q in range(nb):
            sc = abs(ps0[q].values).max()
            assert out[q].stats.nsweeps == ref[q].stats.nsweeps
            assert np.array_equal(out[q].values, pt.gvalues(out[q].alpha, out[q].beta, out[q].alphascale))
            assert pt.match_eigs(ref[q].values, out[q].values) < 1e-9 * sc
            check_problem(probs[q], ps0[q], out[q], sels[q], oracle_run=False, what=("all-true", lr, q))
        for Sarr in (None, (C.c_uint8 * p)(*[1] * p)):
            work = plain()
            flatT, flatZ = [t for ps in work for t in ps.Ts], [z for ps in work for z in ps.Z]
            alpha, beta = np.zeros((nb, n), dtype=np.complex128), np.zeros((nb, n))
            sc = np.zeros((nb, n), dtype=np.int32)
            nsw = (C.c_int * nb)()
            rc = raw(eng, eng.lib.psd_d_gordschur_batch, nb, n, p, eng._ptrs(flatT), eng._ptrs(flatZ), Sarr, lr.encode(),
                     ps0[0].schurindex, np.ascontiguousarray(sels, dtype=np.uint8), 1, alpha, beta, sc, None, nsw)
            assert rc == 0
            for q in range(nb):
                assert nsw[q] == ref[q].stats.nsweeps
                assert np.array_equal(pt.gvalues(alpha[q], beta[q], sc[q]), out[q].values)
                assert all(np.array_equal(a, b) for a, b in zip(work[q].Ts + work[q].Z, out[q].Ts + out[q].Z))


# ------------------------------------------------------------------------------------------------
# 6. per-problem selections
def case_selections(eng):
    """all-false, all-true, the median rule and one member of a pair side by side in one batch; one row for every
    problem"""
    shape = (1, 8, 3, (T, F, T))
    n = shape[1]
    probs, ps0, _ = inputs(eng, shape, "R")
    A, ps0 = probs[0], ps0[0]
    lam0 = ps0.values
    pairs = [i for i in range(1, n - 1) if lam0[i].imag > 0]  # (a pair that does not stand at the top)
    assert pairs
    sels = np.zeros((5, n), dtype=bool)
    sels[1] = True
    sels[2] = median_select(lam0)
    sels[3, pairs[-1]] = True      # the first member of a pair alone
    sels[4, pairs[-1] + 1] = True  # the second member alone
    out = eng.dgordschur_batch_([gclone(ps0) for _ in range(5)], sels)
    assert out[0].stats.nsweeps == 0 and out[1].stats.nsweeps == 0
    for o in out[:2]:
        assert all(np.array_equal(a, b) for a, b in zip(o.Ts + o.Z, ps0.Ts + ps0.Z))  # untouched bit for bit
        assert np.allclose(o.values, lam0, rtol=1e-13, atol=0)  # (recomputed from the same diagonal blocks)
    assert check_problem(A, ps0, out[2], sels[2], what="median") > 0
    for q in (3, 4):  # one member of a pair takes its partner along
        assert check_problem(A, ps0, out[q], sels[q], what="pair member") > 0
        assert pt.match_eigs(out[q].values[:2], lam0[pairs[-1]:pairs[-1] + 2]) < 1e-8 * abs(lam0).max()
    assert _same(out[3], out[4])
    one = eng.dgordschur_batch_([gclone(ps0) for _ in range(3)], sels[2])  # one row for every problem
    assert all(_same(o, out[2]) for o in one)


# ------------------------------------------------------------------------------------------------
# 7. one problem fails
def singular_problem():
    """n = 4, p = 2, S = (T, F), 'R', Z = I: both factors triu(ones) with T1[3, 2] = -1, a 2x2 block at rows 3:4 (which
    keeps the single call on the real driver); row 2 is selected, and rows 1 and 2 carry the same eigenvalue 1.  All
    entries are small integers, so contraction cannot change the outcome.  The values are those of the product
    T1 inv(T2), written down by hand: 1, 1 and the block's 1 and 2."""
    n, p = 4, 2
    Ts = [np.asfortranarray(np.triu(np.ones((n, n)))) for _ in range(p)]
    Ts[0][3, 2] = -1.0
    Z = [np.asfortranarray(np.eye(n)) for _ in range(p)]
    alpha = np.array([1.0, 1.0, 1.0, 2.0], dtype=np.complex128)
    assert pt.match_eigs(np.linalg.eigvals(Ts[0] @ np.linalg.inv(Ts[1])), alpha) < 1e-7  # (a triple eigenvalue)
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
    with pytest.raises(psd_amd.SingularException):
        eng.ordschur_(gclone(work[1]), sels[1])  # (the single call on the same engine rejects it: the yardstick)
    infos = []
    out = eng.dgordschur_batch_([gclone(ps) for ps in work], sels, infos_out=infos)
    assert len(infos) == 4 and infos[0] == 0 and infos[2] == 0 and infos[3] == 0, infos
    assert infos[1] == 3000, infos
    for q in (0, 2, 3):
        check_problem(probs[q], work[q], out[q], sels[q], what=("one fails", q))
    # the failed problem is still a decomposition of its product — the rejected swap left the factors as they were, and
    # Z = I —, with its old values
    assert all(np.array_equal(a, b) for a, b in zip(out[1].Ts + out[1].Z, work[1].Ts + work[1].Z))
    for l in range(2):
        assert np.array_equal(out[1].Z[l] @ out[1].Ts[l] @ out[1].Z[1 - l].T, probs[1][l])
    assert np.array_equal(out[1].values, work[1].values) and np.array_equal(out[1].alpha, work[1].alpha)
    again = [gclone(ps) for ps in work]
    with pytest.raises(psd_amd.SingularException):  # raised after all four have run
        eng.dgordschur_batch_(again, sels)
    for q in (0, 2, 3):
        assert _same(again[q], out[q])


# ------------------------------------------------------------------------------------------------
# 8. C ABI and arguments
def case_argument_codes(eng, shape=CHAIN_SHAPE):
    nb, n, p = shape[:3]
    probs, ps0, sels = inputs(eng, shape, "R")
    w = gclone(ps0[0])
    Tp, Zp = eng._ptrs(w.Ts), eng._ptrs(w.Z)
    buf = np.zeros((p, n, n))
    sel = np.ascontiguousarray(sels[0], dtype=np.uint8)
    alpha, beta, sc = np.zeros(n, dtype=np.complex128), np.zeros(n), np.zeros(n, dtype=np.int32)
    Sok = (C.c_uint8 * p)(*[1 if x else 0 for x in sig(shape, "R")])  # (T, F, T)
    Sbad = (C.c_uint8 * p)(0, 1, 1)
    Slast = (C.c_uint8 * p)(1, 1, 0)
    for fn, Tq, Zq in ((eng.lib.psd_d_gordschur_batch, Tp, Zp),
                       (eng.lib.psd_d_gordschur_batch_dev, C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data))):
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
    for fn, Tq, Zq in ((sharded.lib.psd_d_gordschur_batch, Tp, Zp),
                       (sharded.lib.psd_d_gordschur_batch_dev, C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data))):
        assert raw(sharded, fn, 1, n, p, Tq, Zq, Sok, b"R", 1, sel, 1, alpha, beta, sc) == psd_amd.INFO_NOTIMPL
        assert raw(sharded, fn, 0, n, p, Tq, Zq, Sok, b"R", 1, sel, 1, alpha, beta, sc) == 0
    with pytest.raises(psd_amd.NotImplementedPSD):
        sharded.dgordschur_batch_([gclone(ps0[0])], sels[:1])
    sharded.set_shard(0, 1)
    assert sharded.dgordschur_batch_([gclone(ps0[0])], sels[:1])[0].stats.nsweeps > 0  # (whole again: accepted)
    # (no refused call touched anything)
    assert _same(w, ps0[0]) and not buf.any() and not alpha.any() and not beta.any() and not sc.any()


def case_python_errors(eng):
    nb, n, p, S = CHAIN_SHAPE
    probs, ps0, sels = inputs(eng, CHAIN_SHAPE, "R")
    other = eng.pschur_(bc.work(bc.DG, pt.bench_factors(9, p, seed=3)), "R", S=list(S))
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgordschur_batch([ps0[0], other], np.zeros(n, dtype=bool))  # unequal order
    left = eng.pschur_(bc.work(bc.DG, pt.bench_factors(n, p, seed=4)), "L", S=list(S))
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgordschur_batch([ps0[0], left], sels[:2])  # unequal orientation
    otherS = eng.pschur_(bc.work(bc.DG, pt.bench_factors(n, p, seed=5)), "R", S=[True, True, False])
    with pytest.raises(psd_amd.DimensionMismatch, match="signatures"):
        eng.dgordschur_batch([ps0[0], otherS], sels[:2])  # unequal S
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgordschur_batch(ps0[:2], np.zeros((2, n - 1), dtype=bool))  # select rows of the wrong length
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgordschur_batch(ps0[:2], np.zeros((3, n), dtype=bool))  # ... or the wrong number of them
    # the entries without a signature keep refusing signed problems
    for fn in (eng.ordschur_batch, eng.ordschur_batch_):
        with pytest.raises(psd_amd.NotImplementedPSD, match="use ordschur_ per problem"):
            fn([gclone(ps0[0])], sels[:1])
    # each signed entry names the other one for a problem of the other element type
    for fn in (eng.zgordschur_batch, eng.zgordschur_batch_):
        with pytest.raises(psd_amd.NotImplementedPSD, match="ComplexF64 only.*dgordschur_batch"):
            fn([gclone(ps0[0])], sels[:1])
    cx = eng.pschur_(pt.bench_factors(n, p, seed=3, dtype=np.complex128), "R", S=list(S))
    assert np.iscomplexobj(cx.Ts[0])
    for fn in (eng.dgordschur_batch, eng.dgordschur_batch_):
        with pytest.raises(psd_amd.NotImplementedPSD, match="Float64 only.*zgordschur_batch"):
            fn([cx], sels[:1])
    notf = gclone(ps0[0])
    notf.Ts[1] = np.ascontiguousarray(notf.Ts[1])
    with pytest.raises(TypeError):
        eng.dgordschur_batch_([notf], sels[:1])  # in place needs Fortran order
    ro = gclone(ps0[0])
    ro.Z[0].setflags(write=False)
    with pytest.raises(TypeError):
        eng.dgordschur_batch_([ro], sels[:1])  # ... and writable arrays
    mid = gclone(ps0[0])
    mid.schurindex = 2
    with pytest.raises(ValueError):
        eng.dgordschur_batch_([mid], sels[:1])  # interior schurindex (rordschur.jl:25)
    neg = gclone(ps0[0])
    neg.S = [False, True, True]
    with pytest.raises(ValueError):
        eng.dgordschur_batch_([neg], sels[:1])  # the Schur factor's entry of S is false
    assert eng.dgordschur_batch_([], sels) == [] and eng.dgordschur_batch([], sels[0]) == []
    infos = [7]
    assert eng.dgordschur_batch_([], sels, infos_out=infos) == [] and infos == []
    keep = gclone(ps0[0])
    got = eng.dgordschur_batch([ps0[0]], sels[:1])  # the copying form leaves its input alone
    assert _same(keep, ps0[0]) and got[0].stats.nsweeps > 0 and got[0].S == list(S)
    assert got[0].Ts[0].dtype == np.float64 and not _same(got[0], ps0[0])


# ------------------------------------------------------------------------------------------------
# 9. device entry through the C ABI
def case_dev_abi(eng, shape=CHAIN_SHAPE, launches=1, device=False):
    """psd_d_gordschur_batch_dev through the C ABI on packed [nb][p][n][n] column-major blocks — numpy arrays in the
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
                if shift:  # the quasi-triangular Schur factor goes from the first slot to the last, or back
                    rot = (lambda x: x[1:] + x[:1]) if si == p else (lambda x: x[-1:] + x[:-1])
                    q.Ts, q.Z, q.S = rot(q.Ts), rot(q.Z), rot(q.S)
                    q.schurindex = si
                return q
            host = eng.dgordschur_batch_([placed(ps) for ps in ps0], sels)
            hst = eng.dgordschur_batch_stats
            src = [placed(ps) for ps in ps0]
            Sarr = (C.c_uint8 * p)(*[1 if x else 0 for x in src[0].S])
            dT = np.ascontiguousarray(np.array([pt.pack(ps.Ts, np.float64) for ps in src]))
            dZ = np.ascontiguousarray(np.array([pt.pack(ps.Z, np.float64) for ps in src]))
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
            rc = raw(eng, eng.lib.psd_d_gordschur_batch_dev, nb, n, p, pT, pZ, Sarr, lr.encode(), si, sel, 1, alpha, beta,
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
# 10. device-resident chain (GPU tier)
def case_device_chain(eng, lr, shape=CHAIN_SHAPE):
    """dgpschur_batch_ -> dgordschur_batch_ without a matrix touching the host"""
    import torch

    nb, n, p = shape[:3]
    S = sig(shape, lr)
    probs = bc.problems(bc.DG, shape)
    si = p if lr == "L" else 1
    dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in probs])).cuda()
    T, Z, values, _ = eng.dgpschur_batch_(dA, S, lr)
    assert T.dtype == torch.float64 and Z.dtype == torch.float64
    sels = np.array([median_select(v) for v in values])
    ps0 = [psd_amd.GeneralizedPeriodicSchur(S, [np.asfortranarray(T[q, j].cpu().numpy()) for j in range(p)],
                                            [np.asfortranarray(Z[q, j].cpu().numpy()) for j in range(p)], values[q].copy(),
                                            np.ones(n), np.zeros(n, dtype=np.int32), lr, si) for q in range(nb)]
    host = eng.dgordschur_batch_([gclone(ps) for ps in ps0], sels)
    T1, Z1, values1, st = eng.dgordschur_batch_(T, Z, sels, S=S, lr=lr, schurindex=si)
    assert T1.data_ptr() == T.data_ptr() and Z1.data_ptr() == Z.data_ptr()  # in place
    assert T1.stride() == T.stride() and Z1.stride() == Z.stride()
    assert st.nlaunch_step == 1 and tuple(T1.shape) == (nb, p, n, n) and T1.dtype == torch.float64
    Th, Zh = T1.cpu().numpy(), Z1.cpu().numpy()
    for q in range(nb):
        assert np.array_equal(values1[q], host[q].values)  # (the same kernels on the same bits)
        for j in range(p):
            assert np.array_equal(Th[q, j], host[q].Ts[j]) and np.array_equal(Zh[q, j], host[q].Z[j]), (lr, q, j)
        ps1 = psd_amd.GeneralizedPeriodicSchur(S, [np.asfortranarray(Th[q, j]) for j in range(p)],
                                               [np.asfortranarray(Zh[q, j]) for j in range(p)], host[q].alpha,
                                               host[q].beta, host[q].alphascale, lr, si)
        ps1.stats = psd_amd.Stats()
        ps1.stats.nsweeps = int(eng.dgordschur_batch_nswaps[q])
        check_problem(probs[q], ps0[q], ps1, sels[q], nswaps=host[q].stats.nsweeps, what=("chain", lr, q))
    # any other layout is copied first: the input stays as it was
    Tc = T1.contiguous()
    keep = Tc.clone()
    T2, Z2, v2, _ = eng.dgordschur_batch_(Tc, Z1.contiguous(), np.ones((nb, n), dtype=bool), S=S, lr=lr, schurindex=si)
    assert T2.data_ptr() != Tc.data_ptr() and torch.equal(Tc, keep) and torch.equal(T2, Tc)
    Tn, Zn, vn, _ = eng.dgordschur_batch(T1, None, sels, S=S, lr=lr, schurindex=si, wantZ=False)  # copying form, no Z
    assert Zn is None and Tn.data_ptr() != T1.data_ptr() and torch.equal(T1.cpu(), torch.from_numpy(Th))
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgordschur_batch_(T1[:, :, :, :5], None, sels, S=S, lr=lr, schurindex=si, wantZ=False)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgordschur_batch_(T1, None, sels, S=S[:-1], lr=lr, schurindex=si, wantZ=False)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.dgordschur_batch_(T1.to(torch.complex128), None, sels, S=S, lr=lr, schurindex=si, wantZ=False)
    with pytest.raises(ValueError):
        eng.dgordschur_batch_(T1, Z1, sels, S=S, lr=lr, schurindex=2)
    # an empty batch is returned as it is and describes itself like any other call
    infos = [7]
    T0, Z0, v0, st0 = eng.dgordschur_batch_(T1[:0], Z1[:0], sels[:0], S=S, lr=lr, schurindex=si, infos_out=infos)
    assert T0.shape[0] == 0 and v0.shape == (0, n) and infos == [] and st0.nlaunch_step == 0
    assert eng.dgordschur_batch_stats.nsweeps == 0 and len(eng.dgordschur_batch_nswaps) == 0
