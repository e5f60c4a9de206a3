"""Engine.dgeigvecs_batch (psd_d_geigvecs_batch / psd_d_geigvecs_batch_dev, csrc/psd_gbevec.h): geigvecs of many small
signed Float64 periodic Schur forms in one call — the cases shared by the simulated tier
(test_hostsim_dgeigvecs_batch.py) and the device tier (test_gpu_dgeigvecs_batch.py); they mirror zgbevec_cases.py.  Every
gate is the project's own: the relation ratio gevec_cases.relation_ratio <= GATE (1e-11), agreement with the numpy
prototype gevec_cases.prototype at atol 1e-9 and of the scalars a at rtol 1e-13, norm within 1e-13, a real positive phase
entry, the partner column and scalars of a pair the exact conjugates, and a on 1x1 columns exactly the diagonal entries of
T_l.  The inputs are gevec_cases.signed_form(n, p, S, lr, seed, pairs=..., si=1 if lr == "R" else p) with the seeds 5, 7,
9 and the signature S_ALT(p) for p < 4, else S_TFFT(p).  On these inputs, over the shapes of this file, both orientations,
that signature, all-false and all-true, the single geigvecs on the simulated tier reaches a relation ratio of at most
3.0e-14, the prototype at most 1.1e-14, and the two lie at most 6.0e-12 apart.

The batched path, over every case of this file (FIGURES collects them; test_zz_figures prints them last):
  simulated tier: relation ratio at most 3.0e-14, distance to the prototype at most 6.3e-13; a the same bits as the single
    geigvecs at every shape, V the same bits at every shape with n <= 16 (one chunk of the single path: the same sums in
    the same order) and at most 6.3e-15 from it elsewhere;
  MI355X: relation ratio at most 3.0e-14, distance to the prototype at most 1.0e-12, V at most 7.3e-15 from the single
    geigvecs on the device (not gated on bits there: the two kernels are compiled apart; the timing grid of
    profiles/batch/README.md saw equal bits at n = 8 and 16 and at most 4.9e-16 above), a the same bits (the same host
    function).
Both tiers count 15 perturbed pivots on the repeated eigenvalue and 5 rescaled columns on the graded problem, as the
single call does — far inside every gate."""
import ctypes as C

import numpy as np
import pytest

import gevec_cases as gc
import psd_amd
import psdtest as pt
from zgbevec_cases import _lead, _represented, _same, _sarr, sig

GATE = gc.GATE
SEEDS = (5, 7, 9)
FIGURES = {}  # (tier, figure) -> worst value seen
_cache = {}


def _shared(key, make):
    """Inputs are built once, shared among the cases, and never written to."""
    if key not in _cache:
        out = make()
        for P, As in out:
            for a in list(P.Ts) + list(P.Z) + list(As):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def is_sim(eng):
    return "hostsim" in eng.lib._name


def _figure(eng, name, v):
    key = ("sim" if is_sim(eng) else "gpu", name)
    FIGURES[key] = max(FIGURES.get(key, 0.0), float(v))


def dgform(n, p, lr, seed, pairs=(), S=None, diag=None):
    """a signed real problem: (GeneralizedPeriodicSchur, As)"""
    return gc.signed_form(n, p, sig(p) if S is None else S, lr, diag=diag, seed=seed, pairs=pairs,
                          si=1 if lr == "R" else p)


def completed(P, select):
    """select completed to whole pairs"""
    s = np.zeros(P.Ts[0].shape[0], dtype=bool)
    for k, m in gc._columns(P, select):
        s[k:k + m] = True
    return s


def single(eng, P, select):
    """the single call on the same engine: computed once per (engine, problem, selection)"""
    key = ("single", id(eng), id(P), np.asarray(select, dtype=bool).tobytes())
    if key not in _cache:
        Vs, a = eng.geigvecs(P, list(np.asarray(select, dtype=bool)))
        st = eng.eigvecs_stats
        _cache[key] = (Vs, a, (st.nperturbed, st.nrescaled, st.nzero))
    return _cache[key]


def check_problem(eng, P, As, Vs, a, select, proto=True, vs_single=True):
    """the full check of one problem's result; prints the figures before it asserts"""
    S, p, n = gc._sgn(P), len(P.Ts), P.Ts[0].shape[0]
    cols = gc._columns(P, select)
    nvec = sum(m for _, m in cols)
    assert len(Vs) == p and all(V.shape == (n, nvec) for V in Vs) and a.shape == (p, nvec)
    assert all(np.isfinite(V).all() for V in Vs) and np.isfinite(a).all()
    c = 0
    for k, m in cols:
        if m == 1:  # a_l = T_l(k, k), exactly
            assert all(a[l, c] == P.Ts[l][k, k] for l in range(p))
        else:  # the partner and its scalars: the exact conjugates
            assert all(np.array_equal(V[:, c + 1], np.conj(V[:, c])) for V in Vs)
            assert np.array_equal(a[:, c + 1], np.conj(a[:, c]))
        c += m
    r = gc.relation_ratio(As, S, P.orientation, Vs, a) if nvec else 0.0
    print("(p, n) = (%d, %d) %s: relation ratio %.3e" % (p, n, P.orientation, r))
    _figure(eng, "ratio", r)
    assert r <= GATE, r
    V1 = Vs[0]
    assert np.allclose(np.linalg.norm(V1, axis=0), 1.0, atol=1e-13)
    for c in range(V1.shape[1]):
        am = np.argmax(np.abs(V1[:, c]))
        assert V1[am, c].imag == 0 and V1[am, c].real > 0
    if proto and nvec:
        ref, aref = gc.prototype(P, select)
        d = max(np.abs(Vs[l] - ref[l]).max() for l in range(p))
        print("(p, n) = (%d, %d) %s: distance to the prototype %.3e" % (p, n, P.orientation, d))
        _figure(eng, "proto", d)
        assert np.allclose(a, aref, rtol=1e-13, atol=0)
        for l in range(p):
            assert np.allclose(Vs[l], ref[l], rtol=0, atol=1e-9), (l, np.abs(Vs[l] - ref[l]).max())
    if vs_single and nvec:
        Vr, ar, _ = single(eng, P, select)
        d = max(np.abs(Vs[l] - Vr[l]).max() for l in range(p))
        print("(p, n) = (%d, %d) %s: distance to the single call %.3e" % (p, n, P.orientation, d))
        _figure(eng, "single", d)
        assert np.array_equal(a, ar)  # the same host function
        if is_sim(eng) and n <= 16:  # one chunk of the single path: the same sums in the same order
            assert all(np.array_equal(x, y) for x, y in zip(Vs, Vr))


def check_batch(eng, probs, select, proto=True, vs_single=True):
    """run the batch, check every problem; returns the list of (Vs, a)"""
    Ps = [P for P, _ in probs]
    nb, n = len(Ps), Ps[0].Ts[0].shape[0]
    out = eng.dgeigvecs_batch(Ps, select)
    sel = np.broadcast_to(np.asarray(select, dtype=bool), (nb, n))
    assert len(out) == nb
    for q, (P, As) in enumerate(probs):
        check_problem(eng, P, As, out[q][0], out[q][1], sel[q], proto, vs_single)
    return out


def raw_host(eng, Ps, select, shifted=True, maxvec=None):
    """psd_d_geigvecs_batch through the C ABI: (info, V [nb][nmat][maxvec][n] complex, a [nb][maxvec][p] complex, nvec,
    counts, stats, the completed select)."""
    nb, p, n = len(Ps), len(Ps[0].Ts), Ps[0].Ts[0].shape[0]
    Ts = [np.asfortranarray(t, dtype=np.float64) for P in Ps for t in P.Ts]
    Zs = [np.asfortranarray(z, dtype=np.float64) for P in Ps for z in P.Z]
    sel = np.ascontiguousarray(np.broadcast_to(np.asarray(select, dtype=bool), (nb, n)), dtype=np.uint8)
    dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    nvec = (C.c_int * nb)()
    cnts = np.zeros((nb, 3), dtype=np.int32)
    st = psd_amd.BevecStats()
    info = C.c_int(0)
    head = [eng.ctx, nb, n, p, eng._ptrs(Ts), eng._ptrs(Zs), _sarr(Ps[0]), Ps[0].orientation.encode(), Ps[0].schurindex,
            sel.ctypes.data_as(u8p), int(shifted)]
    tail = [nvec, cnts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st), C.byref(info)]
    eng.lib.psd_d_geigvecs_batch(*head, None, 0, None, *tail)  # the size query: select completed, nvec filled
    assert info.value == 0 and st.nlaunch == 0
    if maxvec is None:
        maxvec = max(nvec)
    nmat = p if shifted else 1
    V = np.full((nb, nmat, maxvec, n), 7.0 + 7.0j)  # (poisoned: the padding has to be written)
    a = np.full((nb, maxvec, p), 7.0 + 7.0j)
    Vp = (C.c_void_p * (nb * nmat))(*[V[q, l].ctypes.data for q in range(nb) for l in range(nmat)])
    rc = eng.lib.psd_d_geigvecs_batch(*head, Vp, maxvec, a.ctypes.data_as(dp), *tail)
    assert rc == info.value
    return info.value, V, a, list(nvec), cnts, st, sel.astype(bool)


# ------------------------------------------------------------------------------------------------
# 1. mixed batch: rows 0 | (1, 2) | 3 | (4, 5) | 6
MIXED_PAIRS = (1, 4)
MIXED_SELECT = np.array([[1, 1, 1, 1, 1, 1, 1],   # all
                         [0, 0, 1, 0, 0, 0, 0],   # the second member of a pair only
                         [0, 0, 0, 0, 0, 0, 0],   # none
                         [1, 0, 0, 1, 0, 1, 0],   # 1x1 rows and a second member
                         [0, 1, 0, 0, 0, 0, 1]], dtype=bool)
MIXED_NVEC = [7, 2, 0, 4, 3]


def mixed_problems():
    return _shared("mixed", lambda: [dgform(7, 3, "L", SEEDS[q % 3] + 10 * (q // 3), MIXED_PAIRS) for q in range(5)])


def case_mixed(eng):
    probs = mixed_problems()
    Ps = [P for P, _ in probs]
    keep = [[x.copy() for x in list(P.Ts) + list(P.Z)] for P in Ps]
    out = check_batch(eng, probs, MIXED_SELECT)
    assert [r[0][0].shape[1] for r in out] == MIXED_NVEC
    one = eng.dgeigvecs_batch(Ps, MIXED_SELECT, shifted=False)
    for q in range(5):
        assert len(one[q][0]) == 1 and np.array_equal(one[q][0][0], out[q][0][0])  # bit-identical
        assert np.array_equal(one[q][1], out[q][1])
    assert all(np.array_equal(x, y) for P, k in zip(Ps, keep) for x, y in zip(list(P.Ts) + list(P.Z), k))
    # the blocks as the ABI leaves them: n x maxvec, the columns at and beyond nvec exactly zero, in V and in a
    info, V, a, nvec, cnts, st, sel = raw_host(eng, Ps, MIXED_SELECT)
    assert info == 0 and nvec == MIXED_NVEC and V.shape[2] == 7
    for q in range(5):
        assert np.array_equal(sel[q], completed(Ps[q], MIXED_SELECT[q]))
        for l in range(3):
            assert np.array_equal(V[q, l, :nvec[q]].T, out[q][0][l])
            assert np.all(V[q, l, nvec[q]:] == 0)
        assert np.array_equal(a[q, :nvec[q]].T, out[q][1]) and np.all(a[q, nvec[q]:] == 0)
    assert st.nb == 5 and st.nvec_total == sum(MIXED_NVEC) and st.ngroups == 1 and st.nlaunch == 4
    assert st.nperturbed == 0 and st.nrescaled == 0 and st.nzero == 0 and not cnts.any()


# ------------------------------------------------------------------------------------------------
# 2. batch independence, bit for bit
def independence_problems():
    base = _shared("indep", lambda: [dgform(6, 2, "R", SEEDS[k % 3] + 10 * (k // 3), (0, 3)) for k in range(5)])
    return [base[q % 5] for q in range(70)]  # (70 crosses any grouping of 32 or 64 units or problems)


def case_independence(eng, eng_groups=None):
    """the whole batch, a problem alone (first, middle, last), the batch reversed, and under PSD_BATCH_GROUP=3: the same
    bits"""
    probs = independence_problems()
    Ps = [P for P, _ in probs]
    select = np.ones(6, dtype=bool)
    whole = eng.dgeigvecs_batch(Ps, select)
    for q in range(5):
        check_problem(eng, Ps[q], probs[q][1], whole[q][0], whole[q][1], select)
    for q in range(70):  # the same problem at another place
        assert _same(whole[q], whole[q % 5]), q
    for pos in (0, 33, 69):
        alone = eng.dgeigvecs_batch([Ps[pos]], select)
        assert _same(alone[0], whole[pos]), pos
    turned = eng.dgeigvecs_batch(Ps[::-1], select)
    assert all(_same(turned[69 - q], whole[q]) for q in range(70))
    if eng_groups is not None:
        parts = eng_groups.dgeigvecs_batch(Ps, select)
        assert eng_groups.eigvecs_batch_stats.ngroups == 24
        assert all(_same(x, y) for x, y in zip(whole, parts))


# ------------------------------------------------------------------------------------------------
# 3. lane layouts and block widths: (p, n, pair rows)
LAYOUTS = [(2, 6, (0, 3)),           # of the mixed shapes
           (1, 5, (2,)),             # p = 1
           (3, 2, (0,)),             # n = 2: the problem is one own 2x2 block
           (3, 1, ()),               # n = 1
           (70, 5, (1,)),            # lanes own two factors, r in the global buffer
           (5, 9, (0, 4, 7)),        # idle lanes in a sub-group of 8; pairs at the top row and at the bottom rows
           (32, 4, (0, 2)),          # one sub-group per half-wave; every row in a pair
           (4, 12, (1, 5, 9)),       # sixteen units per wavefront on blocks of width 1 and 2 in the same step
           (2, 17, (15,)),           # pairs where the single path splits chunks
           (3, 33, (15, 31))]


def layout_id(s):
    return "p%d-n%d" % s[:2]


def case_layout(eng, shape, lr):
    """every row selected; a signature with both senses wherever p > 1"""
    p, n, pairs = shape
    assert p == 1 or len(set(sig(p))) == 2
    probs = _shared(("layout", shape, lr), lambda: [dgform(n, p, lr, s, pairs) for s in SEEDS])
    out = check_batch(eng, probs, np.ones(n, dtype=bool))
    assert all(r[0][0].shape[1] == n for r in out)


def case_all_false(eng, lr):
    """every factor inverted (the quasi-triangular one too)"""
    p, n = 5, 9
    probs = _shared(("allfalse", lr), lambda: [dgform(n, p, lr, s, (0, 4, 7), S=[False] * p) for s in SEEDS])
    check_batch(eng, probs, np.ones(n, dtype=bool))


# ------------------------------------------------------------------------------------------------
# 4. depth and cap
DEPTH_PAIRS = (3, 16, 30, 38)


def depth_problems(lr):
    return _shared(("depth", lr), lambda: [dgform(40, 3, lr, s, DEPTH_PAIRS) for s in SEEDS])


def case_depth(eng, lr):
    n = 40
    select = (np.arange(n) % 7 == 0) | np.isin(np.arange(n), [17, 38])  # 1x1 columns through every pair, two own pairs
    check_batch(eng, depth_problems(lr), select)


def case_cap(eng, n, lr):
    """n = 128: the largest order of the batched kernel; n = 129: the per-problem fallback.  The same gates."""
    pairs = (10, 63, n - 2)
    probs = _shared(("cap", n, lr), lambda: [dgform(n, 2, lr, s, pairs) for s in SEEDS[:2]])
    select = np.zeros(n, dtype=bool)
    select[[0, 11, 63, n - 1]] = True
    check_batch(eng, probs, select)
    assert eng.eigvecs_batch_stats.nvec_total == 14
    assert (eng.eigvecs_batch_stats.nlaunch == 4) == (n <= 128)


# ------------------------------------------------------------------------------------------------
# 5. zero and infinite eigenvalues
def case_zero_infinite(eng, lr):
    """zero diagonal entries on 1x1 rows of a forward and of an inverted factor, a pair above and below them"""
    n, p = 7, 4
    S = [True, False, True, False]
    pairs = (0, 5)
    rs = np.random.RandomState(53)
    diag = [1.0 + rs.rand(n) for _ in range(p)]
    diag[0][2] = 0.0  # zero eigenvalue at row 2
    diag[1][4] = 0.0  # infinite eigenvalue at row 4
    probs = _shared(("zeroinf", lr), lambda: [dgform(n, p, lr, 5, pairs, S=S), dgform(n, p, lr, 7, pairs, S=S, diag=diag),
                                              dgform(n, p, lr, 9, pairs, S=S)])
    select = np.ones(n, dtype=bool)
    out = eng.dgeigvecs_batch([P for P, _ in probs], select)
    cnt = eng.eigvecs_batch_counts.copy()
    nzero = eng.eigvecs_batch_stats.nzero
    assert cnt.tolist() == [[0, 0, 0], [0, 0, 2], [0, 0, 0]] and nzero == 2
    assert single(eng, probs[1][0], select)[2][2] == 2
    for q in range(3):  # (the prototype is not used on the singular problem, as in gevec_cases.case_zero_infinite)
        check_problem(eng, probs[q][0], probs[q][1], out[q][0], out[q][1], select, proto=q != 1)
    Vs, a = out[1]
    As = probs[1][1]
    left = lr == "L"
    v_zero = Vs[0][:, 2] if left else Vs[1][:, 2]  # A_1 v_1 = 0 ('L'), A_1 v_2 = 0 ('R')
    assert np.linalg.norm(As[0] @ v_zero) <= GATE * np.linalg.norm(As[0]) * np.linalg.norm(v_zero)
    v_inf = Vs[2][:, 4] if left else Vs[1][:, 4]  # A_2 v_3 = 0 ('L'), A_2 v_2 = 0 ('R')
    assert np.linalg.norm(As[1] @ v_inf) <= GATE * np.linalg.norm(As[1]) * np.linalg.norm(v_inf)
    assert a[0, 2] == 0 and a[1, 4] == 0


# ------------------------------------------------------------------------------------------------
# 6. repeated eigenvalue
def case_repeated(eng):
    n, p = 6, 4
    probs = _shared("rep", lambda: [dgform(n, p, "L", 7, diag=[np.full(n, 1.5) for _ in range(p)]),
                                    dgform(n, p, "L", 9, (1, 4))])
    select = np.ones(n, dtype=bool)
    out = eng.dgeigvecs_batch([P for P, _ in probs], select)
    cnt = eng.eigvecs_batch_counts.copy()
    nperturbed = eng.eigvecs_batch_stats.nperturbed
    assert all(np.isfinite(V).all() for V in out[0][0]) and out[0][0][0].shape[1] == n
    print("repeated eigenvalue: perturbed pivots", cnt[0, 0])
    assert cnt[0, 0] > 0 and cnt[0, 1] == 0 and cnt[0, 2] == 0 and not cnt[1].any()
    assert nperturbed == cnt[0, 0]
    assert cnt[0, 0] == single(eng, probs[0][0], select)[2][0]  # counted as by the single call
    check_problem(eng, probs[1][0], probs[1][1], out[1][0], out[1][1], select)


# ------------------------------------------------------------------------------------------------
# 7. rescaled columns
def case_rescale(eng, lr):
    """the graded diagonals of gevec_cases.case_rescale (2^+-175 inside the period, each row's signed product moderate).
    Gated on the relations alone: the prototype's SVD null vector fails on this grading."""
    n, p = 8, 6
    S = gc.S_ALT(p)
    diag = []
    for l in range(p):
        g = np.where(np.arange(n) % 2 == 1, 2.0 ** (175 if l < 3 else -175), 1.0)
        d = np.linspace(1.0, 1.7, n) ** (1.0 / p) * g
        diag.append(d if S[l] else 1.0 / d)
    probs = _shared(("resc", lr), lambda: [dgform(n, p, lr, 5, (2,), S=S), dgform(n, p, lr, 23, S=S, diag=diag)])
    select = np.ones(n, dtype=bool)
    out = eng.dgeigvecs_batch([P for P, _ in probs], select)
    cnt = eng.eigvecs_batch_counts.copy()
    nrescaled = eng.eigvecs_batch_stats.nrescaled
    print("rescaled columns:", cnt[:, 1].tolist())
    assert cnt[1, 1] > 0 and cnt[0, 1] == 0 and nrescaled == cnt[1, 1]
    assert cnt[1, 1] == single(eng, probs[1][0], select)[2][1]  # equal to the single call's
    check_problem(eng, probs[1][0], probs[1][1], out[1][0], out[1][1], select, proto=False)
    check_problem(eng, probs[0][0], probs[0][1], out[0][0], out[0][1], select)


# ------------------------------------------------------------------------------------------------
# 8. all-true signature
def case_all_true(eng):
    """an all-true signature runs this path too; a PeriodicSchur and a GeneralizedPeriodicSchur with S all true give the
    same bits"""
    n, p = 7, 3
    probs = _shared("alltrue", lambda: [dgform(n, p, "L", s, MIXED_PAIRS, S=[True] * p) for s in SEEDS])
    select = np.ones(n, dtype=bool)
    out = check_batch(eng, probs, select)
    assert eng.eigvecs_batch_stats.nlaunch == 4
    pss = [psd_amd.PeriodicSchur(P.Ts, P.Z, np.array(P.values), P.orientation, P.schurindex) for P, _ in probs]
    outp = eng.dgeigvecs_batch(pss, select)
    assert all(_same(x, y) for x, y in zip(out, outp))


# ------------------------------------------------------------------------------------------------
# 9. skipped problems
def case_skipped(eng):
    probs = mixed_problems()[:4]
    Ps = [P for P, _ in probs]
    full = eng.dgeigvecs_batch(Ps, np.ones(7, dtype=bool))
    select = np.ones((4, 7), dtype=bool)
    select[1] = select[3] = False
    out = eng.dgeigvecs_batch(Ps, select)
    for q in (1, 3):
        assert all(V.shape == (7, 0) for V in out[q][0]) and out[q][1].shape == (3, 0)
    for q in (0, 2):
        assert _same(out[q], full[q])
    info, V, a, nvec, cnts, st, _ = raw_host(eng, Ps, select)
    assert info == 0 and nvec == [7, 0, 7, 0] and st.nvec_total == 14
    for q in (1, 3):
        assert np.all(V[q] == 0) and np.all(a[q] == 0)
    # nothing selected anywhere: nothing is launched
    none = eng.dgeigvecs_batch(Ps, np.zeros(7, dtype=bool))
    assert all(V.shape == (7, 0) for r in none for V in r[0])
    assert eng.eigvecs_batch_stats.nlaunch == 0 and eng.eigvecs_batch_stats.nvec_total == 0
    info, V, a, nvec, cnts, st, _ = raw_host(eng, Ps, np.zeros(7, dtype=bool), maxvec=2)
    assert info == 0 and nvec == [0, 0, 0, 0] and st.nlaunch == 0 and np.all(V == 0) and np.all(a == 0)


# ------------------------------------------------------------------------------------------------
# 10. launch count
def case_launch_count(eng):
    """the launches of a call depend neither on nb nor on n (below the cap): solve, V_1, norms, the other factors — four
    with shifted and p > 1, three otherwise, none when nothing is selected (the header of psd_gbevec_host.inl)"""
    small = _shared("launch4", lambda: [dgform(4, 3, "L", SEEDS[k], (1,)) for k in range(3)])
    deep = depth_problems("L")
    counts = {}
    for key, Ps in (("nb1", [small[0][0]]), ("nb70", [small[q % 3][0] for q in range(70)]), ("n40", [P for P, _ in deep])):
        eng.dgeigvecs_batch(Ps, np.ones(Ps[0].Ts[0].shape[0], dtype=bool))
        counts[key] = eng.eigvecs_batch_stats.nlaunch
        assert eng.eigvecs_batch_stats.ngroups == 1
    assert counts["nb1"] == counts["nb70"] == counts["n40"] == 4, counts
    eng.dgeigvecs_batch([P for P, _ in small], np.ones(4, dtype=bool), shifted=False)
    assert eng.eigvecs_batch_stats.nlaunch == 3
    one = _shared("launchp1", lambda: [dgform(5, 1, "L", 5, (2,))])
    eng.dgeigvecs_batch([one[0][0]], np.ones(5, dtype=bool))
    assert eng.eigvecs_batch_stats.nlaunch == 3  # p = 1: no other factors
    eng.dgeigvecs_batch([P for P, _ in small], np.zeros(4, dtype=bool))
    assert eng.eigvecs_batch_stats.nlaunch == 0


# ------------------------------------------------------------------------------------------------
# 11. pipeline
def _pipeline_inputs(n, p, nb):
    return [pt.bench_factors(n, p, seed=191 + q) for q in range(nb)]


def case_pipeline_host(eng, lr):
    """dgpschur_batch -> dgordschur_batch_ (|lambda| < 1 first) -> dgeigvecs_batch on the leading rows, host forms"""
    n, p, nb = 8, 3, 6
    S = [True, False, True]
    pss = eng.dgpschur_batch(_pipeline_inputs(n, p, nb), S, lr)
    sels = [_lead(ps.values) for ps in pss]
    eng.dgordschur_batch_(pss, np.array([s[0] for s in sels]))
    lead = np.array([s[1] for s in sels])
    out = eng.dgeigvecs_batch(pss, lead)
    for q, ps in enumerate(pss):
        assert ps.S == S and out[q][0][0].shape == (n, lead[q].sum())
        assert not np.iscomplexobj(ps.Ts[0]) and not np.iscomplexobj(ps.Z[0])
        check_problem(eng, ps, _represented(S, lr, ps.Ts, ps.Z), out[q][0], out[q][1], lead[q], proto=False, vs_single=False)


def case_pipeline(eng, lr):
    """the same, device-resident: no matrix touches the host between the three calls"""
    import torch

    n, p, nb = 8, 3, 6
    S = [True, False, True]
    si = p if lr == "L" else 1
    dA = torch.from_numpy(np.array([[np.array(x) for x in A] for A in _pipeline_inputs(n, p, nb)])).cuda()
    T, Z, values, _ = eng.dgpschur_batch_(dA, S, lr)
    sels = [_lead(v) for v in values]
    T, Z, values, _ = eng.dgordschur_batch_(T, Z, np.array([s[0] for s in sels]), S=S, lr=lr, schurindex=si)
    lead = np.array([s[1] for s in sels])
    V, a, nvec = eng.dgeigvecs_batch(T, Z, lead, S=S, lr=lr, schurindex=si)
    assert eng.eigvecs_batch_stats.nlaunch == 5  # (the gather of the device entry, then four)
    mv = int(lead.sum(axis=1).max())
    assert nvec.tolist() == lead.sum(axis=1).tolist() and nvec.dtype == np.int32
    assert V.is_cuda and V.dtype == torch.complex128 and tuple(V.shape) == (nb, p, n, mv)
    assert a.shape == (nb, p, mv) and a.dtype == np.complex128
    Vh, Th, Zh = V.cpu().numpy(), T.cpu().numpy(), Z.cpu().numpy()
    for q in range(nb):
        assert np.all(Vh[q][:, :, nvec[q]:] == 0) and np.all(a[q][:, nvec[q]:] == 0)
        P = psd_amd.GeneralizedPeriodicSchur(S, [np.asfortranarray(Th[q, l]) for l in range(p)],
                                             [np.asfortranarray(Zh[q, l]) for l in range(p)], values[q], np.ones(n),
                                             np.zeros(n, dtype=np.int32), lr, si)
        check_problem(eng, P, _represented(S, lr, P.Ts, P.Z), [Vh[q, l][:, :nvec[q]] for l in range(p)], a[q][:, :nvec[q]],
                      lead[q], proto=False, vs_single=False)
    V1, a1, nvec1 = eng.dgeigvecs_batch(T, Z, lead, S=S, lr=lr, schurindex=si, shifted=False)
    assert tuple(V1.shape) == (nb, 1, n, mv) and torch.equal(V1[:, 0], V[:, 0]) and np.array_equal(a1, a)
    assert nvec1.tolist() == nvec.tolist()
    with pytest.raises(TypeError, match="zgeigvecs_batch"):
        eng.dgeigvecs_batch(T.to(torch.complex128), Z.to(torch.complex128), lead, S=S, lr=lr, schurindex=si)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgeigvecs_batch(T, Z, lead, S=S[:-1], lr=lr, schurindex=si)
    with pytest.raises(ValueError):
        eng.dgeigvecs_batch(T, None, lead, S=S, lr=lr, schurindex=si)
    with pytest.raises(ValueError, match="argument 9"):
        eng.dgeigvecs_batch(T, Z, lead[:, :-1], S=S, lr=lr, schurindex=si)


# ------------------------------------------------------------------------------------------------
# 12. gpschur_batch(..., real=True) end to end
def case_gpschur_batch(eng):
    """four real pencils (A, B) of order 6: the deflating vectors of each, against the factors its decomposition
    represents"""
    n = 6
    As = [pt.bench_factors(n, 1, seed=300 + 17 * q) for q in range(4)]
    Bs = [pt.bench_factors(n, 1, seed=5300 + 17 * q) for q in range(4)]
    pss = eng.gpschur_batch(As, Bs, real=True)
    select = np.ones(n, dtype=bool)
    out = eng.dgeigvecs_batch(pss, select)
    for q, ps in enumerate(pss):
        assert ps.period == 2 and not all(ps.S) and not np.iscomplexobj(ps.Ts[0])
        check_problem(eng, ps, _represented(ps.S, ps.orientation, ps.Ts, ps.Z), out[q][0], out[q][1], select, proto=False,
                      vs_single=False)


# ------------------------------------------------------------------------------------------------
# 13. errors, and both entries through the C ABI
def case_errors(eng, make_engine):
    probs = mixed_problems()
    Ps = [P for P, _ in probs]
    n, p = 7, 3

    def variant(P, S=None, Z=None, si=None):
        return psd_amd.GeneralizedPeriodicSchur(P.S if S is None else S, P.Ts, P.Z if Z is None else Z, P.alpha, P.beta,
                                                P.alphascale, P.orientation, P.schurindex if si is None else si)

    with pytest.raises(ValueError, match="argument 9"):
        eng.dgeigvecs_batch(Ps, [True] * (n - 1))
    with pytest.raises(ValueError, match="argument 9"):
        eng.dgeigvecs_batch(Ps, np.ones((4, n), dtype=bool))
    with pytest.raises(psd_amd.DimensionMismatch, match="signatures"):
        eng.dgeigvecs_batch([Ps[0], variant(Ps[1], S=[True, True, False])], [True] * n)  # unequal S
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgeigvecs_batch([variant(Ps[0], S=[True, False])] * 2, [True] * n)  # S length
    with pytest.raises(ValueError, match="argument 8"):
        eng.dgeigvecs_batch([variant(Ps[0], si=p + 1)] * 2, [True] * n)  # schurindex outside the period
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgeigvecs_batch([Ps[0], variant(Ps[1], si=1)], [True] * n)  # unequal schurindex
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.dgeigvecs_batch([Ps[0], dgform(6, p, "L", 5)[0]], [True] * n)  # unequal order
    with pytest.raises(ValueError):
        eng.dgeigvecs_batch([variant(Ps[0], Z=[])], [True] * n)  # no Schur vectors
    cplx = gc.signed_form(n, p, [True, False, True], "L", seed=3, cplx=True)[0]
    with pytest.raises(TypeError, match="zgeigvecs_batch"):
        eng.dgeigvecs_batch([cplx], [True] * n)  # ComplexF64
    with pytest.raises(TypeError):
        eng.dgeigvecs_batch(Ps, [True] * n, [True] * n)
    with pytest.raises(TypeError, match="use geigvecs per problem for a Float64 decomposition"):
        eng.zgeigvecs_batch(Ps, [True] * n)  # (the complex entry's message stays)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.eigvecs_batch(Ps, [True] * n)  # the unsigned entry still refuses a signed decomposition
    assert eng.dgeigvecs_batch([], [True] * n) == []
    assert eng.eigvecs_batch_stats.nb == 0 and eng.eigvecs_batch_counts.shape == (0, 3)
    info, V, a, nvec, _, _, _ = raw_host(eng, Ps, MIXED_SELECT, maxvec=6)  # problem 0 has 7 columns
    assert info == -10 and nvec == MIXED_NVEC
    sharded = make_engine()
    sharded.set_shard(0, 2)
    with pytest.raises(psd_amd.NotImplementedPSD):
        sharded.dgeigvecs_batch(Ps, [True] * n)


def case_dev_abi(eng):
    """psd_d_geigvecs_batch_dev through the C ABI on packed blocks (in the simulation device memory is host memory): the
    same bits as the host entry, one launch more (the gather), and the argument codes of both entries."""
    probs = mixed_problems()
    Ps = [P for P, _ in probs]
    nb, n, p = 5, 7, 3
    host = eng.dgeigvecs_batch(Ps, MIXED_SELECT)
    dT = np.ascontiguousarray(np.array([pt.pack(P.Ts) for P in Ps]))
    dZ = np.ascontiguousarray(np.array([pt.pack(P.Z) for P in Ps]))
    sel = np.ascontiguousarray(MIXED_SELECT, dtype=np.uint8)
    done = np.array([completed(P, s) for P, s in zip(Ps, MIXED_SELECT)], dtype=np.uint8)
    dp, u8p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    nvec = (C.c_int * nb)()
    cnts = np.zeros((nb, 3), dtype=np.int32)
    st = psd_amd.BevecStats()
    info = C.c_int(0)
    lib, ctx, Sp, selp = eng.lib, eng.ctx, _sarr(Ps[0]), sel.ctypes.data_as(u8p)
    bT, bZ = C.c_void_p(dT.ctypes.data), C.c_void_p(dZ.ctypes.data)
    tail = [nvec, cnts.ctypes.data_as(i32p), C.byref(st), C.byref(info)]
    rc = lib.psd_d_geigvecs_batch_dev(ctx, nb, n, p, bT, bZ, Sp, b"L", p, selp, 1, None, 0, None, *tail)
    assert rc == 0 and list(nvec) == MIXED_NVEC and st.nlaunch == 1  # the size query: the gather alone
    assert np.array_equal(sel, done)  # select completed in place
    V = np.full((nb, p, 7, n), 7.0 + 7.0j)
    a = np.full((nb, 7, p), 7.0 + 7.0j)
    rc = lib.psd_d_geigvecs_batch_dev(ctx, nb, n, p, bT, bZ, Sp, b"L", p, selp, 1, C.c_void_p(V.ctypes.data), 7,
                                      a.ctypes.data_as(dp), *tail)
    assert rc == 0 and info.value == 0 and st.nb == nb and st.ngroups == 1 and st.nlaunch == 5
    assert st.ms_kernels >= st.ms_solve >= 0
    for q in range(nb):
        for l in range(p):
            assert np.array_equal(V[q, l, :nvec[q]].T, host[q][0][l]) and np.all(V[q, l, nvec[q]:] == 0)
        assert np.array_equal(a[q, :nvec[q]].T, host[q][1]) and np.all(a[q, nvec[q]:] == 0)
    V2 = np.full((nb, p, 7, n), 7.0 + 7.0j)  # without the scalars, shifted = 0: the gather, then three
    rc = lib.psd_d_geigvecs_batch_dev(ctx, nb, n, p, bT, bZ, None, b"L", p, selp, 0, C.c_void_p(V2.ctypes.data), 7, None,
                                      *tail)
    assert rc == 0 and st.nlaunch == 4  # (S = NULL: all true, another problem; the launches are what is looked at)
    sel0 = np.zeros((nb, n), dtype=np.uint8)  # nothing selected: no launch, the gather included
    rc = lib.psd_d_geigvecs_batch_dev(ctx, nb, n, p, bT, bZ, Sp, b"L", p, sel0.ctypes.data_as(u8p), 1,
                                      C.c_void_p(V2.ctypes.data), 7, a.ctypes.data_as(dp), *tail)
    assert rc == 0 and st.nlaunch == 0 and not any(nvec) and np.all(V2 == 0) and np.all(a == 0)
    for q in range(nb):  # the inputs stay as they were
        assert np.array_equal(dT[q], pt.pack(Ps[q].Ts)) and np.array_equal(dZ[q], pt.pack(Ps[q].Z))

    def dev_(c_=ctx, nb_=nb, n_=n, p_=p, T_=bT, Z_=bZ, o=b"L", si=p, sel_=selp, V_=None, mv=0, nv=nvec):
        return lib.psd_d_geigvecs_batch_dev(c_, nb_, n_, p_, T_, Z_, Sp, o, si, sel_, 1, V_, mv, None, nv, None, None, None)

    Tp = eng._ptrs([np.asfortranarray(t, dtype=np.float64) for P in Ps for t in P.Ts])
    Zp = eng._ptrs([np.asfortranarray(z, dtype=np.float64) for P in Ps for z in P.Z])

    def host_(c_=ctx, nb_=nb, n_=n, p_=p, T_=Tp, Z_=Zp, o=b"L", si=p, sel_=selp, V_=None, mv=0, nv=nvec):
        return lib.psd_d_geigvecs_batch(c_, nb_, n_, p_, T_, Z_, Sp, o, si, sel_, 1, V_, mv, None, nv, None, None, None)

    for f in (dev_, host_):
        assert f() == 0
        assert f(c_=None) == -1 and f(n_=0) == -2 and f(p_=0) == -3 and f(T_=None) == -4 and f(Z_=None) == -5
        assert f(o=b"X") == -7 and f(si=0) == -8 and f(si=p + 1) == -8
        assert f(sel_=None) == -9 and f(nb_=-1) == -11 and f(nv=None) == -12
        assert f(nb_=0, T_=None, Z_=None, sel_=None, nv=None) == 0  # nb == 0 touches nothing
    assert dev_(V_=C.c_void_p(V.ctypes.data), mv=6) == -10
    Vp = (C.c_void_p * (nb * p))(*[V[q, l].ctypes.data for q in range(nb) for l in range(p)])
    assert host_(V_=Vp, mv=6) == -10
    # a period-sharded context keeps a slice of Z: both entries refuse it
    sharded = psd_amd.Engine(libpath=eng.lib._name)
    sharded.set_shard(0, 2)
    assert dev_(c_=sharded.ctx) == psd_amd.INFO_NOTIMPL and host_(c_=sharded.ctx) == psd_amd.INFO_NOTIMPL


def print_figures():
    for key in sorted(FIGURES):
        print("dgeigvecs_batch worst %s %s: %.3e" % (key[0], key[1], FIGURES[key]))
