"""Engine.zordschur_batch_ / zordschur_batch (psd_z_ordschur_batch / psd_z_ordschur_batch_dev, csrc/psd_zbord.h): many small
ComplexF64 periodic Schur forms reordered in one call — the cases shared by the simulated tier
(test_hostsim_zordschur_batch.py) and the device tier (test_gpu_zordschur_batch.py).  Inputs are zpschur_batch results of
pt.bench_factors(..., dtype=complex128) with the eigenvalues at or below the median modulus selected; the checks and bounds
of engine_cases.case_zordschur_windows are applied to every problem of a batch.  pt.oracle_ordschur accepts every swap of
every one of them (asserted where the oracle runs)."""
import ctypes as C

import numpy as np
import pytest

import psd_amd
import psdtest as pt
from batch_common import shape_id
from engine_cases import _clone
from ord_batch_cases import median_select

# (nb, n, p) and what each covers
WINDOW_SHAPES = [
    (3, 48, 3),   # W = 32 < n: several windows, all three off-window roles
    (2, 40, 22),  # W = 20
    (2, 30, 70),  # W = 10, window image near the LDS limit
    (33, 12, 3),  # more problems than a 32-wide chunk, n < W
    (3, 5, 1),    # p = 1: the p == 1 branch of the swap, where H_{m-1} is H_m
    (4, 2, 2),    # smallest window; row 2 alone is selected (the median rule selects both rows)
    (3, 1, 3),    # n = 1: no swap
]
NARROW_SHAPE = (3, 20, 3)  # with PSD_BORD_W=6: several narrow windows
GROUP_SHAPE = (6, 20, 3)   # the group loop under PSD_BATCH_GROUP=4
CAP_SHAPE = (2, 20, 3)
CHAIN_SHAPE = (5, 12, 3)

_cache = {}


def factors(shape):
    """The factors of a shape: built once, shared, never written to."""
    nb, n, p = shape
    key = ("A", shape)
    if key not in _cache:
        probs = [pt.bench_factors(n, p, seed=9500 + 131 * q + 7 * n + p, dtype=np.complex128) for q in range(nb)]
        for A in probs:
            for a in A:
                a.setflags(write=False)
        _cache[key] = probs
    return _cache[key]


def select_for(shape, lam):
    if shape[1] == 2:  # (the median rule selects both rows of an order-2 problem: nothing would move)
        return np.array([False, True])
    return median_select(lam)


def inputs(eng, shape, lr):
    """(factors, decompositions, selections) of a shape and orientation: computed once per library (the engines of a tier
    differ in the knobs of the reordering only) and only cloned."""
    key = (eng.lib._name, shape, lr)
    if key not in _cache:
        probs = factors(shape)
        ps0 = eng.zpschur_batch(probs, lr)
        sels = np.array([select_for(shape, ps.values) for ps in ps0])
        _cache[key] = (probs, ps0, sels)
    return _cache[key]


def single(eng, shape, lr, q):
    """ordschur_ of problem q on `eng` (the serial or the default single driver): computed once, never written to."""
    key = ("single", id(eng), shape, lr, q)
    if key not in _cache:
        probs, ps0, sels = inputs(eng, shape, lr)
        _cache[key] = (eng.ordschur_(_clone(ps0[q]), sels[q]), eng)
    return _cache[key][0]


def check_problem(A, ps0, ps1, select, oracle=True, nswaps=None):
    """The checks of engine_cases.case_zordschur_windows with its bounds, for one problem; returns the swap count."""
    n = A[0].shape[0]
    lam0 = ps0.values
    ok, err = pt.checkpsd(ps1, A, thresh=100 * np.sqrt(max(n / 32, 1)))  # (strict: zero strict lower triangles)
    assert ok, err
    m = int(select.sum())
    sc = abs(lam0).max()
    assert pt.match_eigs(lam0[select], ps1.values[:m]) < 1e-9 * sc
    assert pt.match_eigs(lam0[~select], ps1.values[m:]) < 1e-9 * sc
    # the order inside the selected / unselected groups is preserved (stable bubbling)
    assert np.allclose(ps1.values[:m], lam0[select], rtol=1e-7, atol=1e-9 * sc)
    assert np.allclose(ps1.values[m:], lam0[~select], rtol=1e-7, atol=1e-9 * sc)
    if oracle:
        po = pt.oracle_ordschur(pt.PSD(ps0.Ts, ps0.Z, lam0, ps0.orientation, ps0.schurindex), select)
        assert po.info == 0 and ps1.stats.nsweeps == po.nswaps, (ps1.stats.nsweeps, po.nswaps)
    if nswaps is not None:
        assert ps1.stats.nsweeps == nswaps
    return ps1.stats.nsweeps


# ------------------------------------------------------------------------------------------------
# 1. reference shape
def case_reference(eng, lr):
    """engine_cases.case_zordschur_reference per problem of a batch: (nb, n, p) = (4, 7, 3), spectrum 4^j."""
    nb, n, p, nsel = 4, 7, 3, 2
    probs = []
    for q in range(nb):
        A = pt.ord_test_factors(n, p, seed=4000 + p + 37 * q, dtype=np.complex128)
        probs.append(A[::-1] if lr == "R" else A)
    ps0 = eng.zpschur_batch(probs, lr)
    for ps in ps0:
        assert np.allclose(np.sort(np.abs(ps.values)), [4.0 ** (j + 1) for j in range(n)], rtol=1e-8)
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
        out = eng.zordschur_batch_([_clone(ps) for ps in ps0], np.array(sels))
        assert eng.zordschur_batch_stats.nlaunch_step == 1
        for q in range(nb):
            pt.pschur_check(probs[q], out[q], check_lam=False, real=False)
            for j in range(nsel):
                assert np.any(np.isclose(out[q].values[:nsel], ps0[q].values[idxs[q][j]], rtol=1e-8))
            po = pt.oracle_ordschur(pt.PSD(ps0[q].Ts, ps0[q].Z, ps0[q].values, lr, ps0[q].schurindex), sels[q])
            assert out[q].stats.nsweeps == po.nswaps
            assert np.allclose(out[q].values, po.values, rtol=1e-10, atol=0)


# ------------------------------------------------------------------------------------------------
# 2. windows
def case_windows(eng, shape, lr, expect_window=None):
    nb, n, p = shape
    probs, ps0, sels = inputs(eng, shape, lr)
    out = eng.zordschur_batch_([_clone(ps) for ps in ps0], sels)
    st = eng.zordschur_batch_stats
    assert len(out) == nb and st.nlaunch_step == 1 and st.nsweeps == sum(ps.stats.nsweeps for ps in out)
    assert list(eng.zordschur_batch_nswaps) == [ps.stats.nsweeps for ps in out]
    if expect_window is not None:
        assert st.window == expect_window and st.nwindows > nb  # (several windows per problem)
    noz = eng.zordschur_batch_([_clone(ps) for ps in ps0], sels, wantZ=False)
    for q in range(nb):
        one = single(eng, shape, lr, q)
        nsw = check_problem(probs[q], ps0[q], out[q], sels[q], nswaps=one.stats.nsweeps)
        assert (nsw > 0) == (n > 1)
        sc = abs(ps0[q].values).max()
        # wantZ = false leaves Z untouched and gives the same T
        assert all(np.array_equal(a, b) for a, b in zip(noz[q].Z, ps0[q].Z))
        assert max(np.abs(a - b).max() for a, b in zip(noz[q].Ts, out[q].Ts)) < 1e-12 * sc


# ------------------------------------------------------------------------------------------------
# 3. against the serial single driver
def _same(a, b):
    return (np.array_equal(a.values, b.values) and all(np.array_equal(x, y) for x, y in zip(a.Ts, b.Ts))
            and all(np.array_equal(x, y) for x, y in zip(a.Z, b.Z)))


def bits_differ(a, b):
    """The number of entries of T, Z and the values whose bits differ."""
    return sum(int((x != y).sum()) for x, y in zip(a.Ts + a.Z + [a.values], b.Ts + b.Z + [b.values]))


def case_against_serial(make_engine, shape, lr, exact):
    """The single driver with PSD_ORD_PIPE=0 moves one eigenvalue at a time through the same windows with the same
    arithmetic as the batched kernel; the row and column roles of a window touch disjoint entries, so the order of the
    items cannot matter.  exact: bit for bit (the simulation is built with -ffp-contract=off); otherwise 1e-12 * scale
    (contraction may differ between kernels).  Returns the number of entries whose bits differ."""
    nb, n, p = shape
    ser = make_engine({"PSD_ORD_PIPE": "0"})
    probs, ps0, sels = inputs(ser, shape, lr)
    out = ser.zordschur_batch_([_clone(ps) for ps in ps0], sels)
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
            assert _same(one, out[q]), (shape, lr, q)
        else:
            assert max(np.abs(a - b).max() for a, b in zip(one.Ts, out[q].Ts)) <= 1e-12 * sc
            assert max(np.abs(a - b).max() for a, b in zip(one.Z, out[q].Z)) <= 1e-12 * sc
            assert np.abs(one.values - out[q].values).max() <= 1e-12 * sc
    return differ


# ------------------------------------------------------------------------------------------------
# 4. independence
def case_independence(eng, shape, lr="R"):
    """A problem alone in a batch of one gets, bit for bit, what it gets inside the batch."""
    nb, n, p = shape
    probs, ps0, sels = inputs(eng, shape, lr)
    out = eng.zordschur_batch_([_clone(ps) for ps in ps0], sels)
    for q in sorted({0, nb - 2, nb - 1} & set(range(nb))):
        alone = eng.zordschur_batch_([_clone(ps0[q])], sels[q:q + 1])
        assert _same(alone[0], out[q]), (shape, q)


def case_groups(make_engine, shape=GROUP_SHAPE):
    """PSD_BATCH_GROUP=4: a batch worked through in two groups equals one group bit for bit."""
    nb, n, p = shape
    ref = make_engine({})
    eng = make_engine({"PSD_BATCH_GROUP": "4"})
    probs, ps0, sels = inputs(ref, shape, "L")
    whole = ref.zordschur_batch_([_clone(ps) for ps in ps0], sels)
    assert ref.zordschur_batch_stats.nlaunch_step == 1
    parts = eng.zordschur_batch_([_clone(ps) for ps in ps0], sels)
    assert eng.zordschur_batch_stats.nlaunch_step == 2
    for q in range(nb):
        assert _same(whole[q], parts[q]), q
        assert whole[q].stats.nsweeps == parts[q].stats.nsweeps > 0


# ------------------------------------------------------------------------------------------------
# 5. per-problem selections
def case_selections(eng):
    """all-false, all-true and the median rule side by side in one batch; one row for every problem"""
    shape = (1, 8, 3)
    n = shape[1]
    probs, ps0, _ = inputs(eng, shape, "R")
    A, ps0 = probs[0], ps0[0]
    sels = np.zeros((3, n), dtype=bool)
    sels[1] = True
    sels[2] = median_select(ps0.values)
    out = eng.zordschur_batch_([_clone(ps0) for _ in range(3)], sels)
    assert out[0].stats.nsweeps == 0 and out[1].stats.nsweeps == 0
    assert all(np.array_equal(a, b) for a, b in zip(out[0].Ts + out[0].Z, ps0.Ts + ps0.Z))  # untouched bit for bit
    assert np.allclose(out[0].values, ps0.values, rtol=1e-13, atol=0)  # (recomputed from the same diagonals)
    pt.pschur_check(A, out[1], check_lam=False, real=False)
    assert pt.match_eigs(ps0.values, out[1].values) < 1e-9 * abs(ps0.values).max()
    assert check_problem(A, ps0, out[2], sels[2]) > 0
    one = eng.zordschur_batch_([_clone(ps0) for _ in range(3)], sels[2])  # one row for every problem
    assert all(_same(o, out[2]) for o in one)


# ------------------------------------------------------------------------------------------------
# 6. one problem fails
def one_fails_inputs(eng):
    shape = (3, 4, 2)
    n, p = shape[1:]
    good, ps0, gsel = inputs(eng, shape, "R")
    # the problem of engine_cases.case_zordschur_edge: equal eigenvalues, the swap is rejected
    T = [np.asfortranarray(np.triu(np.ones((n, n))).astype(np.complex128)) for _ in range(p)]
    Z = [np.asfortranarray(np.eye(n, dtype=np.complex128)) for _ in range(p)]
    bad = psd_amd.PeriodicSchur(T, Z, np.ones(n, dtype=complex), "R", 1)
    probs = [good[0], [t.copy() for t in T], good[1], good[2]]
    work = [ps0[0], bad, ps0[1], ps0[2]]
    sels = np.array([gsel[0], [False, True, False, False], gsel[1], gsel[2]])
    return probs, work, sels


def case_one_fails(eng):
    probs, work, sels = one_fails_inputs(eng)
    with pytest.raises((psd_amd.SingularException, psd_amd.IllConditionedException)):
        eng.ordschur_(_clone(work[1]), sels[1])  # (the single call rejects it)
    infos = []
    out = eng.zordschur_batch_([_clone(ps) for ps in work], sels, infos_out=infos)
    assert len(infos) == 4 and infos[0] == 0 and infos[2] == 0 and infos[3] == 0, infos
    assert infos[1] == 3000 or 2000 <= infos[1] < 3000, infos
    for q in (0, 2, 3):
        check_problem(probs[q], work[q], out[q], sels[q])
    # the failed problem is still a decomposition of its product: Z_j' A_j Z_{j+1} = T_j
    pt.pschur_check(probs[1], out[1], check_lam=False, real=False)
    assert np.array_equal(out[1].values, work[1].values)
    again = [_clone(ps) for ps in work]
    with pytest.raises((psd_amd.SingularException, psd_amd.IllConditionedException)):  # raised after all four have run
        eng.zordschur_batch_(again, sels)
    for q in (0, 2, 3):
        assert _same(again[q], out[q])


# ------------------------------------------------------------------------------------------------
# 7. fallback above the cap
def case_above_cap(make_engine, shape=CAP_SHAPE):
    """PSD_BORD_NMAX=16 at order 20: the single driver problem by problem on the batch buffers — the single calls' bits."""
    nb, n, p = shape
    eng = make_engine({"PSD_BORD_NMAX": "16"})
    for lr in "RL":
        probs, ps0, sels = inputs(eng, shape, lr)
        out = eng.zordschur_batch_([_clone(ps) for ps in ps0], sels)
        assert eng.zordschur_batch_stats.nlaunch_step > 1
        for q in range(nb):
            one = eng.ordschur_(_clone(ps0[q]), sels[q])
            assert _same(one, out[q]) and one.stats.nsweeps == out[q].stats.nsweeps > 0


# ------------------------------------------------------------------------------------------------
# 8. C ABI and arguments
def raw(eng, fn, nb, n, p, T, Z, orient, si, sel, wantZ, alpha, beta, sc, infos=None, nsw=None, st=None):
    info = C.c_int(0)
    dp = C.POINTER(C.c_double)
    rc = fn(eng.ctx, nb, n, p, T, Z, orient, si, sel.ctypes.data_as(C.POINTER(C.c_uint8)) if sel is not None else None,
            wantZ, alpha.view(np.float64).ctypes.data_as(dp) if alpha is not None else None,
            beta.ctypes.data_as(dp) if beta is not None else None,
            sc.ctypes.data_as(C.POINTER(C.c_int32)) if sc is not None else None,
            infos, nsw, C.byref(st) if st is not None else None, C.byref(info))
    assert rc == info.value
    return rc


def case_argument_codes(eng, shape=CHAIN_SHAPE):
    nb, n, p = shape
    probs, ps0, sels = inputs(eng, shape, "R")
    w = _clone(ps0[0])
    Tp, Zp = eng._ptrs(w.Ts), eng._ptrs(w.Z)
    buf = np.zeros((p, n, n), dtype=np.complex128)
    sel = np.ascontiguousarray(sels[0], dtype=np.uint8)
    alpha, beta, sc = np.zeros(n, dtype=np.complex128), np.zeros(n), np.zeros(n, dtype=np.int32)
    for fn, T, Z in ((eng.lib.psd_z_ordschur_batch, Tp, Zp),
                     (eng.lib.psd_z_ordschur_batch_dev, C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data))):
        def f(nb_=1, n_=n, p_=p, T_=T, Z_=Z, o=b"R", si=1, sel_=sel, wz=1, a_=alpha, b_=beta, s_=sc):
            return raw(eng, fn, nb_, n_, p_, T_, Z_, o, si, sel_, wz, a_, b_, s_)
        assert f(n_=0) == -2 and f(p_=0) == -3 and f(T_=None) == -4 and f(Z_=None) == -5 and f(o=b"X") == -6
        assert f(si=2) == -7 and f(si=0) == -7 and f(si=p + 1) == -7  # strictly inside, or outside, the period
        assert f(sel_=None) == -8 and f(a_=None) == -9 and f(b_=None) == -9 and f(s_=None) == -9 and f(nb_=-1) == -11
        assert f(nb_=0) == 0 and f(nb_=0, T_=None) == 0
        info = C.c_int(0)
        assert fn(None, 1, n, p, T, Z, b"R", 1, sel.ctypes.data_as(C.POINTER(C.c_uint8)), 1, None, None, None, None, None,
                  None, C.byref(info)) == -1
    # a period-sharded context keeps a slice of Z: the batched entries refuse it (an engine of its own, let go afterwards)
    sharded = psd_amd.Engine(libpath=eng.lib._name)
    sharded.set_shard(0, 2)
    for fn, T, Z in ((sharded.lib.psd_z_ordschur_batch, Tp, Zp),
                     (sharded.lib.psd_z_ordschur_batch_dev, C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data))):
        assert raw(sharded, fn, 1, n, p, T, Z, b"R", 1, sel, 1, alpha, beta, sc) == psd_amd.INFO_NOTIMPL
        assert raw(sharded, fn, 0, n, p, T, Z, b"R", 1, sel, 1, alpha, beta, sc) == 0
    with pytest.raises(psd_amd.NotImplementedPSD):
        sharded.zordschur_batch_([_clone(ps0[0])], sels[:1])
    sharded.set_shard(0, 1)
    assert sharded.zordschur_batch_([_clone(ps0[0])], sels[:1])[0].stats.nsweeps > 0  # (whole again: accepted)
    # (no refused call touched anything)
    assert _same(w, ps0[0]) and not buf.any() and not alpha.any() and not beta.any() and not sc.any()


def case_python_errors(eng):
    nb, n, p = CHAIN_SHAPE
    probs, ps0, sels = inputs(eng, CHAIN_SHAPE, "R")
    other = eng.pschur(pt.bench_factors(9, p, seed=3, dtype=np.complex128), "R")
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zordschur_batch([ps0[0], other], np.zeros(n, dtype=bool))  # unequal order
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zordschur_batch([ps0[0], eng.pschur(probs[1], "L")], sels[:2])  # unequal orientation
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zordschur_batch(ps0[:2], np.zeros((2, n - 1), dtype=bool))  # select rows of the wrong length
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zordschur_batch(ps0[:2], np.zeros((3, n), dtype=bool))  # ... or the wrong number of them
    # ordschur_batch still refuses ComplexF64 and zordschur_batch refuses Float64, each naming the other
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.ordschur_batch([ps0[0]], sels[:1])
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.ordschur_batch_([_clone(ps0[0])], sels[:1])
    rl = eng.pschur(pt.bench_factors(n, p, seed=3), "R")
    for fn in (eng.zordschur_batch, eng.zordschur_batch_):
        with pytest.raises(psd_amd.NotImplementedPSD, match="ordschur_batch"):
            fn([_clone(rl)], sels[:1])
    S = [True] * p
    S[1] = False
    signed = psd_amd.GeneralizedPeriodicSchur(S, ps0[0].Ts, ps0[0].Z, ps0[0].values, np.ones(n), np.zeros(n, dtype=np.int32), "R", 1)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.zordschur_batch([signed], sels[:1])
    notf = _clone(ps0[0])
    notf.Ts[1] = np.ascontiguousarray(notf.Ts[1])
    with pytest.raises(TypeError):
        eng.zordschur_batch_([notf], sels[:1])  # in place needs Fortran order
    ro = _clone(ps0[0])
    ro.Z[0].setflags(write=False)
    with pytest.raises(TypeError):
        eng.zordschur_batch_([ro], sels[:1])  # ... and writable arrays
    mid = _clone(ps0[0])
    mid.schurindex = 2
    with pytest.raises(ValueError):
        eng.zordschur_batch_([mid], sels[:1])  # interior schurindex (ordschur.jl:32)
    assert eng.zordschur_batch_([], sels) == [] and eng.zordschur_batch([], sels[0]) == []
    infos = [7]
    assert eng.zordschur_batch_([], sels, infos_out=infos) == [] and infos == []
    keep = _clone(ps0[0])
    got = eng.zordschur_batch([ps0[0]], sels[:1])  # the copying form leaves its input alone
    assert _same(keep, ps0[0]) and got[0].stats.nsweeps > 0


# ------------------------------------------------------------------------------------------------
# 9. device entry through the C ABI
def case_dev_abi(eng, shape=CHAIN_SHAPE, launches=1, device=False):
    """psd_z_ordschur_batch_dev through the C ABI on packed [nb][p][n][n] column-major blocks — numpy arrays in the
    simulation, where device memory is host memory, torch CUDA tensors through data_ptr() on the GPU (device=True): the
    same bits as the host entry, for all four alignments of (orient, schurindex).
    `launches`: the groups the engine's PSD_BATCH_GROUP cuts the batch into (the shifted alignments are then gathered a
    group at a time as well)."""
    nb, n, p = shape
    for lr in "RL":
        probs, ps0, sels = inputs(eng, shape, lr)
        si0 = ps0[0].schurindex
        for si in (si0, p + 1 - si0):
            # (the other alignment of the same orientation: the same decomposition written with its factors shifted.
            #  Only the bits matter here.)
            shift = si != si0

            def placed(ps):
                q = _clone(ps)
                if shift:  # the triangular Schur factor goes from the first slot to the last, or back
                    q.Ts = (q.Ts[1:] + q.Ts[:1]) if si == p else (q.Ts[-1:] + q.Ts[:-1])
                    q.Z = (q.Z[1:] + q.Z[:1]) if si == p else (q.Z[-1:] + q.Z[:-1])
                    q.schurindex = si
                return q
            host = eng.zordschur_batch_([placed(ps) for ps in ps0], sels)
            hst = eng.zordschur_batch_stats
            src = [placed(ps) for ps in ps0]
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
            rc = raw(eng, eng.lib.psd_z_ordschur_batch_dev, nb, n, p, pT, pZ, lr.encode(), si, sel, 1, alpha, beta, sc,
                     infos, nsw, st)
            if device:  # (the entry returns with its stream drained)
                dT, dZ = gT.cpu().numpy(), gZ.cpu().numpy()
            assert rc == 0 and not any(infos) and st.nlaunch_step == hst.nlaunch_step == launches and st.window == hst.window
            assert st.nsweeps == hst.nsweeps == sum(nsw) > 0 and st.ms_total >= 0
            values = alpha / beta * np.exp2(sc.astype(np.float64))
            for q in range(nb):
                assert nsw[q] == host[q].stats.nsweeps
                assert np.array_equal(values[q], host[q].values)
                for j in range(p):
                    assert np.array_equal(dT[q, j].T, host[q].Ts[j]) and np.array_equal(dZ[q, j].T, host[q].Z[j]), (lr, si, q, j)


# ------------------------------------------------------------------------------------------------
# 11. device-resident chain (GPU tier)
def case_device_chain(eng, lr, shape=CHAIN_SHAPE):
    """zpschur_batch_ -> zordschur_batch_ without a matrix touching the host"""
    import torch

    nb, n, p = shape
    probs = factors(shape)
    si = p if lr == "L" else 1
    dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in probs])).cuda()
    T, Z, values, _ = eng.zpschur_batch_(dA, lr)
    sels = np.array([median_select(v) for v in values])
    ps0 = [psd_amd.PeriodicSchur([np.asfortranarray(T[q, j].cpu().numpy()) for j in range(p)],
                                 [np.asfortranarray(Z[q, j].cpu().numpy()) for j in range(p)], values[q].copy(), lr, si)
           for q in range(nb)]
    host = eng.zordschur_batch_([_clone(ps) for ps in ps0], sels)
    T1, Z1, values1, st = eng.zordschur_batch_(T, Z, sels, lr=lr, schurindex=si)
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
        ps1 = psd_amd.PeriodicSchur([np.asfortranarray(Th[q, j]) for j in range(p)],
                                    [np.asfortranarray(Zh[q, j]) for j in range(p)], values1[q], lr, si)
        ps1.stats = psd_amd.Stats()
        ps1.stats.nsweeps = int(eng.zordschur_batch_nswaps[q])
        check_problem(probs[q], ps0[q], ps1, sels[q], nswaps=host[q].stats.nsweeps)
    # any other layout is copied first: the input stays as it was
    Tc = T1.contiguous()
    keep = Tc.clone()
    T2, Z2, v2, _ = eng.zordschur_batch_(Tc, Z1.contiguous(), np.ones((nb, n), dtype=bool), lr=lr, schurindex=si)
    assert T2.data_ptr() != Tc.data_ptr() and torch.equal(Tc, keep) and torch.equal(T2, Tc)
    Tn, Zn, vn, _ = eng.zordschur_batch(T1, None, sels, lr=lr, schurindex=si, wantZ=False)  # copying form, no Z
    assert Zn is None and Tn.data_ptr() != T1.data_ptr() and torch.equal(T1.cpu(), torch.from_numpy(Th))
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zordschur_batch_(T1[:, :, :, :5], None, sels, lr=lr, schurindex=si, wantZ=False)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.zordschur_batch_(T1.real.contiguous(), None, sels, lr=lr, schurindex=si, wantZ=False)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.ordschur_batch_(T1, None, sels, lr=lr, schurindex=si, wantZ=False)
    if p > 2:
        with pytest.raises(ValueError):
            eng.zordschur_batch_(T1, Z1, sels, lr=lr, schurindex=2)
    # an empty batch is returned as it is and describes itself like any other call
    infos = [7]
    T0, Z0, v0, st0 = eng.zordschur_batch_(T1[:0], Z1[:0], sels[:0], lr=lr, schurindex=si, infos_out=infos)
    assert T0.shape[0] == 0 and v0.shape == (0, n) and infos == [] and st0.nlaunch_step == 0
    assert eng.zordschur_batch_stats.nsweeps == 0 and len(eng.zordschur_batch_nswaps) == 0
