"""Engine.ordschur_batch_ / ordschur_batch (psd_d_ordschur_batch / psd_d_ordschur_batch_dev, csrc/psd_bord.h): many small
periodic Schur forms reordered in one call — the cases shared by the simulated tier (test_hostsim_ordschur_batch.py) and
the device tier (test_gpu_ordschur_batch.py).  Inputs are pschur results of pt.bench_factors with the eigenvalues at or
below the median modulus selected, as engine_cases.case_rordschur_windows selects; its checks and bounds are applied to
every problem of a batch.  Problem 0 of a shape has that case's seed, the others fresh ones; pt.oracle_ordschur accepts
every swap of every one of them (asserted where the oracle runs)."""
import ctypes as C

import numpy as np
import pytest

import psd_amd
import psdtest as pt
from batch_common import shape_id  # noqa: F401 (used by the test files)
from engine_cases import _clone

# (nb, n, p): several windows at the widest W; narrow W from a large p (two of them); more problems than a 32-wide chunk
WINDOW_SHAPES = [(3, 48, 3), (2, 40, 22), (2, 30, 70), (33, 12, 3)]
NARROW_SHAPE = (3, 20, 3)  # with PSD_BORD_W=6: several windows at a small order
GROUP_SHAPE = (6, 20, 3)
CAP_SHAPE = (2, 20, 3)
CHAIN_SHAPE = (5, 12, 3)

_cache = {}


def factors(shape):
    """The factors of a shape: built once, shared, never written to."""
    nb, n, p = shape
    key = ("A", shape)
    if key not in _cache:
        probs = [pt.bench_factors(n, p, seed=90 + n + p + 1000 * q) for q in range(nb)]
        for A in probs:
            for a in A:
                a.setflags(write=False)
        _cache[key] = probs
    return _cache[key]


def median_select(lam):
    n = len(lam)
    return np.abs(lam) <= np.sort(np.abs(lam))[n // 2]


def inputs(eng, shape, lr):
    """(factors, decompositions, selections) of a shape and orientation on this engine; computed once and only cloned."""
    key = (id(eng), shape, lr)
    if key not in _cache:
        probs = factors(shape)
        ps0 = eng.pschur_batch(probs, lr)
        sels = np.array([median_select(ps.values) for ps in ps0])
        _cache[key] = (probs, ps0, sels, eng)  # (the engine lives as long as its entry: its id is not given out again)
    return _cache[key][:3]


def check_problem(A, ps0, ps1, select, oracle=True, nswaps=None):
    """The checks of engine_cases.case_rordschur_windows with its bounds, for one problem; returns the swap count."""
    n = A[0].shape[0]
    lam0 = ps0.values
    ok, err = pt.checkpsd(ps1, A, thresh=100 * np.sqrt(max(n / 32, 1)))
    assert ok, err
    closed = select.copy()  # (the device closes the selection under conjugation)
    for i in range(n - 1):
        if lam0[i].imag > 0 and (select[i] or select[i + 1]):
            closed[i] = closed[i + 1] = True
    m = int(closed.sum())
    sc = abs(lam0).max()
    assert pt.match_eigs(lam0[closed], ps1.values[:m]) < 1e-8 * sc
    assert pt.match_eigs(lam0[~closed], ps1.values[m:]) < 1e-8 * sc
    for i in range(n - 1):  # structure: sub-diagonal entries only inside conjugate pairs
        if ps1.values[i].imag == 0 or ps1.values[i].imag < 0:
            assert ps1.T1[i + 1, i] == 0
    if oracle:
        po = pt.oracle_ordschur(pt.PSD(ps0.Ts, ps0.Z, lam0, ps0.orientation, ps0.schurindex), select)
        assert po.info == 0 and ps1.stats.nsweeps == po.nswaps, (ps1.stats.nsweeps, po.nswaps)
    if nswaps is not None:
        assert ps1.stats.nsweeps == nswaps
    return ps1.stats.nsweeps


# ------------------------------------------------------------------------------------------------
# 1. reference shape
def case_reference(eng, lr):
    """engine_cases.case_rordschur_reference_real per problem of a batch: (nb, n, p) = (4, 7, 3), spectrum 4^j."""
    nb, n, p, nsel = 4, 7, 3, 2
    probs = []
    for q in range(nb):
        A = pt.ord_test_factors(n, p, seed=4000 + p + 37 * q)
        probs.append(A[::-1] if lr == "R" else A)
    ps0 = eng.pschur_batch(probs, lr)
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
        out = eng.ordschur_batch_([_clone(ps) for ps in ps0], np.array(sels))
        assert eng.ordschur_batch_stats.nlaunch_step == 1
        for q in range(nb):
            pt.pschur_check(probs[q], out[q], check_lam=False)
            for j in range(nsel):
                assert np.any(np.isclose(out[q].values[:nsel], ps0[q].values[idxs[q][j]], rtol=1e-8))


def case_pairs(eng):
    """engine_cases.case_rordschur_pairs as one batch: mkrps (3, 7, 2), pairs at rows 3:4 and 6:7, against the oracle."""
    n, p = 7, 2
    selsets = [[1, 2, 5], [1, 3, 4], [1, 2, 6, 7]]
    made = [pt.mkrps(n, p, [3, 6], seed=900 + p + 11 * q) for q in range(len(selsets))]
    work = [psd_amd.PeriodicSchur([t.copy(order="F") for t in ps0.Ts], [z.copy(order="F") for z in ps0.Z],
                                  ps0.values.copy(), "L", p) for ps0, _ in made]
    sels = np.zeros((len(selsets), n), dtype=bool)
    for q, ss in enumerate(selsets):
        sels[q, [j - 1 for j in ss]] = True
    out = eng.ordschur_batch_(work, sels)
    for q, (ps0, A) in enumerate(made):
        pt.pschur_check(A, out[q], check_lam=False)
        for j in selsets[q]:
            assert np.any(np.isclose(out[q].values[:len(selsets[q])], ps0.values[j - 1], rtol=1e-8))
        po = pt.oracle_ordschur(ps0, sels[q])
        assert po.info == 0 and out[q].stats.nsweeps == po.nswaps
        assert pt.match_eigs(po.values, out[q].values) < 1e-10 * abs(po.values).max()


# ------------------------------------------------------------------------------------------------
# 2. windows
def case_windows(eng, shape, lr, expect_window=None):
    nb, n, p = shape
    probs, ps0, sels = inputs(eng, shape, lr)
    out = eng.ordschur_batch_([_clone(ps) for ps in ps0], sels)
    st = eng.ordschur_batch_stats
    assert len(out) == nb and st.nlaunch_step == 1 and st.nsweeps == sum(ps.stats.nsweeps for ps in out)
    if expect_window is not None:
        assert st.window == expect_window and st.nwindows > nb  # (several windows per problem)
    noz = eng.ordschur_batch_([_clone(ps) for ps in ps0], sels, wantZ=False)
    for q in range(nb):
        single = eng.ordschur_(_clone(ps0[q]), sels[q])
        nsw = check_problem(probs[q], ps0[q], out[q], sels[q], nswaps=single.stats.nsweeps)
        assert nsw > 0
        sc = abs(ps0[q].values).max()
        assert pt.match_eigs(single.values, out[q].values) < 1e-9 * sc
        # wantZ = false leaves Z untouched and gives the same T
        assert all(np.array_equal(a, b) for a, b in zip(noz[q].Z, ps0[q].Z))
        assert max(np.abs(a - b).max() for a, b in zip(noz[q].Ts, out[q].Ts)) < 1e-12 * max(1.0, sc)


# ------------------------------------------------------------------------------------------------
# 3. independence
def _same(a, b):
    return (np.array_equal(a.values, b.values) and all(np.array_equal(x, y) for x, y in zip(a.Ts, b.Ts))
            and all(np.array_equal(x, y) for x, y in zip(a.Z, b.Z)))


def case_independence(eng, shape, lr="R"):
    """A problem alone in a batch of one gets, bit for bit, what it gets inside the batch."""
    nb, n, p = shape
    probs, ps0, sels = inputs(eng, shape, lr)
    out = eng.ordschur_batch_([_clone(ps) for ps in ps0], sels)
    for q in sorted({0, nb - 2, nb - 1} & set(range(nb))):
        alone = eng.ordschur_batch_([_clone(ps0[q])], sels[q:q + 1])
        assert _same(alone[0], out[q]), (shape, q)


def case_groups(make_engine, shape=GROUP_SHAPE):
    """PSD_BATCH_GROUP=4: a batch worked through in two groups equals one group bit for bit."""
    nb, n, p = shape
    ref = make_engine({})
    eng = make_engine({"PSD_BATCH_GROUP": "4"})
    probs, ps0, sels = inputs(ref, shape, "L")
    whole = ref.ordschur_batch_([_clone(ps) for ps in ps0], sels)
    assert ref.ordschur_batch_stats.nlaunch_step == 1
    parts = eng.ordschur_batch_([_clone(ps) for ps in ps0], sels)
    assert eng.ordschur_batch_stats.nlaunch_step == 2
    for q in range(nb):
        assert _same(whole[q], parts[q]), q


# ------------------------------------------------------------------------------------------------
# 4. per-problem selections
def case_selections(eng):
    """all-false, all-true, one member of a conjugate pair, and the median rule side by side in one batch"""
    n, p = 8, 3
    A = pt.bench_factors(n, p, seed=5)  # (the problem of engine_cases.case_rordschur_edge)
    ps0 = eng.pschur(A, "R")
    cp = np.where(ps0.values.imag > 0)[0]
    assert len(cp) > 0
    j = int(cp[-1])
    sels = np.zeros((4, n), dtype=bool)
    sels[1] = True
    sels[2, j + 1] = True
    sels[3] = median_select(ps0.values)
    out = eng.ordschur_batch_([_clone(ps0) for _ in range(4)], sels)
    assert out[0].stats.nsweeps == 0 and out[1].stats.nsweeps == 0
    assert all(np.array_equal(a, b) for a, b in zip(out[0].Ts + out[0].Z, ps0.Ts + ps0.Z))  # untouched bit for bit
    pt.pschur_check(A, out[1], check_lam=False)
    assert pt.match_eigs(ps0.values, out[1].values) < 1e-8 * abs(ps0.values).max()
    pt.pschur_check(A, out[2], check_lam=False)  # the partner comes along (rordschur.jl:46-75)
    assert np.isclose(out[2].values[0], ps0.values[j]) and np.isclose(out[2].values[1], ps0.values[j + 1])
    check_problem(A, ps0, out[2], sels[2])
    check_problem(A, ps0, out[3], sels[3])
    one = eng.ordschur_batch_([_clone(ps0) for _ in range(3)], sels[3])  # one row for every problem
    assert all(_same(o, out[3]) for o in one)


# ------------------------------------------------------------------------------------------------
# 5. one problem fails
def one_fails_inputs(eng):
    n, p = 4, 2
    good = [pt.bench_factors(n, p, seed=90 + n + p + 1000 * q) for q in range(3)]
    ps0 = [eng.pschur(A, "R") for A in good]
    T = [np.asfortranarray(np.triu(np.ones((n, n)))) for _ in range(p)]
    Z = [np.asfortranarray(np.eye(n)) for _ in range(p)]
    bad = psd_amd.PeriodicSchur(T, Z, np.ones(n, dtype=complex), "R", 1)  # equal eigenvalues: the swap is rejected
    probs = [good[0], [t.copy() for t in T], good[1], good[2]]
    work = [ps0[0], bad, ps0[1], ps0[2]]
    sels = np.array([median_select(ps0[0].values), [False, True, False, False], median_select(ps0[1].values),
                     median_select(ps0[2].values)])
    return probs, work, sels


def case_one_fails(eng):
    probs, work, sels = one_fails_inputs(eng)
    with pytest.raises((psd_amd.SingularException, psd_amd.IllConditionedException)):
        eng.ordschur_(_clone(work[1]), sels[1])  # (the single call rejects it)
    infos = []
    out = eng.ordschur_batch_([_clone(ps) for ps in work], sels, infos_out=infos)
    assert len(infos) == 4 and infos[0] == 0 and infos[2] == 0 and infos[3] == 0, infos
    assert infos[1] == 3000 or 2000 <= infos[1] < 3000, infos
    for q in (0, 2, 3):
        check_problem(probs[q], work[q], out[q], sels[q])
    # the failed problem is still a decomposition of its product: Z_j' A_j Z_{j+1} = T_j
    pt.pschur_check(probs[1], out[1], check_lam=False)
    assert np.array_equal(out[1].values, work[1].values)
    again = [_clone(ps) for ps in work]
    with pytest.raises((psd_amd.SingularException, psd_amd.IllConditionedException)):  # raised after all four have run
        eng.ordschur_batch_(again, sels)
    for q in (0, 2, 3):
        assert _same(again[q], out[q])


# ------------------------------------------------------------------------------------------------
# 6. fallback above the cap
def case_above_cap(make_engine, shape=CAP_SHAPE):
    """PSD_BORD_NMAX=16 at order 20: the single driver problem by problem on the batch buffers — the single calls' bits."""
    nb, n, p = shape
    eng = make_engine({"PSD_BORD_NMAX": "16"})
    for lr in "RL":
        probs, ps0, sels = inputs(eng, shape, lr)
        out = eng.ordschur_batch_([_clone(ps) for ps in ps0], sels)
        assert eng.ordschur_batch_stats.nlaunch_step > 1
        for q in range(nb):
            single = eng.ordschur_(_clone(ps0[q]), sels[q])
            assert _same(single, out[q]) and single.stats.nsweeps == out[q].stats.nsweeps > 0


# ------------------------------------------------------------------------------------------------
# 7. C ABI and arguments
def raw(eng, fn, nb, n, p, T, Z, orient, si, sel, wantZ, wr, wi, infos=None, nsw=None, st=None):
    info = C.c_int(0)
    dp = C.POINTER(C.c_double)
    rc = fn(eng.ctx, nb, n, p, T, Z, orient, si, sel.ctypes.data_as(C.POINTER(C.c_uint8)) if sel is not None else None,
            wantZ, wr.ctypes.data_as(dp) if wr is not None else None, wi.ctypes.data_as(dp) if wi is not None else None,
            infos, nsw, C.byref(st) if st is not None else None, C.byref(info))
    assert rc == info.value
    return rc


def case_argument_codes(eng, shape=CHAIN_SHAPE):
    nb, n, p = shape
    probs, ps0, sels = inputs(eng, shape, "R")
    w = _clone(ps0[0])
    Tp, Zp = eng._ptrs(w.Ts), eng._ptrs(w.Z)
    buf = np.zeros((p, n, n))
    sel = np.ascontiguousarray(sels[0], dtype=np.uint8)
    wr, wi = np.zeros(n), np.zeros(n)
    for fn, T, Z in ((eng.lib.psd_d_ordschur_batch, Tp, Zp),
                     (eng.lib.psd_d_ordschur_batch_dev, C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data))):
        def f(nb_=1, n_=n, p_=p, T_=T, Z_=Z, o=b"R", si=1, sel_=sel, wz=1, wr_=wr, wi_=wi):
            return raw(eng, fn, nb_, n_, p_, T_, Z_, o, si, sel_, wz, wr_, wi_)
        assert f(n_=0) == -2 and f(p_=0) == -3 and f(T_=None) == -4 and f(Z_=None) == -5 and f(o=b"X") == -6
        assert f(si=2) == -7 and f(si=0) == -7 and f(si=p + 1) == -7  # strictly inside, or outside, the period
        assert f(sel_=None) == -8 and f(wr_=None) == -9 and f(wi_=None) == -9 and f(nb_=-1) == -11
        assert f(nb_=0) == 0 and f(nb_=0, T_=None) == 0
        info = C.c_int(0)
        assert fn(None, 1, n, p, T, Z, b"R", 1, sel.ctypes.data_as(C.POINTER(C.c_uint8)), 1, None, None, None, None, None,
                  C.byref(info)) == -1
    assert np.array_equal(w.Ts[0], ps0[0].Ts[0]) and not buf.any()  # (no refused call touched anything)


def case_python_errors(eng):
    nb, n, p = CHAIN_SHAPE
    probs, ps0, sels = inputs(eng, CHAIN_SHAPE, "R")
    other = eng.pschur(pt.bench_factors(9, p, seed=3), "R")
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.ordschur_batch([ps0[0], other], np.zeros(n, dtype=bool))  # unequal order
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.ordschur_batch([ps0[0], eng.pschur(probs[1], "L")], sels[:2])  # unequal orientation
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.ordschur_batch(ps0[:2], np.zeros((2, n - 1), dtype=bool))  # select rows of the wrong length
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.ordschur_batch(ps0[:2], np.zeros((3, n), dtype=bool))  # ... or the wrong number of them
    cz = psd_amd.PeriodicSchur([t.astype(np.complex128) for t in ps0[0].Ts], [z.astype(np.complex128) for z in ps0[0].Z],
                               ps0[0].values, "R", 1)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.ordschur_batch([cz], sels[:1])
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.ordschur_batch_([cz], sels[:1])
    S = [True] * p
    S[1] = False
    signed = psd_amd.GeneralizedPeriodicSchur(S, ps0[0].Ts, ps0[0].Z, ps0[0].values, np.ones(n), np.zeros(n, dtype=np.int32), "R", 1)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.ordschur_batch([signed], sels[:1])
    notf = _clone(ps0[0])
    notf.Ts[1] = np.ascontiguousarray(notf.Ts[1])
    with pytest.raises(TypeError):
        eng.ordschur_batch_([notf], sels[:1])  # in place needs Fortran order
    ro = _clone(ps0[0])
    ro.Z[0].setflags(write=False)
    with pytest.raises(TypeError):
        eng.ordschur_batch_([ro], sels[:1])  # ... and writable arrays
    mid = _clone(ps0[0])
    mid.schurindex = 2
    with pytest.raises(ValueError):
        eng.ordschur_batch_([mid], sels[:1])  # interior schurindex (rordschur.jl:25)
    assert eng.ordschur_batch_([], sels) == [] and eng.ordschur_batch([], sels[0]) == []
    infos = [7]
    assert eng.ordschur_batch_([], sels, infos_out=infos) == [] and infos == []
    keep = _clone(ps0[0])
    eng.ordschur_batch([ps0[0]], sels[:1])  # the copying form leaves its input alone
    assert _same(keep, ps0[0])


def case_dev_abi(eng, shape=CHAIN_SHAPE, launches=1):
    """psd_d_ordschur_batch_dev through the C ABI on packed [nb][p][n][n] column-major blocks (in the simulation device
    memory is host memory): the same bits as the host entry, for all four alignments of (orient, schurindex).
    `launches`: the groups the engine's PSD_BATCH_GROUP cuts the batch into (the shifted alignments are then gathered a
    group at a time as well)."""
    nb, n, p = shape
    for lr in "RL":
        probs, ps0, sels = inputs(eng, shape, lr)
        si0 = ps0[0].schurindex
        for si in (si0, p + 1 - si0):
            # (the other alignment of the same orientation: the same decomposition written with its factors shifted —
            #  'R': P_1 = T_1 ... T_p -> T_p T_1 ... T_{p-1}; 'L' alike.  Only the bits matter here.)
            shift = si != si0
            def placed(ps):
                q = _clone(ps)
                if shift:  # the quasi-triangular factor goes from the first slot to the last, or back
                    q.Ts = (q.Ts[1:] + q.Ts[:1]) if si == p else (q.Ts[-1:] + q.Ts[:-1])
                    q.Z = (q.Z[1:] + q.Z[:1]) if si == p else (q.Z[-1:] + q.Z[:-1])
                    q.schurindex = si
                return q
            host = eng.ordschur_batch_([placed(ps) for ps in ps0], sels)
            hst = eng.ordschur_batch_stats
            src = [placed(ps) for ps in ps0]
            dT = np.ascontiguousarray(np.array([pt.pack(ps.Ts) for ps in src]))
            dZ = np.ascontiguousarray(np.array([pt.pack(ps.Z) for ps in src]))
            wr, wi = np.zeros((nb, n)), np.zeros((nb, n))
            infos, nsw = (C.c_int * nb)(), (C.c_int * nb)()
            st = psd_amd.Stats()
            sel = np.ascontiguousarray(sels, dtype=np.uint8)
            rc = raw(eng, eng.lib.psd_d_ordschur_batch_dev, nb, n, p, C.c_void_p(dT.ctypes.data), C.c_void_p(dZ.ctypes.data),
                     lr.encode(), si, sel, 1, wr, wi, infos, nsw, st)
            assert rc == 0 and not any(infos) and st.nlaunch_step == hst.nlaunch_step == launches and st.window == hst.window
            assert st.nsweeps == hst.nsweeps == sum(nsw) and st.ms_total >= 0
            for q in range(nb):
                assert nsw[q] == host[q].stats.nsweeps
                assert np.array_equal(wr[q] + 1j * wi[q], host[q].values)
                for j in range(p):
                    assert np.array_equal(dT[q, j].T, host[q].Ts[j]) and np.array_equal(dZ[q, j].T, host[q].Z[j]), (lr, si, q, j)


# ------------------------------------------------------------------------------------------------
# 8. device-resident chain (GPU tier)
def case_device_chain(eng, lr, shape=CHAIN_SHAPE):
    """pschur_batch_ -> ordschur_batch_ -> eigvecs_batch without a matrix touching the host"""
    import torch

    import evec_cases as vc

    nb, n, p = shape
    probs = factors(shape)
    si = p if lr == "L" else 1
    dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in probs])).cuda()
    T, Z, values, _ = eng.pschur_batch_(dA, lr)
    sels = np.array([median_select(v) for v in values])
    ps0 = [psd_amd.PeriodicSchur([np.asfortranarray(T[q, j].cpu().numpy()) for j in range(p)],
                                 [np.asfortranarray(Z[q, j].cpu().numpy()) for j in range(p)], values[q].copy(), lr, si)
           for q in range(nb)]
    host = eng.ordschur_batch_([_clone(ps) for ps in ps0], sels)
    T1, Z1, values1, st = eng.ordschur_batch_(T, Z, sels, lr=lr, schurindex=si)
    assert T1.data_ptr() == T.data_ptr() and Z1.data_ptr() == Z.data_ptr() and T1.stride() == T.stride()  # in place
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
        ps1.stats.nsweeps = int(eng.ordschur_batch_nswaps[q])
        check_problem(probs[q], ps0[q], ps1, sels[q], nswaps=host[q].stats.nsweeps)
    # the leading group's eigenvectors: the columns of the invariant subspace just moved to the top
    lead = np.zeros((nb, n), dtype=bool)
    for q in range(nb):
        closed = sels[q].copy()  # (the device closes the selection under conjugation)
        for i in range(n - 1):
            if values[q][i].imag > 0 and (closed[i] or closed[i + 1]):
                closed[i] = closed[i + 1] = True
        lead[q, :int(closed.sum())] = True
    V, nvec = eng.eigvecs_batch(T1, Z1, values1, lead, lr=lr, schurindex=si)
    Vh = V.cpu().numpy()
    for q in range(nb):
        ps1 = psd_amd.PeriodicSchur([np.asfortranarray(Th[q, j]) for j in range(p)],
                                    [np.asfortranarray(Zh[q, j]) for j in range(p)], values1[q], lr, si)
        Vs = [Vh[q, l][:, :nvec[q]] for l in range(p)]
        lams = vc.order_values(ps1, lead[q])
        assert Vs[0].shape[1] == len(lams) == int(lead[q].sum())
        vc.ec.ev_check(probs[q], Vs, lams, left=(lr == "L"))
        assert vc.relation_ratio(probs[q], Vs, lams, left=(lr == "L")) <= vc.GATE, (lr, q)
    # any other layout is copied first: the input stays as it was
    Tc = T1.contiguous()
    keep = Tc.clone()
    T2, Z2, v2, _ = eng.ordschur_batch_(Tc, Z1.contiguous(), np.ones((nb, n), dtype=bool), lr=lr, schurindex=si)
    assert T2.data_ptr() != Tc.data_ptr() and torch.equal(Tc, keep) and torch.equal(T2, Tc)
    Tn, Zn, vn, _ = eng.ordschur_batch(T1, None, sels, lr=lr, schurindex=si, wantZ=False)  # copying form, no Z
    assert Zn is None and Tn.data_ptr() != T1.data_ptr() and torch.equal(T1.cpu(), torch.from_numpy(Th))
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.ordschur_batch_(T1[:, :, :, :5], None, sels, lr=lr, schurindex=si, wantZ=False)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.ordschur_batch_(T1.to(torch.complex128), None, sels, lr=lr, schurindex=si, wantZ=False)
    if p > 2:
        with pytest.raises(ValueError):
            eng.ordschur_batch_(T1, Z1, sels, lr=lr, schurindex=2)
