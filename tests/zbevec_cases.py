"""Engine.zeigvecs_batch (psd_z_eigvecs_batch / psd_z_eigvecs_batch_dev, csrc/psd_zbevec.h): eigenvectors of many small
ComplexF64 periodic Schur forms in one call — the cases shared by the simulated tier (test_hostsim_zeigvecs_batch.py) and
the device tier (test_gpu_zeigvecs_batch.py); they mirror bevec_cases.py.  Every problem goes through
evec_cases.check_columns: relation ratio <= evec_cases.GATE, agreement with the numpy prototype backsub_ref at its atol,
norm and phase.  The inputs are evec_cases.schur_form(..., cplx=True) with the diagonals of `zdiag`: genuinely complex
eigenvalues, so the principal root matters.  On these inputs backsub_ref itself reaches a relation ratio of at most
4.7e-15 and norms within 5e-16 (shapes (p, n) = (3,7), (2,6), (1,5), (70,5), (3,1), (5,9), (32,4), (3,40), (2,129),
(3,12), seeds 5, 7, 9): far inside every gate."""
import ctypes as C

import numpy as np
import pytest

import bevec_cases as bc
import evec_cases as vc
import psd_amd
import psdtest as pt

_cache = {}
SEEDS = bc.SEEDS


def _shared(key, make):
    """Inputs are built once, shared among the cases, and never written to."""
    if key not in _cache:
        out = make()
        for ps, As in out:
            for a in list(ps.Ts) + list(ps.Z) + list(As):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def zdiag(n, p, seed):
    """per factor: moduli linspace(1, 2, n) ** (1/p) — every row's product has modulus linspace(1, 2, n)[row] — times
    phases exp(i U(-pi, pi))"""
    rs = np.random.RandomState(1000 + seed)
    return [np.linspace(1.0, 2.0, n) ** (1.0 / p) * np.exp(1j * rs.uniform(-np.pi, np.pi, n)) for _ in range(p)]


def zform(n, p, seed):
    """an ordinary complex problem"""
    return vc.schur_form(n, p, zdiag(n, p, seed), seed, cplx=True)


def _values(pss):
    """alpha [nb][n] complex, beta [nb][n] of a list of PeriodicSchur"""
    alpha = np.ascontiguousarray(np.array([np.asarray(ps.values, dtype=np.complex128) for ps in pss]))
    return alpha, np.ones(alpha.shape)


def raw_host(eng, pss, select, shifted=True, maxvec=None):
    """psd_z_eigvecs_batch through the C ABI (ascale NULL): (info, V [nb][nmat][maxvec][n] complex, nvec, counts, stats,
    select)."""
    nb, p, n = len(pss), len(pss[0].Ts), pss[0].Ts[0].shape[0]
    Ts = [np.asfortranarray(t, dtype=np.complex128) for ps in pss for t in ps.Ts]
    Zs = [np.asfortranarray(z, dtype=np.complex128) for ps in pss for z in ps.Z]
    alpha, beta = _values(pss)
    sel = np.ascontiguousarray(np.broadcast_to(np.asarray(select, dtype=bool), (nb, n)), dtype=np.uint8)
    dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    nvec = (C.c_int * nb)()
    cnts = np.zeros((nb, 3), dtype=np.int32)
    st = psd_amd.BevecStats()
    info = C.c_int(0)
    head = [eng.ctx, nb, n, p, eng._ptrs(Ts), eng._ptrs(Zs), alpha.ctypes.data_as(dp), beta.ctypes.data_as(dp), None,
            pss[0].orientation.encode(), pss[0].schurindex, sel.ctypes.data_as(u8p), int(shifted)]
    tail = [nvec, cnts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st), C.byref(info)]
    eng.lib.psd_z_eigvecs_batch(*head, None, 0, *tail)
    assert info.value == 0
    if maxvec is None:
        maxvec = max(nvec)
    nmat = p if shifted else 1
    V = np.full((nb, nmat, maxvec, n), 7.0 + 7.0j)  # (poisoned: the padding has to be written)
    Vp = (C.c_void_p * (nb * nmat))(*[V[q, l].ctypes.data for q in range(nb) for l in range(nmat)])
    rc = eng.lib.psd_z_eigvecs_batch(*head, Vp, maxvec, *tail)
    assert rc == info.value
    return info.value, V, list(nvec), cnts, st, sel


def check_batch(eng, probs, select):
    """run the batch, check every problem's columns; returns the vectors"""
    pss = [ps for ps, _ in probs]
    nb, n = len(pss), pss[0].Ts[0].shape[0]
    Vs = eng.zeigvecs_batch(pss, select)
    sel = np.broadcast_to(np.asarray(select, dtype=bool), (nb, n))
    assert len(Vs) == nb
    for q, (ps, As) in enumerate(probs):
        assert len(Vs[q]) == len(ps.Ts)
        vc.check_columns(ps, Vs[q], sel[q], As)
    return Vs


# ------------------------------------------------------------------------------------------------
# 1. mixed batch
def mixed_problems():
    return _shared("mixed", lambda: [zform(7, 3, SEEDS[q]) for q in range(5)])


MIXED_SELECT = np.array([
    [1, 1, 1, 1, 1, 1, 1],
    [0, 1, 0, 0, 1, 0, 0],
    [0, 0, 1, 0, 0, 0, 1],
    [1, 0, 0, 0, 0, 0, 0],
    [0, 1, 0, 0, 1, 1, 0],
], dtype=bool)
MIXED_NVEC = [7, 2, 2, 1, 3]  # (the rows as given: nothing to complete)


def case_mixed(eng):
    probs = mixed_problems()
    pss = [ps for ps, _ in probs]
    keep = [[a.copy() for a in list(ps.Ts) + list(ps.Z)] for ps in pss]
    Vs = check_batch(eng, probs, MIXED_SELECT)
    assert [V[0].shape[1] for V in Vs] == MIXED_NVEC
    V1 = eng.zeigvecs_batch(pss, MIXED_SELECT, shifted=False)
    for q in range(5):
        assert len(V1[q]) == 1 and np.array_equal(V1[q][0], Vs[q][0])  # bit-identical
    assert all(np.array_equal(a, b) for ps, k in zip(pss, keep) for a, b in zip(list(ps.Ts) + list(ps.Z), k))
    # the blocks as the ABI leaves them: n x maxvec, the columns at and beyond nvec exactly zero, select as given
    info, V, nvec, cnts, st, sel = raw_host(eng, pss, MIXED_SELECT)
    assert info == 0 and nvec == MIXED_NVEC and V.shape[2] == 7
    assert np.array_equal(sel, MIXED_SELECT.astype(np.uint8))
    for q in range(5):
        for l in range(3):
            assert np.array_equal(V[q, l, :nvec[q]].T, Vs[q][l])
            assert np.all(V[q, l, nvec[q]:] == 0)
    assert st.nb == 5 and st.nvec_total == sum(MIXED_NVEC) and not cnts.any()


# ------------------------------------------------------------------------------------------------
# 2. batch independence, bit for bit
def independence_problems():
    base = _shared("indep", lambda: [zform(6, 2, SEEDS[k]) for k in range(5)])
    return [base[q % 5] for q in range(70)]  # (70 crosses any grouping of 32 or 64 units or problems)


def _same(Va, Vb):
    return len(Va) == len(Vb) and all(np.array_equal(a, b) for a, b in zip(Va, Vb))


def case_independence(eng, eng_groups=None):
    """a problem alone, first, in the middle or last of 70, and run twice: the same bits (also under PSD_BATCH_GROUP=3)"""
    probs = independence_problems()
    pss = [ps for ps, _ in probs]
    select = np.ones(6, dtype=bool)
    whole = eng.zeigvecs_batch(pss, select)
    again = eng.zeigvecs_batch(pss, select)
    assert all(_same(a, b) for a, b in zip(whole, again))
    for q in range(5):
        vc.check_columns(pss[q], whole[q], select, probs[q][1])
    for pos in (0, 33, 69):
        alone = eng.zeigvecs_batch([pss[pos]], select)
        assert _same(alone[0], whole[pos]), pos
        for q in (0, 33, 69):  # the same problem at another place
            if q % 5 == pos % 5:
                assert _same(whole[q], whole[pos])
    rot = pss[33:] + pss[:33]
    turned = eng.zeigvecs_batch(rot, select)
    assert _same(turned[0], whole[33]) and _same(turned[36], whole[69]) and _same(turned[37], whole[0])
    if eng_groups is not None:
        parts = eng_groups.zeigvecs_batch(pss, select)
        assert eng_groups.eigvecs_batch_stats.ngroups == 24
        assert all(_same(a, b) for a, b in zip(whole, parts))


# ------------------------------------------------------------------------------------------------
# 3. factor layouts
LAYOUTS = bc.LAYOUTS  # (p, n)
layout_id = bc.layout_id


def case_layout(eng, shape):
    """p = 1; p = 70 (lanes own two factors); n = 1; p = 5 (idle lanes inside a sub-group of 8); p = 32 (one sub-group per
    half-wave)"""
    p, n = shape
    probs = _shared(("layout", shape), lambda: [zform(n, p, SEEDS[q]) for q in range(3)])
    check_batch(eng, probs, np.ones(n, dtype=bool))


# ------------------------------------------------------------------------------------------------
# 4. depth
def depth_problems():
    return _shared("depth", lambda: [zform(40, 3, s) for s in (5, 7, 9)])


def case_depth(eng):
    probs = depth_problems()
    for select in (np.ones(40, dtype=bool), np.arange(40) % 3 == 0):
        check_batch(eng, probs, select)


# ------------------------------------------------------------------------------------------------
# 5. special columns inside a batch
def case_special_repeated(eng):
    n, p = 6, 3
    probs = _shared("rep", lambda: [vc.schur_form(n, p, [np.full(n, 1.5) for _ in range(p)], seed=7, cplx=True),
                                    zform(n, p, 9)])
    select = np.ones(n, dtype=bool)
    Vs = eng.zeigvecs_batch([ps for ps, _ in probs], select)
    cnt = eng.eigvecs_batch_counts
    assert all(np.isfinite(V).all() for V in Vs[0]) and Vs[0][0].shape[1] == n
    assert cnt[0, 0] > 0 and cnt[0, 1] == 0 and cnt[0, 2] == 0 and not cnt[1].any()
    assert eng.eigvecs_batch_stats.nperturbed == cnt[0, 0]
    vc.check_columns(probs[1][0], Vs[1], select, probs[1][1])


def case_special_zero(eng):
    n, p = 6, 3
    diag = zdiag(n, p, 9)
    diag[0][3] = 0.0
    probs = _shared("zero", lambda: [zform(n, p, 7), vc.schur_form(n, p, diag, seed=9, cplx=True), zform(n, p, 5)])
    select = np.ones(n, dtype=bool)
    Vs = eng.zeigvecs_batch([ps for ps, _ in probs], select)
    cnt = eng.eigvecs_batch_counts
    assert cnt[:, 2].tolist() == [0, 1, 0] and eng.eigvecs_batch_stats.nzero == 1
    assert all(np.isnan(V[:, 3]).all() for V in Vs[1])
    keep = [0, 1, 2, 4, 5]
    assert vc.relation_ratio(probs[1][1], [V[:, keep] for V in Vs[1]], np.asarray(probs[1][0].values)[keep]) <= vc.GATE
    for q in (0, 2):  # the NaNs stay in their problem
        vc.check_columns(probs[q][0], Vs[q], select, probs[q][1])


def case_special_rescale(eng):
    """the rescale case of bevec_cases (diagonals graded over 2^+-175 inside the period) with complex phases"""
    n, p = 8, 6
    rs = np.random.RandomState(1000 + 23)
    diag = []
    for l in range(p):
        g = np.where(np.arange(n) % 2 == 1, 2.0 ** (175 if l < 3 else -175), 1.0)
        diag.append(np.linspace(1.0, 1.7, n) ** (1.0 / p) * g * np.exp(1j * rs.uniform(-np.pi, np.pi, n)))
    probs = _shared("resc", lambda: [zform(n, p, 5), vc.schur_form(n, p, diag, seed=23, cplx=True)])
    select = np.ones(n, dtype=bool)
    Vs = eng.zeigvecs_batch([ps for ps, _ in probs], select)
    cnt = eng.eigvecs_batch_counts
    assert cnt[1, 1] > 0 and cnt[0, 1] == 0 and eng.eigvecs_batch_stats.nrescaled == cnt[1, 1]
    ps, As = probs[1]
    assert all(np.isfinite(V).all() for V in Vs[1])
    assert vc.relation_ratio(As, Vs[1], np.asarray(ps.values)) <= vc.GATE
    ref = vc.backsub_ref(ps, select)
    for l in range(p):
        for c in range(n):
            err = np.linalg.norm(Vs[1][l][:, c] - ref[l][:, c])
            assert err <= 1e-9 * np.linalg.norm(ref[l][:, c]), (l, c, err)
    vc.check_columns(probs[0][0], Vs[0], select, probs[0][1])


# ------------------------------------------------------------------------------------------------
# 6. skipped problems
def case_skipped(eng):
    probs = mixed_problems()[:3]
    pss = [ps for ps, _ in probs]
    select = np.ones((3, 7), dtype=bool)
    select[1] = False
    Vs = eng.zeigvecs_batch(pss, select)
    assert all(V.shape == (7, 0) for V in Vs[1])
    for q in (0, 2):
        vc.check_columns(pss[q], Vs[q], select[q], probs[q][1])
    info, V, nvec, cnts, st, _ = raw_host(eng, pss, select)
    assert info == 0 and nvec == [7, 0, 7] and np.all(V[1] == 0)
    # nothing selected anywhere: nothing is launched
    none = eng.zeigvecs_batch(pss, np.zeros(7, dtype=bool))
    assert all(V.shape == (7, 0) for Vq in none for V in Vq)
    assert eng.eigvecs_batch_stats.nlaunch == 0 and eng.eigvecs_batch_stats.nvec_total == 0
    info, V, nvec, cnts, st, _ = raw_host(eng, pss, np.zeros(7, dtype=bool), maxvec=2)
    assert info == 0 and nvec == [0, 0, 0] and st.nlaunch == 0 and np.all(V == 0)


# ------------------------------------------------------------------------------------------------
# 7. launch count
def case_launch_count(eng):
    """the launches of a call depend neither on nb nor on n (below the cap): solve, V_1, norms, the other factors"""
    base = _shared("launch", lambda: [zform(12, 3, SEEDS[k]) for k in range(5)])
    counts = {}
    for nb in (3, 40):
        probs = [base[q % 5] for q in range(nb)]
        check_batch(eng, probs, np.ones(12, dtype=bool))
        counts[nb] = eng.eigvecs_batch_stats.nlaunch
    check_batch(eng, depth_problems(), np.ones(40, dtype=bool))
    deep = eng.eigvecs_batch_stats.nlaunch
    assert counts[3] == counts[40] == deep == 4, (counts, deep)
    assert eng.eigvecs_batch_stats.ngroups == 1
    eng.zeigvecs_batch([ps for ps, _ in base], np.ones(12, dtype=bool), shifted=False)
    assert eng.eigvecs_batch_stats.nlaunch == 3


# ------------------------------------------------------------------------------------------------
# 8. above the cap
def case_above_cap(eng):
    n, p = bc.bev_nmax() + 1, 2
    probs = _shared(("cap", n), lambda: [zform(n, p, s) for s in (5, 7)])
    select = np.zeros((2, n), dtype=bool)
    select[0] = np.arange(n) % 4 == 1  # (nvec differs: the staging into n x maxvec blocks)
    select[1] = np.arange(n) % 8 == 0
    check_batch(eng, probs, select)


# ------------------------------------------------------------------------------------------------
# 9. device entry through the C ABI (simulated tier)
def case_dev_abi(eng):
    """psd_z_eigvecs_batch_dev through the C ABI on packed blocks (in the simulation device memory is host memory): the
    same bits as the host entry, and the argument codes of both entries."""
    probs = mixed_problems()
    pss = [ps for ps, _ in probs]
    nb, n, p = 5, 7, 3
    host = eng.zeigvecs_batch(pss, MIXED_SELECT)
    dT = np.ascontiguousarray(np.array([pt.pack(ps.Ts, np.complex128) for ps in pss]))
    dZ = np.ascontiguousarray(np.array([pt.pack(ps.Z, np.complex128) for ps in pss]))
    alpha, beta = _values(pss)
    sc = np.zeros((nb, n), dtype=np.int32)
    sel = np.ascontiguousarray(MIXED_SELECT, dtype=np.uint8)
    dp, u8p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    nvec = (C.c_int * nb)()
    cnts = np.zeros((nb, 3), dtype=np.int32)
    st = psd_amd.BevecStats()
    info = C.c_int(0)
    lib, ctx = eng.lib, eng.ctx
    ap, bp, scp, selp = alpha.ctypes.data_as(dp), beta.ctypes.data_as(dp), sc.ctypes.data_as(i32p), sel.ctypes.data_as(u8p)
    bT, bZ = C.c_void_p(dT.ctypes.data), C.c_void_p(dZ.ctypes.data)
    rc = lib.psd_z_eigvecs_batch_dev(ctx, nb, n, p, bT, bZ, ap, bp, scp, b"L", p, selp, 1, None, 0, nvec,
                                     cnts.ctypes.data_as(i32p), C.byref(st), C.byref(info))
    assert rc == 0 and list(nvec) == MIXED_NVEC
    V = np.full((nb, p, 7, n), 7.0 + 7.0j)
    rc = lib.psd_z_eigvecs_batch_dev(ctx, nb, n, p, bT, bZ, ap, bp, scp, b"L", p, selp, 1, C.c_void_p(V.ctypes.data), 7,
                                     nvec, cnts.ctypes.data_as(i32p), C.byref(st), C.byref(info))
    assert rc == 0 and info.value == 0 and st.nb == nb and st.ngroups == 1 and st.nlaunch == 4
    assert st.ms_kernels >= st.ms_solve >= 0
    for q in range(nb):
        for l in range(p):
            assert np.array_equal(V[q, l, :nvec[q]].T, host[q][l]) and np.all(V[q, l, nvec[q]:] == 0)
    for q in range(nb):  # the inputs stay as they were
        assert np.array_equal(dT[q], pt.pack(pss[q].Ts, np.complex128))
        assert np.array_equal(dZ[q], pt.pack(pss[q].Z, np.complex128))
    assert np.array_equal(sel, MIXED_SELECT.astype(np.uint8)) and np.array_equal(alpha, _values(pss)[0])

    def dev_(c_=ctx, nb_=nb, n_=n, p_=p, T_=bT, Z_=bZ, a_=ap, b_=bp, o=b"L", si=p, sel_=selp, V_=None, mv=0, nv=nvec):
        return lib.psd_z_eigvecs_batch_dev(c_, nb_, n_, p_, T_, Z_, a_, b_, scp, o, si, sel_, 1, V_, mv, nv, None, None, None)

    Tp = eng._ptrs([np.asfortranarray(t, dtype=np.complex128) for ps in pss for t in ps.Ts])
    Zp = eng._ptrs([np.asfortranarray(z, dtype=np.complex128) for ps in pss for z in ps.Z])

    def host_(c_=ctx, nb_=nb, n_=n, p_=p, T_=Tp, Z_=Zp, a_=ap, b_=bp, o=b"L", si=p, sel_=selp, V_=None, mv=0, nv=nvec):
        return lib.psd_z_eigvecs_batch(c_, nb_, n_, p_, T_, Z_, a_, b_, scp, o, si, sel_, 1, V_, mv, nv, None, None, None)

    for f in (dev_, host_):
        assert f() == 0
        assert f(c_=None) == -1 and f(n_=0) == -2 and f(p_=0) == -3 and f(T_=None) == -4 and f(Z_=None) == -5
        assert f(a_=None) == -6 and f(b_=None) == -6 and f(o=b"X") == -7 and f(si=0) == -8 and f(si=p + 1) == -8
        assert f(sel_=None) == -9 and f(nb_=-1) == -11 and f(nv=None) == -12
        assert f(nb_=0, T_=None, Z_=None, a_=None, b_=None, sel_=None, nv=None) == 0  # nb == 0 touches nothing
    assert dev_(V_=C.c_void_p(V.ctypes.data), mv=6) == -10
    Vp = (C.c_void_p * (nb * p))(*[V[q, l].ctypes.data for q in range(nb) for l in range(p)])
    assert host_(V_=Vp, mv=6) == -10
    # a period-sharded context keeps a slice of Z: both entries refuse it
    sharded = psd_amd.Engine(libpath=eng.lib._name)
    sharded.set_shard(0, 2)
    assert dev_(c_=sharded.ctx) == psd_amd.INFO_NOTIMPL and host_(c_=sharded.ctx) == psd_amd.INFO_NOTIMPL


# ------------------------------------------------------------------------------------------------
# 10. errors
def case_errors(eng, make_engine):
    probs = mixed_problems()
    pss = [ps for ps, _ in probs]
    n, p = 7, 3
    with pytest.raises(ValueError, match="argument 9"):
        eng.zeigvecs_batch(pss, [True] * (n - 1))
    with pytest.raises(ValueError, match="argument 9"):
        eng.zeigvecs_batch(pss, np.ones((4, n), dtype=bool))
    bad = vc._clone(pss[1])
    bad.schurindex = p + 1
    with pytest.raises(ValueError, match="argument 8"):
        eng.zeigvecs_batch([bad, bad], [True] * n)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zeigvecs_batch([pss[0], zform(6, p, 5)[0]], [True] * n)  # unequal order
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zeigvecs_batch([pss[0], zform(n, 2, 5)[0]], [True] * n)  # unequal period
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.zeigvecs_batch([pss[0], bad], [True] * n)  # unequal schurindex
    real = bc.plain_form(n, p, 5)[0]
    with pytest.raises(TypeError, match="eigvecs_batch"):
        eng.zeigvecs_batch([real], [True] * n)  # Float64: the real entry
    with pytest.raises(psd_amd.NotImplementedPSD, match="zeigvecs_batch"):
        eng.eigvecs_batch([pss[0]], [True] * n)  # ... which still refuses ComplexF64, naming this one
    mixed = vc._clone(pss[0])
    mixed.Z = [np.asfortranarray(z.real) for z in mixed.Z]
    with pytest.raises(TypeError):
        eng.zeigvecs_batch([mixed], [True] * n)  # complex T with real Z
    mixed = vc._clone(real)
    mixed.Z = [z.astype(np.complex128) for z in mixed.Z]
    with pytest.raises(TypeError):
        eng.zeigvecs_batch([mixed], [True] * n)  # real T with complex Z
    g = psd_amd.GeneralizedPeriodicSchur([True, False, True], pss[0].Ts, pss[0].Z, np.array(pss[0].values), np.ones(n),
                                         np.zeros(n, dtype=np.int32), "L", p)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.zeigvecs_batch([pss[0], g], [True] * n)
    # an all-true signature is the plain decomposition (alpha / beta * 2^ascale its eigenvalues)
    g = psd_amd.GeneralizedPeriodicSchur([True] * p, pss[0].Ts, pss[0].Z, 0.5 * np.array(pss[0].values), np.full(n, 2.0),
                                         np.full(n, 2, dtype=np.int32), "L", p)
    sel = [True, False, True, False, False, True, True]
    assert _same(eng.zeigvecs_batch([g], sel)[0], eng.zeigvecs_batch([pss[0]], sel)[0])
    bad = vc._clone(pss[0])
    bad.Z = []
    with pytest.raises(ValueError):
        eng.zeigvecs_batch([bad], [True] * n)
    assert eng.zeigvecs_batch([], [True] * n) == []
    info, V, nvec, _, _, _ = raw_host(eng, pss, MIXED_SELECT, maxvec=6)  # problem 0 has 7 columns
    assert info == -10 and nvec == MIXED_NVEC
    sharded = make_engine()
    sharded.set_shard(0, 2)
    with pytest.raises(psd_amd.NotImplementedPSD):
        sharded.zeigvecs_batch(pss, [True] * n)


# ------------------------------------------------------------------------------------------------
# 11. pipeline, device-resident (GPU tier)
def case_pipeline(eng, lr):
    import torch

    n, p, nb = 12, 3, 5
    facs = [pt.bench_factors(n, p, seed=91 + q, dtype=np.complex128) for q in range(nb)]
    dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in facs])).cuda()
    T, Z, values, _ = eng.zpschur_batch_(dA, lr)
    si = p if lr == "L" else 1
    select = np.ones((nb, n), dtype=bool)
    select[1] = np.arange(n) % 2 == 0
    V, nvec = eng.zeigvecs_batch(T, Z, values, select, lr=lr, schurindex=si)
    assert nvec.tolist() == [n, n // 2, n, n, n]
    assert V.is_cuda and tuple(V.shape) == (nb, p, n, int(max(nvec)))
    Vh, Th, Zh = V.cpu().numpy(), T.cpu().numpy(), Z.cpu().numpy()
    for q in range(nb):
        Vs = [Vh[q, l][:, :nvec[q]] for l in range(p)]
        assert np.all(Vh[q][:, :, nvec[q]:] == 0)
        lams = np.asarray(values[q])[select[q]]
        assert Vs[0].shape[1] == len(lams)
        vc.ec.ev_check(facs[q], Vs, lams, left=(lr == "L"))
        r = vc.relation_ratio(facs[q], Vs, lams, left=(lr == "L"))
        assert r <= vc.GATE, (lr, q, r)
        single = eng.eigvecs_dev(T[q].transpose(1, 2).contiguous(), Z[q].transpose(1, 2).contiguous(), values[q],
                                 select[q], lr=lr, schurindex=si)
        for l in range(p):
            d = np.abs(Vs[l] - single[l].cpu().numpy()).max()
            print("pipeline %s q=%d l=%d: max |V_batch - V_single| = %.3e" % (lr, q, l, d))
            assert d <= 1e-9, (lr, q, l, d)
    V1, nvec1 = eng.zeigvecs_batch(T, Z, values, select, lr=lr, schurindex=si, shifted=False)
    assert tuple(V1.shape) == (nb, 1, n, int(max(nvec))) and torch.equal(V1[:, 0], V[:, 0])
    assert nvec1.tolist() == nvec.tolist()
    with pytest.raises(TypeError):
        eng.zeigvecs_batch(T.real.contiguous(), Z.real.contiguous(), values, select, lr=lr, schurindex=si)
    with pytest.raises(TypeError):
        eng.zeigvecs_batch(T, Z.real.contiguous(), values, select, lr=lr, schurindex=si)
    with pytest.raises(psd_amd.NotImplementedPSD, match="zeigvecs_batch"):
        eng.eigvecs_batch(T, Z, values, select, lr=lr, schurindex=si)
