"""Engine.eigvecs_batch (psd_d_eigvecs_batch / psd_d_eigvecs_batch_dev, csrc/psd_bevec.h): eigenvectors of many small
periodic Schur forms in one call — the cases shared by the simulated tier (test_hostsim_eigvecs_batch.py) and the device
tier (test_gpu_eigvecs_batch.py).  Every problem goes through evec_cases.check_columns: relation ratio <= evec_cases.GATE,
agreement with the numpy prototype backsub_ref at its atol, norm, phase and conjugates.  The inputs come from the
generators and seeds of the single-problem tests (evec_cases.schur_form, psdtest.bench_factors)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import evec_cases as vc
import psd_amd
import psdtest as pt

_cache = {}


def _shared(key, make):
    """Inputs are built once, shared among the cases, and never written to."""
    if key not in _cache:
        out = make()
        for ps, As in out:
            for a in list(ps.Ts) + list(ps.Z) + list(As):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def bev_nmax():
    """PSD_BEV_NMAX as the kernel header defines it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "periodicschurdecompositions.jl_amd", "csrc", "psd_bevec.h")) as fh:
        return int(re.search(r"^#define PSD_BEV_NMAX (\d+)", fh.read(), re.M).group(1))


SEEDS = (5, 7, 9, 17, 23)  # (the seeds of evec_cases' own schur_form problems)


def plain_form(n, p, seed, pairs=()):
    """an ordinary problem: every row's product of diagonals is linspace(1, 2, n)[row], distinct and moderate"""
    return vc.schur_form(n, p, [np.linspace(1.0, 2.0, n) ** (1.0 / p) for _ in range(p)], seed=seed, pairs=pairs)


def raw_host(eng, pss, select, shifted=True, maxvec=None):
    """psd_d_eigvecs_batch through the C ABI: (info, V [nb][nmat][maxvec][n] complex, nvec, counts, stats, select)."""
    nb, p, n = len(pss), len(pss[0].Ts), pss[0].Ts[0].shape[0]
    Ts = [np.asfortranarray(t, dtype=np.float64) for ps in pss for t in ps.Ts]
    Zs = [np.asfortranarray(z, dtype=np.float64) for ps in pss for z in ps.Z]
    vals = np.array([np.asarray(ps.values, dtype=complex) for ps in pss])
    wr, wi = np.ascontiguousarray(vals.real), np.ascontiguousarray(vals.imag)
    sel = np.ascontiguousarray(np.broadcast_to(np.asarray(select, dtype=bool), (nb, n)), dtype=np.uint8)
    dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    nvec = (C.c_int * nb)()
    cnts = np.zeros((nb, 3), dtype=np.int32)
    st = psd_amd.BevecStats()
    info = C.c_int(0)
    head = [eng.ctx, nb, n, p, eng._ptrs(Ts), eng._ptrs(Zs), wr.ctypes.data_as(dp), wi.ctypes.data_as(dp),
            pss[0].orientation.encode(), pss[0].schurindex, sel.ctypes.data_as(u8p), int(shifted)]
    tail = [nvec, cnts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st), C.byref(info)]
    eng.lib.psd_d_eigvecs_batch(*head, None, 0, *tail)
    assert info.value == 0
    if maxvec is None:
        maxvec = max(nvec)
    nmat = p if shifted else 1
    V = np.full((nb, nmat, maxvec, n), 7.0 + 7.0j)  # (poisoned: the padding has to be written)
    Vp = (C.c_void_p * (nb * nmat))(*[V[q, l].ctypes.data for q in range(nb) for l in range(nmat)])
    rc = eng.lib.psd_d_eigvecs_batch(*head, Vp, maxvec, *tail)
    assert rc == info.value
    return info.value, V, list(nvec), cnts, st, sel


def check_batch(eng, probs, select):
    """run the batch, check every problem's columns; returns the vectors"""
    pss = [ps for ps, _ in probs]
    nb, n = len(pss), pss[0].Ts[0].shape[0]
    Vs = eng.eigvecs_batch(pss, select)
    sel = np.broadcast_to(np.asarray(select, dtype=bool), (nb, n))
    assert len(Vs) == nb
    for q, (ps, As) in enumerate(probs):
        assert len(Vs[q]) == len(ps.Ts)
        vc.check_columns(ps, Vs[q], sel[q], As)
    return Vs


# ------------------------------------------------------------------------------------------------
# 1. mixed batch
def mixed_problems():
    n, p = 7, 3
    pairs = [(), (0,), (2, 5), (4,), (1, 3)]
    return _shared("mixed", lambda: [plain_form(n, p, SEEDS[q], pairs[q]) for q in range(5)])


MIXED_SELECT = np.array([
    [1, 1, 1, 1, 1, 1, 1],
    [0, 1, 0, 0, 1, 0, 0],  # (row 1 is the SECOND member of the pair at rows 0, 1)
    [0, 0, 1, 0, 0, 0, 1],
    [1, 0, 0, 0, 0, 0, 0],
    [0, 1, 0, 0, 1, 1, 0],
], dtype=bool)
MIXED_NVEC = [7, 3, 4, 1, 5]


def case_mixed(eng):
    probs = mixed_problems()
    pss = [ps for ps, _ in probs]
    keep = [[a.copy() for a in list(ps.Ts) + list(ps.Z)] for ps in pss]
    Vs = check_batch(eng, probs, MIXED_SELECT)
    assert [V[0].shape[1] for V in Vs] == MIXED_NVEC
    V1 = eng.eigvecs_batch(pss, MIXED_SELECT, shifted=False)
    for q in range(5):
        assert len(V1[q]) == 1 and np.array_equal(V1[q][0], Vs[q][0])  # bit-identical
        for V in Vs[q]:  # the partner of a pair is the exact conjugate
            lam = vc.order_values(pss[q], MIXED_SELECT[q])
            for c in range(len(lam) - 1):
                if lam[c].imag > 0:
                    assert np.array_equal(V[:, c + 1], np.conj(V[:, c]))
    assert all(np.array_equal(a, b) for ps, k in zip(pss, keep) for a, b in zip(list(ps.Ts) + list(ps.Z), k))
    # the blocks as the ABI leaves them: n x maxvec, the columns at and beyond nvec exactly zero, select completed
    info, V, nvec, cnts, st, sel = raw_host(eng, pss, MIXED_SELECT)
    assert info == 0 and nvec == MIXED_NVEC and V.shape[2] == 7
    assert sel[1].tolist() == [1, 1, 0, 0, 1, 0, 0] and sel[2].tolist() == [0, 0, 1, 1, 0, 1, 1]
    for q in range(5):
        for l in range(3):
            assert np.array_equal(V[q, l, :nvec[q]].T, Vs[q][l])
            assert np.all(V[q, l, nvec[q]:] == 0)
    assert st.nb == 5 and st.nvec_total == sum(MIXED_NVEC) and not cnts.any()


# ------------------------------------------------------------------------------------------------
# 2. batch independence, bit for bit
def independence_problems():
    n, p = 6, 2
    pairs = [(), (1,), (3,), (0, 4), (2,)]
    base = _shared("indep", lambda: [plain_form(n, p, SEEDS[k], pairs[k]) for k in range(5)])
    return [base[q % 5] for q in range(70)]  # (70 crosses any grouping of 32 or 64 units or problems)


def _same(Va, Vb):
    return len(Va) == len(Vb) and all(np.array_equal(a, b) for a, b in zip(Va, Vb))


def case_independence(eng, eng_groups=None):
    """a problem alone, first, in the middle or last of 70, and run twice: the same bits (also under PSD_BATCH_GROUP=3)"""
    probs = independence_problems()
    pss = [ps for ps, _ in probs]
    select = np.ones(6, dtype=bool)
    whole = eng.eigvecs_batch(pss, select)
    again = eng.eigvecs_batch(pss, select)
    assert all(_same(a, b) for a, b in zip(whole, again))
    for q in range(5):
        vc.check_columns(pss[q], whole[q], select, probs[q][1])
    for pos in (0, 33, 69):
        alone = eng.eigvecs_batch([pss[pos]], select)
        assert _same(alone[0], whole[pos]), pos
        for q in (0, 33, 69):  # the same problem at another place
            if q % 5 == pos % 5:
                assert _same(whole[q], whole[pos])
    rot = pss[33:] + pss[:33]
    turned = eng.eigvecs_batch(rot, select)
    assert _same(turned[0], whole[33]) and _same(turned[36], whole[69]) and _same(turned[37], whole[0])
    if eng_groups is not None:
        parts = eng_groups.eigvecs_batch(pss, select)
        assert eng_groups.eigvecs_batch_stats.ngroups == 24
        assert all(_same(a, b) for a, b in zip(whole, parts))


# ------------------------------------------------------------------------------------------------
# 3. factor layouts
LAYOUTS = [(1, 5), (70, 5), (3, 1), (5, 9), (32, 4)]  # (p, n)


def layout_id(s):
    return "p%d_n%d" % s


def case_layout(eng, shape):
    """p = 1; p = 70 (lanes own two factors); n = 1; p = 5 (idle lanes inside a sub-group of 8); p = 32 (one sub-group per
    half-wave)"""
    p, n = shape
    pairs = [(), (1,) if n >= 4 else (), (n - 2,) if n >= 4 else ()]
    probs = _shared(("layout", shape), lambda: [plain_form(n, p, SEEDS[q], pairs[q]) for q in range(3)])
    check_batch(eng, probs, np.ones(n, dtype=bool))


# ------------------------------------------------------------------------------------------------
# 4. depth
def depth_problems():
    n, p = 40, 3
    rs = np.random.RandomState(13)
    diag = [np.linspace(0.6, 1.9, n) * (1 + 0.2 * rs.rand(n)) for _ in range(p)]  # (evec_cases.case_chunks)
    return _shared("depth", lambda: [vc.schur_form(n, p, diag, seed=s, pairs=(5, 23, 37)) for s in (17, 7, 9)])


def case_depth(eng):
    probs = depth_problems()
    for select in (np.ones(40, dtype=bool), np.arange(40) % 3 == 0):
        check_batch(eng, probs, select)


# ------------------------------------------------------------------------------------------------
# 5. special columns inside a batch
def case_special_negative(eng):
    """evec_cases.case_negative_even_p beside an ordinary problem"""
    n, p = 6, 4
    diag = [np.linspace(1.0, 2.0, n) for _ in range(p)]
    diag[1] = diag[1].copy()
    diag[1][2] = -1.3
    probs = _shared("neg", lambda: [plain_form(n, p, 7, (4,)), vc.schur_form(n, p, diag, seed=5, pairs=(4,))])
    Vs = check_batch(eng, probs, np.ones(n, dtype=bool))
    assert np.abs(Vs[1][0][:, 2].imag).max() < 1e-12 and np.abs(Vs[1][1][:, 2].imag).max() > 1e-3
    assert not eng.eigvecs_batch_counts.any()


def case_special_repeated(eng):
    n, p = 6, 3
    probs = _shared("rep", lambda: [vc.schur_form(n, p, [np.full(n, 1.5) for _ in range(p)], seed=7),
                                    plain_form(n, p, 9)])
    select = np.ones(n, dtype=bool)
    Vs = eng.eigvecs_batch([ps for ps, _ in probs], select)
    cnt = eng.eigvecs_batch_counts
    assert all(np.isfinite(V).all() for V in Vs[0]) and Vs[0][0].shape[1] == n
    assert cnt[0, 0] > 0 and cnt[0, 1] == 0 and cnt[0, 2] == 0 and not cnt[1].any()
    assert eng.eigvecs_batch_stats.nperturbed == cnt[0, 0]
    vc.check_columns(probs[1][0], Vs[1], select, probs[1][1])


def case_special_zero(eng):
    n, p = 6, 3
    diag = [np.linspace(1.0, 2.0, n) for _ in range(p)]
    diag[0] = diag[0].copy()
    diag[0][3] = 0.0
    probs = _shared("zero", lambda: [plain_form(n, p, 7), vc.schur_form(n, p, diag, seed=9), plain_form(n, p, 5)])
    select = np.ones(n, dtype=bool)
    Vs = eng.eigvecs_batch([ps for ps, _ in probs], select)
    cnt = eng.eigvecs_batch_counts
    assert cnt[:, 2].tolist() == [0, 1, 0] and eng.eigvecs_batch_stats.nzero == 1
    assert all(np.isnan(V[:, 3]).all() for V in Vs[1])
    keep = [0, 1, 2, 4, 5]
    assert vc.relation_ratio(probs[1][1], [V[:, keep] for V in Vs[1]], np.asarray(probs[1][0].values)[keep]) <= vc.GATE
    for q in (0, 2):  # the NaNs stay in their problem
        vc.check_columns(probs[q][0], Vs[q], select, probs[q][1])


def case_special_rescale(eng):
    n, p = 8, 6
    diag = []
    for l in range(p):
        g = np.where(np.arange(n) % 2 == 1, 2.0 ** (175 if l < 3 else -175), 1.0)
        diag.append(np.linspace(1.0, 1.7, n) ** (1.0 / p) * g)
    probs = _shared("resc", lambda: [plain_form(n, p, 5), vc.schur_form(n, p, diag, seed=23)])
    select = np.ones(n, dtype=bool)
    Vs = eng.eigvecs_batch([ps for ps, _ in probs], select)
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
    Vs = eng.eigvecs_batch(pss, select)
    assert all(V.shape == (7, 0) for V in Vs[1])
    for q in (0, 2):
        vc.check_columns(pss[q], Vs[q], select[q], probs[q][1])
    info, V, nvec, cnts, st, _ = raw_host(eng, pss, select)
    assert info == 0 and nvec == [7, 0, 7] and np.all(V[1] == 0)
    # nothing selected anywhere: no solve is launched
    none = eng.eigvecs_batch(pss, np.zeros(7, dtype=bool))
    assert all(V.shape == (7, 0) for Vq in none for V in Vq)
    assert eng.eigvecs_batch_stats.nlaunch == 0 and eng.eigvecs_batch_stats.nvec_total == 0
    info, V, nvec, cnts, st, _ = raw_host(eng, pss, np.zeros(7, dtype=bool), maxvec=2)
    assert info == 0 and nvec == [0, 0, 0] and st.nlaunch == 0 and np.all(V == 0)


# ------------------------------------------------------------------------------------------------
# 7. launch count
def case_launch_count(eng):
    """the launches of a call depend neither on nb nor on n (below the cap)"""
    base = _shared("launch", lambda: [plain_form(12, 3, SEEDS[k], [(), (3,), (7,), (0, 9), (5,)][k]) for k in range(5)])
    counts = {}
    for nb in (3, 40):
        probs = [base[q % 5] for q in range(nb)]
        check_batch(eng, probs, np.ones(12, dtype=bool))
        counts[nb] = eng.eigvecs_batch_stats.nlaunch
    check_batch(eng, depth_problems(), np.ones(40, dtype=bool))
    deep = eng.eigvecs_batch_stats.nlaunch
    assert counts[3] == counts[40] == deep and deep > 0, (counts, deep)
    assert eng.eigvecs_batch_stats.ngroups == 1


# ------------------------------------------------------------------------------------------------
# 8. above the cap
def case_above_cap(eng):
    n, p = bev_nmax() + 1, 2
    rs = np.random.RandomState(13)
    diag = [np.linspace(0.6, 1.9, n) * (1 + 0.2 * rs.rand(n)) for _ in range(p)]
    probs = _shared(("cap", n), lambda: [vc.schur_form(n, p, diag, seed=s, pairs=(5, 23, n - 3)) for s in (17, 7)])
    select = np.zeros((2, n), dtype=bool)
    select[0] = np.arange(n) % 4 == 1  # (with the first pair and the last; nvec differs: the staging into n x maxvec blocks)
    select[1] = np.arange(n) % 8 == 0
    check_batch(eng, probs, select)


# ------------------------------------------------------------------------------------------------
# 9. pipeline, device-resident (GPU tier)
def case_pipeline(eng, lr):
    import torch

    n, p, nb = 12, 3, 5
    facs = [pt.bench_factors(n, p, seed=91 + q) for q in range(nb)]
    dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in facs])).cuda()
    T, Z, values, _ = eng.pschur_batch_(dA, lr)
    si = p if lr == "L" else 1
    select = np.ones((nb, n), dtype=bool)
    select[1] = np.arange(n) % 2 == 0
    V, nvec = eng.eigvecs_batch(T, Z, values, select, lr=lr, schurindex=si)
    assert V.is_cuda and tuple(V.shape) == (nb, p, n, int(max(nvec)))
    Vh, Th, Zh = V.cpu().numpy(), T.cpu().numpy(), Z.cpu().numpy()
    for q in range(nb):
        ps = psd_amd.PeriodicSchur([np.asfortranarray(Th[q, l]) for l in range(p)],
                                   [np.asfortranarray(Zh[q, l]) for l in range(p)], values[q], lr, si)
        Vs = [Vh[q, l][:, :nvec[q]] for l in range(p)]
        assert np.all(Vh[q][:, :, nvec[q]:] == 0)
        lams = vc.order_values(ps, select[q])
        assert Vs[0].shape[1] == len(lams)
        vc.ec.ev_check(facs[q], Vs, lams, left=(lr == "L"))
        r = vc.relation_ratio(facs[q], Vs, lams, left=(lr == "L"))
        assert r <= vc.GATE, (lr, q, r)
        single = eng.eigvecs_dev(T[q].transpose(1, 2).contiguous(), Z[q].transpose(1, 2).contiguous(), values[q],
                                 select[q], lr=lr, schurindex=si)
        for l in range(p):
            assert np.allclose(Vs[l], single[l].cpu().numpy(), rtol=0, atol=1e-9), (lr, q, l)
    V1, nvec1 = eng.eigvecs_batch(T, Z, values, select, lr=lr, schurindex=si, shifted=False)
    assert tuple(V1.shape) == (nb, 1, n, int(max(nvec))) and torch.equal(V1[:, 0], V[:, 0])
    assert nvec1.tolist() == nvec.tolist()


# ------------------------------------------------------------------------------------------------
# 10. errors
def case_errors(eng, make_engine):
    probs = mixed_problems()
    pss = [ps for ps, _ in probs]
    n, p = 7, 3
    with pytest.raises(ValueError, match="argument 9"):
        eng.eigvecs_batch(pss, [True] * (n - 1))
    with pytest.raises(ValueError, match="argument 9"):
        eng.eigvecs_batch(pss, np.ones((4, n), dtype=bool))
    bad = vc._clone(pss[1])
    bad.schurindex = p + 1
    with pytest.raises(ValueError, match="argument 8"):
        eng.eigvecs_batch([bad, bad], [True] * n)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.eigvecs_batch([pss[0], plain_form(6, p, 5)[0]], [True] * n)  # unequal order
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.eigvecs_batch([pss[0], plain_form(n, 2, 5)[0]], [True] * n)  # unequal period
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.eigvecs_batch([pss[0], bad], [True] * n)  # unequal schurindex
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.eigvecs_batch([vc.schur_form(n, p, [np.linspace(1.0, 2.0, n)] * p, seed=5, cplx=True)[0]], [True] * n)
    g = psd_amd.GeneralizedPeriodicSchur([True, False, True], pss[0].Ts, pss[0].Z, np.array(pss[0].values), np.ones(n),
                                         np.zeros(n, dtype=np.int32), "L", p)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.eigvecs_batch([pss[0], g], [True] * n)
    bad = vc._clone(pss[0])
    bad.Z = [z.astype(np.complex128) for z in bad.Z]
    with pytest.raises(TypeError):
        eng.eigvecs_batch([bad], [True] * n)
    bad = vc._clone(pss[0])
    bad.Z = []
    with pytest.raises(ValueError):
        eng.eigvecs_batch([bad], [True] * n)
    assert eng.eigvecs_batch([], [True] * n) == []
    info, V, nvec, _, _, _ = raw_host(eng, pss, MIXED_SELECT, maxvec=6)  # problem 0 has 7 columns
    assert info == -10 and nvec == MIXED_NVEC
    sharded = make_engine()
    sharded.set_shard(0, 2)
    with pytest.raises(psd_amd.NotImplementedPSD):
        sharded.eigvecs_batch(pss, [True] * n)


def case_dev_abi(eng):
    """psd_d_eigvecs_batch_dev through the C ABI on packed blocks (in the simulation device memory is host memory): the
    same bits as the host entry, and the argument codes of both entries."""
    probs = mixed_problems()
    pss = [ps for ps, _ in probs]
    nb, n, p = 5, 7, 3
    host = eng.eigvecs_batch(pss, MIXED_SELECT)
    dT = np.ascontiguousarray(np.array([pt.pack(ps.Ts) for ps in pss]))
    dZ = np.ascontiguousarray(np.array([pt.pack(ps.Z) for ps in pss]))
    vals = np.array([np.asarray(ps.values, dtype=complex) for ps in pss])
    wr, wi = np.ascontiguousarray(vals.real), np.ascontiguousarray(vals.imag)
    sel = np.ascontiguousarray(MIXED_SELECT, dtype=np.uint8)
    dp, u8p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    nvec = (C.c_int * nb)()
    cnts = np.zeros((nb, 3), dtype=np.int32)
    st = psd_amd.BevecStats()
    info = C.c_int(0)
    lib, ctx = eng.lib, eng.ctx
    wrp, wip, selp = wr.ctypes.data_as(dp), wi.ctypes.data_as(dp), sel.ctypes.data_as(u8p)
    bT, bZ = C.c_void_p(dT.ctypes.data), C.c_void_p(dZ.ctypes.data)
    rc = lib.psd_d_eigvecs_batch_dev(ctx, nb, n, p, bT, bZ, wrp, wip, b"L", p, selp, 1, None, 0, nvec,
                                     cnts.ctypes.data_as(i32p), C.byref(st), C.byref(info))
    assert rc == 0 and list(nvec) == MIXED_NVEC
    V = np.full((nb, p, 7, n), 7.0 + 7.0j)
    rc = lib.psd_d_eigvecs_batch_dev(ctx, nb, n, p, bT, bZ, wrp, wip, b"L", p, selp, 1, C.c_void_p(V.ctypes.data), 7,
                                     nvec, cnts.ctypes.data_as(i32p), C.byref(st), C.byref(info))
    assert rc == 0 and info.value == 0 and st.nb == nb and st.ngroups == 1 and st.nlaunch == 5
    assert st.ms_kernels >= st.ms_solve >= 0
    for q in range(nb):
        for l in range(p):
            assert np.array_equal(V[q, l, :nvec[q]].T, host[q][l]) and np.all(V[q, l, nvec[q]:] == 0)
    assert all(np.array_equal(dT[q], pt.pack(pss[q].Ts)) for q in range(nb))  # the inputs stay as they were

    def dev_(c_=ctx, nb_=nb, n_=n, p_=p, T_=bT, Z_=bZ, wr_=wrp, o=b"L", si=p, sel_=selp, V_=None, mv=0, nv=nvec):
        return lib.psd_d_eigvecs_batch_dev(c_, nb_, n_, p_, T_, Z_, wr_, wip, o, si, sel_, 1, V_, mv, nv, None, None, None)

    Tp = eng._ptrs([np.asfortranarray(t, dtype=np.float64) for ps in pss for t in ps.Ts])
    Zp = eng._ptrs([np.asfortranarray(z, dtype=np.float64) for ps in pss for z in ps.Z])

    def host_(c_=ctx, nb_=nb, n_=n, p_=p, T_=Tp, Z_=Zp, wr_=wrp, o=b"L", si=p, sel_=selp, V_=None, mv=0, nv=nvec):
        return lib.psd_d_eigvecs_batch(c_, nb_, n_, p_, T_, Z_, wr_, wip, o, si, sel_, 1, V_, mv, nv, None, None, None)

    for f in (dev_, host_):
        assert f() == 0
        assert f(c_=None) == -1 and f(n_=0) == -2 and f(p_=0) == -3 and f(T_=None) == -4 and f(Z_=None) == -5
        assert f(wr_=None) == -6 and f(o=b"X") == -7 and f(si=0) == -8 and f(si=p + 1) == -8 and f(sel_=None) == -9
        assert f(nb_=-1) == -11 and f(nv=None) == -12
        assert f(nb_=0, T_=None, Z_=None, sel_=None, nv=None) == 0  # nb == 0 touches nothing
    assert dev_(V_=C.c_void_p(V.ctypes.data), mv=6) == -10
