"""Case bodies of the batched verifier (checkpsd_batch; csrc/psd_bcheck.h, psd_bcheck_host.inl): one body for all four
batch families, shared by the CPU tier (the serial simulation) and the GPU tier.

The inputs are synthetic decompositions built on the host, no pschur call: Z_l the Q factor of a seeded Gaussian matrix,
T_l = triu(Gaussian) / sqrt(n) (real families: the factor at schurindex carries sub-diagonal entries 0.3 at rows j + 1,
j = 0, 3, 6, ...), schurindex 1 for 'R' and p for 'L', and A_l = Z_a T_l Z_b' formed in extended precision and rounded
(formed in float64, numpy would reproduce it exactly and the reference error would be 0).  The references are
psdtest.checkpsd, the numpy restatement of the reference's checkpsd, and the norms as engine_cases forms them; the
tolerances are those of engine_cases.case_checkpsd."""
import ctypes as C

import numpy as np
import pytest

import batch_common as bc
import psd_amd
import psdtest as pt
from batch_common import T
from engine_cases import _checkpsd_numpy_details

# the two entries per element type serve the signed families too: the signature is an argument
D = bc.D
Z = bc.Z
ZG = bc.ZG.with_(csym="psd_z_")
DG = bc.DG.with_(csym="psd_d_")
FAMILIES = [D, Z, ZG, DG]

# the tile and period edges: one element, below / at / above one tile, three tiles with a partial one, the cap
SHAPES = [(5, 1, 1), (3, 3, 2), (4, 15, 3), (4, 16, 2), (4, 17, 3), (3, 33, 2), (2, 48, 5), (2, 64, 2)]
DAMAGE_SHAPE = (6, 17, 3)
INDEP_SHAPE = (7, 17, 3)
FALLBACK_SHAPE = (3, 17, 2)
ABOVE_CAP_SHAPE = (2, 65, 2)
CHAIN_SHAPE = (8, 24, 3)
KNOBS = ("PSD_BATCH_GROUP", "PSD_BCK_NMAX")


def shape_id(s):
    return bc.shape_id(s)


def signature(fam, p, lr):
    """None for the plain families; S = [T] + [q even] for the signed ones, reversed for 'L'"""
    if not fam.signed:
        return None
    return bc.sig((0, 0, p, [T] + [q % 2 == 0 for q in range(1, p)]), lr)


def _gauss(fam, seed, stream, n):
    if fam.cplx:
        g = pt.randn_counter(seed, stream, 2 * n * n)
        return (g[: n * n] + 1j * g[n * n:]).reshape(n, n)
    return pt.randn_counter(seed, stream, n * n).reshape(n, n)


def form_A(fam, Ts, Zs, lr, S):
    """A_l = Z_a T_l Z_b' (diagnostics.jl:249-253) in extended precision, rounded to working precision"""
    p = len(Ts)
    wide = np.clongdouble if fam.cplx else np.longdouble
    S = [True] * p if S is None else S
    out = []
    for l in range(p):
        l1 = (l + 1) % p
        a, b = (l, l1) if S[l] != (lr == "L") else (l1, l)
        out.append(np.asfortranarray((Zs[a].astype(wide) @ Ts[l].astype(wide) @ Zs[b].astype(wide).conj().T).astype(fam.dtype)))
    return out


def decomposition(fam, Ts, Zs, lr, S):
    n, p = Ts[0].shape[0], len(Ts)
    si = p if lr == "L" else 1
    if S is None:
        return psd_amd.PeriodicSchur(Ts, Zs, np.zeros(n, dtype=np.complex128), lr, si)
    return psd_amd.GeneralizedPeriodicSchur(S, Ts, Zs, np.zeros(n, dtype=np.complex128), np.ones(n),
                                            np.zeros(n, dtype=np.int32), lr, si)


def synth_one(fam, n, p, lr, S, seed, extra_sub=False):
    si = p if lr == "L" else 1
    Zs = [np.asfortranarray(np.linalg.qr(_gauss(fam, seed, l, n))[0].astype(fam.dtype)) for l in range(p)]
    Ts = [np.asfortranarray((np.triu(_gauss(fam, seed, p + l, n)) / np.sqrt(n)).astype(fam.dtype)) for l in range(p)]
    if not fam.cplx:
        for j in range(0, n - 1, 3):
            Ts[si - 1][j + 1, j] = 0.3
        if extra_sub and n > 2:
            Ts[si - 1][2, 1] = 0.25
    return decomposition(fam, Ts, Zs, lr, S), form_A(fam, Ts, Zs, lr, S)


def batch(fam, shape, lr):
    """(S, Ps, As_list) of a shape, built once and read-only"""
    nb, n, p = shape[:3]
    S = signature(fam, p, lr)

    def make():
        probs = [synth_one(fam, n, p, lr, S, 4000 + 131 * n + 17 * p + q) for q in range(nb)]
        for ps, As in probs:
            for m in list(ps.Ts) + list(ps.Z) + As:
                m.setflags(write=False)
        return probs

    probs = bc.cached(("check", fam.name, nb, n, p, lr), make)
    return S, [pr[0] for pr in probs], [pr[1] for pr in probs]


def clone(fam, ps, As):
    return (decomposition(fam, [t.copy(order="F") for t in ps.Ts], [z.copy(order="F") for z in ps.Z], ps.orientation,
                          getattr(ps, "S", None)), [a.copy(order="F") for a in As])


def reference(Ps, As_list, S, thresh=100, strict=True):
    """(ok, err, orth, tri) per problem from the numpy restatement of the reference"""
    ok, err, orth, tri = [], [], [], []
    for ps, As in zip(Ps, As_list):
        o, e = pt.checkpsd(ps, As, thresh=thresh, strict=strict, S=S)
        r, t = _checkpsd_numpy_details(ps, As, S)
        ok.append(o), err.append(e), orth.append(r), tri.append(t)
    return np.array(ok), np.array(err), np.array(orth), np.array(tri)


def within(n, got, ref, what):
    """the tolerances of engine_cases.case_checkpsd, for every problem of the batch"""
    ok, err, orth, tri = got
    ok_ref, err_ref, orth_ref, tri_ref = ref
    print(what, "err", err.max(), "err_ref", err_ref.max(), "orth", orth.max(), "orth_ref", orth_ref.max())
    assert np.array_equal(ok, ok_ref), (what, ok, ok_ref, err, err_ref)
    assert np.all(np.abs(err - err_ref) <= 0.25 * err_ref + 2.0), (what, err, err_ref)
    assert np.all(np.abs(orth - orth_ref) <= 0.5 * orth_ref + 4 * pt.EPS * np.sqrt(n)), (what, orth, orth_ref)
    assert np.all(tri == tri_ref), (what, tri, tri_ref)


# ---- 1, 2: against the reference restatement and against the single entry ---------------------------------------------
def case_reference(eng, fam, shape, lr):
    nb, n, p = shape[:3]
    S, Ps, As_list = batch(fam, shape, lr)
    got = eng.checkpsd_batch(Ps, As_list, details=True)
    assert got[0].dtype == bool and got[0].shape == (nb,) and all(x.shape == (nb, p) for x in got[1:])
    assert np.all(got[0]), (fam, shape, lr, got)
    within(n, got, reference(Ps, As_list, S), (fam, shape, lr))
    ok2, err2 = eng.checkpsd_batch(Ps, As_list)
    assert np.array_equal(ok2, got[0]) and np.array_equal(err2, got[1])
    st = eng.checkpsd_batch_stats
    assert (st.nb, st.nfail, st.ngroups, st.nlaunch) == (nb, 0, 1, 1)


def case_single(eng, fam, shape, lr):
    nb, n, p = shape[:3]
    S, Ps, As_list = batch(fam, shape, lr)
    got = eng.checkpsd_batch(Ps, As_list, details=True)
    single = [eng.checkpsd(ps, As, S=S, details=True) for ps, As in zip(Ps, As_list)]
    # (two summation orders: the numbers agree as they agree with the reference, not bit for bit)
    within(n, got, tuple(np.array([s[k] for s in single]) for k in range(4)), (fam, shape, lr, "single"))


# ---- 3: it has to say no, to the right problem only -------------------------------------------------------------------
def damaged(fam, lr, nan=False):
    """the DAMAGE_SHAPE batch with problems 1 .. 5 damaged, each in its own way (a) - (e); `nan`: only a NaN in one Z
    entry of problem 5"""
    nb, n, p = DAMAGE_SHAPE
    S, Ps, As_list = batch(fam, DAMAGE_SHAPE, lr)
    work = [clone(fam, ps, As) for ps, As in zip(Ps, As_list)]
    si = p if lr == "L" else 1
    j = p // 2
    if nan:
        work[5][0].Z[1][3, 2] = np.nan
        return S, [w[0] for w in work], [w[1] for w in work]
    work[1][0].Ts[j][n - 1, 0] = 1e-3                                 # (a)
    work[2][0].Z[0] = np.asfortranarray(work[2][0].Z[0] * (1 + 1e-9))  # (b)
    work[3][0].Ts[0][0, n - 1] += 1e-6                                # (c)
    if fam.cplx:
        work[5][0].Ts[si - 1][2, 1] = 0.25                            # (e) complex: a sub-diagonal entry is damage
    else:
        work[4][0].Ts[si % p][1, 0] = 1e-3                            # (d) below the diagonal of a triangular factor
        # (e) real: a sub-diagonal entry of the quasi-triangular factor belongs to a valid form (with its own A)
        work[5] = synth_one(fam, n, p, lr, S, 4000 + 131 * n + 17 * p + 5, extra_sub=True)
    return S, [w[0] for w in work], [w[1] for w in work]


def case_says_no(eng, fam, lr, check=None):
    """`check(Ps, As_list, **kw)`: the call under test (default: the batch method of eng)"""
    nb, n, p = DAMAGE_SHAPE
    check = check or (lambda Ps, As, **kw: eng.checkpsd_batch(Ps, As, details=True, **kw))
    S, Ps0, As0 = batch(fam, DAMAGE_SHAPE, lr)
    clean = check(Ps0, As0)
    assert np.all(clean[0])
    S, Ps, As_list = damaged(fam, lr)
    ok, err, orth, tri = got = check(Ps, As_list)
    j = p // 2
    assert not ok[1] and abs(tri[1, j] - 1e-3) < 1e-12, (ok, tri[1])
    assert not check(Ps, As_list, strict=False, thresh=1e9)[0][1]  # 1e-3 is far above 10 eps n as well
    assert not ok[2] and orth[2, 0] > 10 * pt.EPS * n
    assert not ok[3]
    for q in (2, 3):
        ok_ref, err_ref = pt.checkpsd(Ps[q], As_list[q], S=S)
        assert not ok_ref and np.allclose(err[q], err_ref, rtol=1e-3, atol=2.0), (q, err[q], err_ref)
    if fam.cplx:
        assert ok[4] and not ok[5] and tri[5, (p if lr == "L" else 1) - 1] == 0.25
        same = (0, 4)
    else:
        assert not ok[4] and abs(tri[4, (p if lr == "L" else 1) % p] - 1e-3) < 1e-12
        assert ok[5] and np.all(tri[5] == 0.0)  # (e)
        ok5, err5 = pt.checkpsd(Ps[5], As_list[5], S=S)
        assert ok5 and np.all(np.abs(err[5] - err5) <= 0.25 * err5 + 2.0)
        same = (0,)
    for q in same:  # the undamaged problems: the clean batch's numbers, bit for bit
        for k in range(4):
            assert np.array_equal(got[k][q], clean[k][q]), (q, k)
    return clean


def case_nan(eng, fam, lr):
    """(f) a NaN in one Z entry: false through the !(e <= thresh) rule, as the single entry says"""
    S, Ps0, As0 = batch(fam, DAMAGE_SHAPE, lr)
    clean = eng.checkpsd_batch(Ps0, As0, details=True)
    S, Ps, As_list = damaged(fam, lr, nan=True)
    got = eng.checkpsd_batch(Ps, As_list, details=True)
    assert not got[0][5] and np.all(got[0][:5])
    assert not eng.checkpsd(Ps[5], As_list[5], S=S)[0]
    assert eng.checkpsd_batch_stats.nfail == 1
    for q in range(5):
        for k in range(4):
            assert np.array_equal(got[k][q], clean[k][q]), (q, k)


# ---- 4: independence, bit for bit ---------------------------------------------------------------------------------------
def case_independence(make_engine, fam, lr):
    nb, n, p = INDEP_SHAPE
    S, Ps, As_list = batch(fam, INDEP_SHAPE, lr)
    eng, grouped = make_engine({}), make_engine({"PSD_BATCH_GROUP": "3"})
    base = eng.checkpsd_batch(Ps, As_list, details=True)
    assert (eng.checkpsd_batch_stats.ngroups, eng.checkpsd_batch_stats.nlaunch) == (1, 1)
    got = grouped.checkpsd_batch(Ps, As_list, details=True)
    assert (grouped.checkpsd_batch_stats.ngroups, grouped.checkpsd_batch_stats.nlaunch) == (3, 3)
    rev = eng.checkpsd_batch(Ps[::-1], As_list[::-1], details=True)
    for k in range(4):
        assert np.array_equal(got[k], base[k]), ("grouped", k)
        assert np.array_equal(rev[k], base[k][::-1]), ("reversed", k)
    for q in range(nb):
        one = eng.checkpsd_batch([Ps[q]], [As_list[q]], details=True)
        for k in range(4):
            assert np.array_equal(one[k][0], base[k][q]), ("alone", q, k)


# ---- 5: above the cap ---------------------------------------------------------------------------------------------------
def case_fallback(make_engine, fam, lr):
    """an engine whose cap is 16: the single verifier on the slices of the batch"""
    nb, n, p = FALLBACK_SHAPE
    low = make_engine({"PSD_BCK_NMAX": "16"})
    S, Ps, As_list = batch(fam, FALLBACK_SHAPE, lr)
    got = low.checkpsd_batch(Ps, As_list, details=True)
    st = low.checkpsd_batch_stats
    assert st.nlaunch > st.ngroups == 1 and st.nfail == 0
    within(n, got, reference(Ps, As_list, S), (fam, "fallback", lr))
    # the verdicts on damaged inputs: (a) - (c) of case_says_no in a batch of this shape
    work = [clone(fam, ps, As) for ps, As in zip(Ps, As_list)]
    work[0][0].Ts[p // 2][n - 1, 0] = 1e-3
    work[1][0].Z[0] = np.asfortranarray(work[1][0].Z[0] * (1 + 1e-9))
    work[2][0].Ts[0][0, n - 1] += 1e-6
    ok, err, orth, tri = low.checkpsd_batch([w[0] for w in work], [w[1] for w in work], details=True)
    assert not ok.any() and abs(tri[0, p // 2] - 1e-3) < 1e-12 and orth[1, 0] > 10 * pt.EPS * n
    assert low.checkpsd_batch_stats.nfail == nb
    assert not low.checkpsd_batch([w[0] for w in work], [w[1] for w in work], strict=False, thresh=1e9)[0][0]
    for q in (1, 2):
        ok_ref, err_ref = pt.checkpsd(work[q][0], work[q][1], S=S)
        assert not ok_ref and np.allclose(err[q], err_ref, rtol=1e-3, atol=2.0)


def case_above_default_cap(eng, fam):
    nb, n, p = ABOVE_CAP_SHAPE
    assert n == bc.cap("psd_bcheck.h", "PSD_BCK_NMAX") + 1
    S, Ps, As_list = batch(fam, ABOVE_CAP_SHAPE, "R")
    got = eng.checkpsd_batch(Ps, As_list, details=True)
    assert eng.checkpsd_batch_stats.nlaunch > eng.checkpsd_batch_stats.ngroups
    within(n, got, reference(Ps, As_list, S), (fam, "above the cap"))


def case_cap_knob(make_engine):
    """PSD_BCK_NMAX may only lower the cap: a value above 64 or below 1 leaves it at 64"""
    cap = bc.cap("psd_bcheck.h", "PSD_BCK_NMAX")
    assert cap == 64
    S, Ps, As_list = batch(D, SHAPES[-1], "R")
    S1, Ps1, As1 = batch(D, ABOVE_CAP_SHAPE, "R")
    assert SHAPES[-1][1] == cap
    for value in ("65", "128", "0", "-3"):
        eng = make_engine({"PSD_BCK_NMAX": value})
        assert np.all(eng.checkpsd_batch(Ps, As_list)[0])
        assert eng.checkpsd_batch_stats.nlaunch == eng.checkpsd_batch_stats.ngroups == 1, value
        assert np.all(eng.checkpsd_batch(Ps1, As1)[0])
        assert eng.checkpsd_batch_stats.nlaunch > eng.checkpsd_batch_stats.ngroups, value


# ---- 6: ABI ---------------------------------------------------------------------------------------------------------------
def case_abi(eng, fam, dev=None):
    """every code of the table through the C entries; `dev`: packs a list of matrices into a device block and returns
    (pointer, keep-alive) — the device entry is exercised with it"""
    nb, n, p = 3, 5, 2
    lr = "R"
    S, Ps, As_list = batch(fam, (nb, n, p), lr)
    Tm = [np.array(t, order="F") for ps in Ps for t in ps.Ts]
    Zm = [np.array(z, order="F") for ps in Ps for z in ps.Z]
    Am = [np.array(a, order="F") for As in As_list for a in As]
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    ptrs = psd_amd.Engine._ptrs
    if dev is None:
        entry, keep = fam.entry(eng, "checkpsd_batch"), None
        mats = [ptrs(Tm), ptrs(Zm), ptrs(Am)]
    else:
        entry = fam.entry(eng, "checkpsd_batch_dev")
        packed = [dev(M) for M in (Tm, Zm, Am)]
        mats, keep = [C.c_void_p(x[0]) for x in packed], packed
    sarr = bc.sarr(S) if S is not None else None

    def call(ctx=eng.ctx, nb=nb, n=n, p=p, mats=mats, orient=b"R", si=1, thresh=100.0, strict=1, err=True, orth=True,
             tri=True, ok=True, stats=True, nbrows=nb):
        out = {"err": np.full((nbrows, max(p, 1)), -7.0), "orth": np.full((nbrows, max(p, 1)), -7.0),
               "tri": np.full((nbrows, max(p, 1)), -7.0), "ok": np.full(nbrows, -7, dtype=np.int32),
               "stats": psd_amd.BcheckStats(), "info": C.c_int(99)}
        out["stats"].nb = -7
        rc = entry(ctx, nb, n, p, mats[0], mats[1], mats[2], sarr, orient, si, thresh, strict,
                   out["err"].ctypes.data_as(dp) if err else None, out["orth"].ctypes.data_as(dp) if orth else None,
                   out["tri"].ctypes.data_as(dp) if tri else None, out["ok"].ctypes.data_as(i32p) if ok else None,
                   C.byref(out["stats"]) if stats else None, C.byref(out["info"]))
        assert rc == out["info"].value
        return rc, out

    assert call(ctx=None)[0] == -1
    assert call(nb=-1)[0] == -2
    assert call(n=0)[0] == -3
    assert call(p=0)[0] == -4
    for k in range(3):
        assert call(mats=[None if j == k else m for j, m in enumerate(mats)])[0] == -5
    assert call(orient=b"X")[0] == -8
    assert call(si=0)[0] == -9 and call(si=p + 1)[0] == -9
    assert call(err=False)[0] == -13
    # the order of the checks: the first wrong argument names the code
    assert call(nb=-1, n=0)[0] == -2 and call(n=0, p=0)[0] == -3 and call(orient=b"X", si=0)[0] == -8
    # nb == 0: nothing is touched (the stats, as in every batch entry, are zeroed at the head of the call)
    rc, out = call(nb=0)
    assert rc == 0
    assert np.all(out["err"] == -7.0) and np.all(out["orth"] == -7.0) and np.all(out["tri"] == -7.0)
    assert np.all(out["ok"] == -7) and out["stats"].nlaunch == 0 and out["stats"].ngroups == 0
    assert call(nb=0, mats=[None, None, None], err=False)[0] == 0
    # a full call, and each optional output left out
    rc, full = call()
    assert rc == 0 and np.all(full["ok"] == 1) and full["stats"].nb == nb and full["stats"].nfail == 0
    assert full["stats"].nlaunch == 1 and full["stats"].ngroups == 1
    for leave in ("orth", "tri", "ok", "stats"):
        rc, out = call(**{leave: False})
        assert rc == 0 and np.array_equal(out["err"], full["err"])
        for name in ("orth", "tri", "ok"):
            assert np.array_equal(out[name], full[name]) if name != leave else np.all(out[name] == -7), (leave, name)
    info_null = entry(eng.ctx, nb, n, p, mats[0], mats[1], mats[2], sarr, b"R", 1, 100.0, 1, full["err"].ctypes.data_as(dp),
                      None, None, None, None, None)
    assert info_null == 0
    # a failed check is a verdict: 0, with the problem counted
    rc, out = call(thresh=0.0)
    assert rc == 0 and not out["ok"].any() and out["stats"].nfail == nb
    del keep


def case_python_errors(eng):
    nb, n, p = 3, 5, 2
    S, Ps, As_list = batch(D, (nb, n, p), "R")
    DM = psd_amd.DimensionMismatch
    with pytest.raises(DM, match="length of Hs vector must match period of P"):
        eng.checkpsd_batch(Ps, [As_list[0], As_list[1][:1], As_list[2]])
    with pytest.raises(DM, match="size of Hs matrices must match P"):
        eng.checkpsd_batch(Ps, [As_list[0], [a[:4, :4] for a in As_list[1]], As_list[2]])
    with pytest.raises(DM, match="equal order and period"):
        S4, Ps4, As4 = batch(D, (3, 3, 2), "R")
        eng.checkpsd_batch([Ps[0], Ps4[0]], [As_list[0], As4[0]])
    with pytest.raises(DM, match="equal order and period"):
        S3, Ps3, As3 = batch(D, (4, 5, 3), "R")
        eng.checkpsd_batch([Ps[0], Ps3[0]], [As_list[0], As3[0]])
    with pytest.raises(DM):  # orientation (the schurindex of a period 2 differs with it)
        SL, PsL, AsL = batch(D, (nb, n, p), "L")
        eng.checkpsd_batch([Ps[0], PsL[0]], [As_list[0], AsL[0]])
    with pytest.raises(DM):
        eng.checkpsd_batch(Ps, As_list[:2])
    with pytest.raises(TypeError, match="all real or all complex"):
        Sz, Psz, Asz = batch(Z, (nb, n, p), "R")
        eng.checkpsd_batch([Ps[0], Psz[0]], [As_list[0], Asz[0]])
    with pytest.raises(DM, match="equal signatures"):
        Sg, Psg, Asg = batch(DG, (nb, n, p), "R")
        eng.checkpsd_batch([Psg[0], Ps[0]], [Asg[0], As_list[0]])
    with pytest.raises(DM, match="length of S"):
        eng.checkpsd_batch(Ps, As_list, S=[True])
    with pytest.raises(TypeError):
        eng.checkpsd_batch(Ps)
    # an explicit signature takes the place of the decompositions', as in checkpsd
    Sg, Psg, Asg = batch(DG, (nb, n, p), "R")
    ok_wrong, _ = eng.checkpsd_batch(Psg, Asg, S=[True] * p)
    assert np.array_equal(ok_wrong, [eng.checkpsd(ps, As, S=[True] * p)[0] for ps, As in zip(Psg, Asg)])
    # nb = 0
    eng.checkpsd_batch_stats = None
    ok, err = eng.checkpsd_batch([], [])
    assert ok.shape == (0,) and ok.dtype == bool and err.shape == (0, 0)
    assert len(eng.checkpsd_batch([], [], details=True)) == 4 and eng.checkpsd_batch_stats.nlaunch == 0


# ---- 7: the complex twin of the single device entry ---------------------------------------------------------------------
def case_zcheckpsd_dev(eng, n, dev):
    """psd_z_checkpsd_dev / checkpsd_dev(cplx=True) against psd_z_checkpsd on the same operands; `dev` as in case_abi"""
    p = 3
    for fam, lr in ((Z, "R"), (ZG, "L")):
        S, Ps, As_list = batch(fam, (1, n, p), lr)
        ps, As = Ps[0], As_list[0]
        host = eng.checkpsd(ps, As, S=S, details=True)
        packed = [dev(M) for M in (ps.Ts, ps.Z, As)]
        got = eng.checkpsd_dev(packed[0][0], packed[1][0], packed[2][0], n, p, lr, ps.schurindex, S=S, cplx=True)
        assert got[0] == host[0] and got[0]
        assert n <= 64  # (one tile per launch: the same sums in the same order, so the same bits)
        for k in range(1, 4):
            assert np.array_equal(got[k], host[k]), (n, lr, k)
        bad = [np.array(t, order="F") for t in ps.Ts]
        bad[0][0, n - 1] += 1e-6
        pk = dev(bad)
        assert not eng.checkpsd_dev(pk[0], packed[1][0], packed[2][0], n, p, lr, ps.schurindex, S=S, cplx=True)[0]
    # the real entry is what it was
    S, Ps, As_list = batch(D, (1, n, p), "R")
    packed = [dev(M) for M in (Ps[0].Ts, Ps[0].Z, As_list[0])]
    got = eng.checkpsd_dev(packed[0][0], packed[1][0], packed[2][0], n, p, "R", 1)
    host = eng.checkpsd(Ps[0], As_list[0], details=True)
    assert got[0] == host[0] and all(np.array_equal(got[k], host[k]) for k in range(1, 4))
    info = C.c_int(5)
    assert eng.lib.psd_z_checkpsd_dev(eng.ctx, n, p, None, None, None, None, b"R", 1, 100.0, 1, None, None, None, None,
                                      C.byref(info)) == -4 and info.value == -4


def host_dev(mats):
    """the serial simulation's "device" memory is host memory: a packed [len][n][n] column-major block"""
    block = pt.pack(mats, dtype=mats[0].dtype)
    return block.ctypes.data, block


# ---- 8: the device-resident pipeline (GPU tier only) ----------------------------------------------------------------------
def case_device_chain(eng, fam, lr):
    import torch

    nb, n, p = CHAIN_SHAPE
    S = signature(fam, p, lr)
    si = p if lr == "L" else 1
    probs = bc.factors(fam.dtype, range(700, 700 + nb), n, p)
    dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in probs])).cuda()
    A = dA.clone()
    Tt, Zt, values, _ = fam.method(eng, "pschur_batch_")(dA, *fam.sargs(S), lr)
    keep = [x.clone() for x in (Tt, Zt, A)]
    thresh = 100 * np.sqrt(max(n / 32, 1))
    got = eng.checkpsd_batch(Tt, Zt, A, lr=lr, schurindex=si, S=S, thresh=thresh, details=True)
    st = eng.checkpsd_batch_stats
    assert (st.nb, st.nfail, st.ngroups, st.nlaunch) == (nb, 0, 1, 1)
    assert np.all(got[0]), got
    assert all(torch.equal(x, k) for x, k in zip((Tt, Zt, A), keep))
    Th, Zh = Tt.cpu().numpy(), Zt.cpu().numpy()
    Ps = [decomposition(fam, [np.asfortranarray(Th[q, j]) for j in range(p)],
                        [np.asfortranarray(Zh[q, j]) for j in range(p)], lr, S) for q in range(nb)]
    within(n, got, reference(Ps, probs, S, thresh=thresh), (fam, "chain", lr))
    # the host entry on the downloaded results: the same kernel on the same bits
    host = eng.checkpsd_batch(Ps, probs, thresh=thresh, details=True)
    for k in range(4):
        assert np.array_equal(host[k], got[k]), k
    # a layout that is not the entries' own is copied, and read all the same
    again = eng.checkpsd_batch(Tt.contiguous(), Zt.contiguous(), A.contiguous(), lr=lr, schurindex=si, S=S,
                               thresh=thresh, details=True)
    for k in range(4):
        assert np.array_equal(again[k], got[k]), k
    with pytest.raises(TypeError):
        other = torch.zeros_like(A, dtype=torch.float64 if fam.cplx else torch.complex128)
        eng.checkpsd_batch(Tt, Zt, other, lr=lr, schurindex=si, S=S)
    with pytest.raises(TypeError):
        eng.checkpsd_batch(Tt, Zt, lr=lr)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.checkpsd_batch(Tt, Zt, A[:, :, :, :5], lr=lr, schurindex=si, S=S)


def case_empty_device_batch(eng):
    import torch

    for dt in (torch.float64, torch.complex128):
        E = torch.zeros((0, 2, 3, 3), dtype=dt, device="cuda")
        eng.checkpsd_batch_stats = None
        ok, err = eng.checkpsd_batch(E, E.clone(), E.clone(), lr="L", schurindex=2)
        assert ok.shape == (0,) and ok.dtype == bool and err.shape == (0, 2)
        assert eng.checkpsd_batch_stats.nlaunch == 0
        assert [x.shape for x in eng.checkpsd_batch(E, E, E, details=True)] == [(0,), (0, 2), (0, 2), (0, 2)]
