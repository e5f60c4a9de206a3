"""Engine.eigvecs_batch / zeigvecs_batch with side="L" / "B" (psd_?_leigvecs_batch[_dev], csrc/psd_lbevec.h) and
Engine.eigcond_batch (psd_eigcond_batch[_dev]): left eigenvectors and eigenvalue condition numbers of many small periodic
Schur forms — the cases shared by the simulated tier (test_hostsim_leigvecs_batch.py) and the device tier
(test_gpu_leigvecs_batch.py).

Every problem goes through check_left: the left relation ratio <= evec_cases.GATE with mu from the caller's eigenvalue,
w_l' v_l constant over l, agreement with the numpy prototype evec_cases.backsub_ref run on the flip-adjoint form
(flip_adjoint below: T'_l = J T_l' J, Z'_l = Z_l J, eigenvalues conjugated and reversed, the opposite orientation) at its
atol, norm, phase and exact conjugate partners.  The inputs come from evec_cases.schur_form and bevec_cases.plain_form
with their seeds; an 'R' decomposition is the flip-adjoint of an 'L' form, taken as a decomposition of the factors A_l'."""
import ctypes as C

import numpy as np
import pytest

import bevec_cases as bc
import evec_cases as vc
import psd_amd
import psdtest as pt
from batch_common import cap

_cache = {}
SEEDS = bc.D.seeds


def _shared(key, make):
    """Inputs are built once, shared among the cases, and never written to."""
    if key not in _cache:
        out = make()
        for ps, As in out:
            for a in list(ps.Ts) + list(ps.Z) + list(As):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def flip_adjoint(ps):
    """the periodic Schur form of the adjoint factors: opposite orientation, same factor indexing and schurindex"""
    Ts = [np.asfortranarray(t.conj().T[::-1, ::-1]) for t in ps.Ts]
    Zs = [np.asfortranarray(z[:, ::-1]) for z in ps.Z]
    vals = np.conj(np.asarray(ps.values))[::-1] + 0.0  # (+ 0: a real eigenvalue keeps a positive zero imaginary part)
    return psd_amd.PeriodicSchur(Ts, Zs, vals, "R" if ps.orientation == "L" else "L", ps.schurindex)


def as_right(prob):
    """an 'R' decomposition (schurindex as the 'L' form's) for free: the flip-adjoint, of the factors A_l'"""
    ps, As = prob
    return flip_adjoint(ps), [np.asfortranarray(a.conj().T) for a in As]


def assemble(Ts, Zs, pairs=()):
    """(ps, As) of an 'L' form with schurindex len(Ts) from its factors, as evec_cases.schur_form assembles them"""
    p = len(Ts)
    vals = np.prod(np.array([np.diag(t) for t in Ts]), axis=0).astype(complex)
    for i in pairs:
        P = np.eye(2)
        for t in Ts:
            P = t[i:i + 2, i:i + 2] @ P
        ev = np.linalg.eigvals(P)
        vals[i], vals[i + 1] = ev[np.argmax(ev.imag)], ev[np.argmin(ev.imag)]
    As = [Zs[(l + 1) % p] @ Ts[l] @ Zs[l].conj().T for l in range(p)]
    return psd_amd.PeriodicSchur(Ts, Zs, vals, "L", p), As


def schur_form_si(n, p, seed, pairs, si):
    """bevec_cases.plain_form with the 2x2 blocks in T_si instead of T_p"""
    ps, _ = bc.plain_form(n, p, seed)
    Ts = [t.copy(order="F") for t in ps.Ts]
    t = Ts[si - 1]
    for i in pairs:
        t[i, i + 1], t[i + 1, i], t[i + 1, i + 1] = 0.7, -0.5, t[i, i]
    ps, As = assemble(Ts, [z.copy(order="F") for z in ps.Z], pairs)
    ps.schurindex = si
    return ps, As


def mu_of(lam, p):
    return complex(lam + 0j) ** (1.0 / p)


def left_ratio(ps, As, Ws, lams):
    """max over l and columns of ||w_a' A_l - mu w_b'|| / (||A_l||_F ||w_a||): (a, b) = (l + 1, l) for 'L', (l, l + 1)
    for 'R'"""
    p = len(As)
    worst = 0.0
    for k in range(Ws[0].shape[1]):
        mu = mu_of(lams[k], p)
        for l in range(p):
            a, b = ((l + 1) % p, l) if ps.orientation == "L" else (l, (l + 1) % p)
            wa, wb = Ws[a][:, k], Ws[b][:, k]
            worst = max(worst, np.linalg.norm(wa.conj() @ As[l] - mu * wb.conj())
                        / (np.linalg.norm(As[l]) * np.linalg.norm(wa)))
    return worst


def left_ref(ps, select):
    """the numpy prototype on the flip-adjoint form, its columns reversed back.  The prototype takes the principal root of
    the flipped eigenvalue, the entry the conjugate of the caller's root: they differ for a negative real eigenvalue.  Of
    a real problem the conjugated column is then the entry's; of a complex one the column belongs to another root and is
    not compared (returned in `skip`)."""
    real = not np.iscomplexobj(ps.Ts[0])
    ref = [r[:, ::-1] for r in vc.backsub_ref(flip_adjoint(ps), np.asarray(select, dtype=bool)[::-1])]
    lams = vc.order_values(ps, select)
    neg = [k for k, l in enumerate(lams) if l.imag == 0 and l.real < 0]
    if real:
        ref = [r.copy() for r in ref]
        for r in ref:
            r[:, neg] = np.conj(r[:, neg])
        neg = []
    return ref, neg


def check_left(ps, Ws, select, As, Vs=None):
    lams = vc.order_values(ps, select)
    p = len(As)
    assert len(Ws) == p and Ws[0].shape[1] == len(lams)
    r = left_ratio(ps, As, Ws, lams)
    assert r <= vc.GATE, r
    if Vs is not None:  # column j of W and of V belong to the same eigenvalue and root: w_l' v_l is one number
        assert Vs[0].shape == Ws[0].shape
        d = np.array([[np.vdot(Ws[l][:, k], Vs[l][:, k]) for k in range(len(lams))] for l in range(p)])
        assert np.all(np.abs(d - d[0]) <= 1e-9 * np.abs(d[0])), np.abs(d - d[0]).max()
    ref, skip = left_ref(ps, select)
    cols = [k for k in range(len(lams)) if k not in skip]
    for l in range(p):
        assert np.allclose(Ws[l][:, cols], ref[l][:, cols], rtol=0, atol=1e-9), (l, np.abs(Ws[l] - ref[l]).max())
    W1 = Ws[0]
    assert np.allclose(np.linalg.norm(W1, axis=0), 1.0, atol=1e-13)
    for c in range(W1.shape[1]):
        am = np.argmax(np.abs(W1[:, c]))
        assert W1[am, c].imag == 0 and W1[am, c].real > 0
    if not np.iscomplexobj(ps.Ts[0]):  # the partner of a pair is the exact conjugate
        for W in Ws:
            for c in range(len(lams) - 1):
                if lams[c].imag > 0:
                    assert np.array_equal(W[:, c + 1], np.conj(W[:, c]))
    return lams


def _call(eng, cplx):
    return eng.zeigvecs_batch if cplx else eng.eigvecs_batch


def check_batch(eng, probs, select, cplx=False):
    """side="B" on the batch: the right vectors through evec_cases.check_columns, the left ones through check_left"""
    pss = [ps for ps, _ in probs]
    nb, n = len(pss), pss[0].Ts[0].shape[0]
    keep = [[a.copy() for a in list(ps.Ts) + list(ps.Z)] for ps in pss]
    Vs, Ws = _call(eng, cplx)(pss, select, side="B")
    sel = np.broadcast_to(np.asarray(select, dtype=bool), (nb, n))
    assert len(Vs) == len(Ws) == nb
    for q, (ps, As) in enumerate(probs):
        vc.check_columns(ps, Vs[q], sel[q], As)
        check_left(ps, Ws[q], sel[q], As, Vs[q])
    assert all(np.array_equal(a, b) for ps, k in zip(pss, keep) for a, b in zip(list(ps.Ts) + list(ps.Z), k))
    return Vs, Ws


def _same(Va, Vb):
    return len(Va) == len(Vb) and all(np.array_equal(a, b) for a, b in zip(Va, Vb))


def raw_host(eng, pss, select, shifted=True, maxvec=None, cplx=False):
    """psd_d_leigvecs_batch / psd_z_leigvecs_batch through the C ABI: (info, W [nb][nmat][maxvec][n], nvec, counts, stats)"""
    nb, p, n = len(pss), len(pss[0].Ts), pss[0].Ts[0].shape[0]
    dt = np.complex128 if cplx else np.float64
    Ts = [np.asfortranarray(t, dtype=dt) for ps in pss for t in ps.Ts]
    Zs = [np.asfortranarray(z, dtype=dt) for ps in pss for z in ps.Z]
    vals = np.ascontiguousarray(np.array([np.asarray(ps.values, dtype=complex) for ps in pss]))
    dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    if cplx:
        beta = np.ones(vals.shape)
        ev = [vals.ctypes.data_as(dp), beta.ctypes.data_as(dp), None]
    else:
        wr, wi = np.ascontiguousarray(vals.real), np.ascontiguousarray(vals.imag)
        ev = [wr.ctypes.data_as(dp), wi.ctypes.data_as(dp)]
    sel = np.ascontiguousarray(np.broadcast_to(np.asarray(select, dtype=bool), (nb, n)), dtype=np.uint8)
    nvec = (C.c_int * nb)()
    cnts = np.zeros((nb, 3), dtype=np.int32)
    st = psd_amd.BevecStats()
    info = C.c_int(0)
    fn = eng.lib.psd_z_leigvecs_batch if cplx else eng.lib.psd_d_leigvecs_batch
    head = [eng.ctx, nb, n, p, eng._ptrs(Ts), eng._ptrs(Zs), *ev, pss[0].orientation.encode(), pss[0].schurindex,
            sel.ctypes.data_as(u8p), int(shifted)]
    tail = [nvec, cnts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st), C.byref(info)]
    fn(*head, None, 0, *tail)
    assert info.value == 0
    if maxvec is None:
        maxvec = max(nvec)
    nmat = p if shifted else 1
    W = np.full((nb, nmat, maxvec, n), 7.0 + 7.0j)  # (poisoned: the padding has to be written)
    Wp = (C.c_void_p * (nb * nmat))(*[W[q, l].ctypes.data for q in range(nb) for l in range(nmat)])
    rc = fn(*head, Wp, maxvec, *tail)
    assert rc == info.value
    return info.value, W, list(nvec), cnts, st


# ------------------------------------------------------------------------------------------------
# 1. mixed batch
def mixed_problems(cplx):
    return bc.mixed_problems(bc.Z) if cplx else bc.mixed_problems()


def case_mixed(eng, cplx):
    probs = mixed_problems(cplx)
    pss = [ps for ps, _ in probs]
    nvec0 = bc.Z.mixed_nvec if cplx else bc.D.mixed_nvec
    Vs, Ws = check_batch(eng, probs, bc.D.mixed_select, cplx)
    assert [W[0].shape[1] for W in Ws] == nvec0
    right = _call(eng, cplx)(pss, bc.D.mixed_select)
    right_launches = eng.eigvecs_batch_stats.nlaunch
    assert all(_same(a, b) for a, b in zip(right, Vs))  # the right vectors of "B" are those of the right call
    WL = _call(eng, cplx)(pss, bc.D.mixed_select, side="L")
    assert eng.eigvecs_batch_stats.nlaunch == right_launches + 2
    assert all(_same(a, b) for a, b in zip(WL, Ws))
    W1 = _call(eng, cplx)(pss, bc.D.mixed_select, side="L", shifted=False)
    for q in range(5):
        assert len(W1[q]) == 1 and np.array_equal(W1[q][0], Ws[q][0])  # bit-identical
    # the blocks as the ABI leaves them: n x maxvec, the columns at and beyond nvec exactly zero
    info, W, nvec, cnts, st = raw_host(eng, pss, bc.D.mixed_select, cplx=cplx)
    assert info == 0 and nvec == nvec0 and W.shape[2] == 7
    for q in range(5):
        for l in range(3):
            assert np.array_equal(W[q, l, :nvec[q]].T, Ws[q][l])
            assert np.all(W[q, l, nvec[q]:] == 0)
    assert st.nb == 5 and st.nvec_total == sum(nvec0) and not cnts.any()


# ------------------------------------------------------------------------------------------------
# 2. batch independence, bit for bit (the vectors and the condition numbers)
def case_independence(eng, eng_groups):
    probs = bc.independence_problems()
    pss = [ps for ps, _ in probs]
    select = np.ones(6, dtype=bool)
    whole = eng.eigvecs_batch(pss, select, side="L")
    swhole, _, _ = eng.eigcond_batch(pss, select)
    for q in range(5):
        check_left(pss[q], whole[q], select, probs[q][1])
    for pos in (0, 33, 69):
        alone = eng.eigvecs_batch([pss[pos]], select, side="L")
        assert _same(alone[0], whole[pos]), pos
        salone, _, Wa = eng.eigcond_batch([pss[pos]], select)
        assert np.array_equal(salone[0], swhole[pos]) and _same(Wa[0], whole[pos])
        for q in (0, 33, 69):  # the same problem at another place
            if q % 5 == pos % 5:
                assert _same(whole[q], whole[pos]) and np.array_equal(swhole[q], swhole[pos])
    rot = pss[33:] + pss[:33]
    turned = eng.eigvecs_batch(rot, select, side="L")
    assert _same(turned[0], whole[33]) and _same(turned[36], whole[69]) and _same(turned[37], whole[0])
    sturned, _, _ = eng.eigcond_batch(rot, select)
    assert np.array_equal(sturned[0], swhole[33]) and np.array_equal(sturned[37], swhole[0])
    parts = eng_groups.eigvecs_batch(pss, select, side="L")
    assert eng_groups.eigvecs_batch_stats.ngroups == 24
    assert all(_same(a, b) for a, b in zip(whole, parts))
    sparts, _, Wp = eng_groups.eigcond_batch(pss, select)
    assert eng_groups.eigvecs_batch_stats.ngroups == 24
    assert all(np.array_equal(a, b) for a, b in zip(swhole, sparts)) and all(_same(a, b) for a, b in zip(whole, Wp))


# ------------------------------------------------------------------------------------------------
# 3. factor layouts
def case_layout(eng, shape):
    p, n = shape
    pairs = [(), (1,) if n >= 4 else (), (n - 2,) if n >= 4 else ()]
    probs = bc._shared(("layout", shape), lambda: [bc.plain_form(n, p, SEEDS[q], pairs[q]) for q in range(3)])
    check_batch(eng, probs, np.ones(n, dtype=bool))


# ------------------------------------------------------------------------------------------------
# 4. orientation and schurindex
def case_orientation(eng):
    """'R' with schurindex p; 'L' with schurindex 2 of 3; n = 6, one pair"""
    n, p = 6, 3
    right = _shared("orientR", lambda: [as_right(bc.plain_form(n, p, 7, (2,))), as_right(bc.plain_form(n, p, 9, (3,)))])
    assert right[0][0].orientation == "R" and right[0][0].schurindex == p
    mid = _shared("si2", lambda: [schur_form_si(n, p, 7, (1,), 2), schur_form_si(n, p, 5, (4,), 2)])
    for probs in (right, mid):
        check_batch(eng, probs, np.ones(n, dtype=bool))
        check_batch(eng, probs, np.array([[0, 0, 1, 0, 1, 0], [1, 0, 0, 0, 1, 1]], dtype=bool))


# ------------------------------------------------------------------------------------------------
# 5. special columns
def negative_problems(p, cplx):
    n = 6
    diag = [np.linspace(1.0, 2.0, n) for _ in range(p)]
    diag[1] = diag[1].copy()
    diag[1][2] = -1.3
    if cplx:
        return _shared(("negz", p), lambda: [bc.zform(n, p, 7), vc.schur_form(n, p, diag, seed=5, cplx=True)])
    return _shared(("neg", p), lambda: [bc.plain_form(n, p, 7, (4,)), vc.schur_form(n, p, diag, seed=5, pairs=(4,))])


def case_negative(eng, p, cplx):
    """a negative real eigenvalue: the relation holds with the CALLER's root and w_l' v_l is constant — with
    psd_ev_root(conj lambda) in place of conj(psd_ev_root(lambda)) the vectors belong to another root and both fail"""
    probs = negative_problems(p, cplx)
    assert probs[1][0].values[2].real < 0 and probs[1][0].values[2].imag == 0
    Vs, Ws = check_batch(eng, probs, np.ones(6, dtype=bool), cplx)
    assert np.abs(Ws[1][1][:, 2].imag).max() > 1e-3  # (mu is complex: so are the vectors of the other factors)
    assert not eng.eigvecs_batch_counts.any()
    check_batch(eng, [as_right(pr) for pr in probs], np.ones(6, dtype=bool), cplx)


def case_zero(eng):
    n, p = 6, 3
    diag = [np.linspace(1.0, 2.0, n) for _ in range(p)]
    diag[0] = diag[0].copy()
    diag[0][3] = 0.0
    probs = bc._shared("zero", lambda: [bc.plain_form(n, p, 7), vc.schur_form(n, p, diag, seed=9), bc.plain_form(n, p, 5)])
    pss = [ps for ps, _ in probs]
    select = np.ones(n, dtype=bool)
    s, Vs, Ws = eng.eigcond_batch(pss, select)
    cnt = eng.eigvecs_batch_counts
    assert cnt[:, 2].tolist() == [0, 1, 0] and eng.eigvecs_batch_stats.nzero == 1
    assert all(np.isnan(W[:, 3]).all() for W in Ws[1]) and np.isnan(s[1][:, 3]).all()
    keep = [0, 1, 2, 4, 5]
    assert np.isfinite(s[1][:, keep]).all() and np.all(s[1][:, keep] > 0)
    assert left_ratio(pss[1], probs[1][1], [W[:, keep] for W in Ws[1]], np.asarray(pss[1].values)[keep]) <= vc.GATE
    for q in (0, 2):  # the NaNs stay in their problem
        check_left(pss[q], Ws[q], select, probs[q][1], Vs[q])
        assert np.isfinite(s[q]).all()


def case_rescale(eng):
    n, p = 8, 6
    diag = []
    for l in range(p):
        g = np.where(np.arange(n) % 2 == 1, 2.0 ** (175 if l < 3 else -175), 1.0)
        diag.append(np.linspace(1.0, 1.7, n) ** (1.0 / p) * g)
    probs = bc._shared("resc", lambda: [bc.plain_form(n, p, 5), vc.schur_form(n, p, diag, seed=23)])
    pss = [ps for ps, _ in probs]
    select = np.ones(n, dtype=bool)
    Ws = eng.eigvecs_batch(pss, select, side="L")
    cnt = eng.eigvecs_batch_counts
    assert cnt[1, 1] > 0 and cnt[0, 1] == 0 and eng.eigvecs_batch_stats.nrescaled == cnt[1, 1]
    assert all(np.isfinite(W).all() for W in Ws[1])
    assert left_ratio(pss[1], probs[1][1], Ws[1], np.asarray(pss[1].values)) <= vc.GATE
    check_left(pss[0], Ws[0], select, probs[0][1])


def case_repeated(eng):
    n, p = 6, 3
    probs = bc._shared("rep", lambda: [vc.schur_form(n, p, [np.full(n, 1.5) for _ in range(p)], seed=7),
                                       bc.plain_form(n, p, 9)])
    pss = [ps for ps, _ in probs]
    select = np.ones(n, dtype=bool)
    Ws = eng.eigvecs_batch(pss, select, side="L")
    cnt = eng.eigvecs_batch_counts
    assert all(np.isfinite(W).all() for W in Ws[0]) and Ws[0][0].shape[1] == n
    assert cnt[0, 0] > 0 and cnt[0, 1] == 0 and cnt[0, 2] == 0 and not cnt[1].any()
    assert eng.eigvecs_batch_stats.nperturbed == cnt[0, 0]
    check_left(pss[1], Ws[1], select, probs[1][1])


# ------------------------------------------------------------------------------------------------
# 6. depth, and above the cap
def case_depth(eng):
    probs = bc.depth_problems()
    check_batch(eng, probs, np.ones(40, dtype=bool))
    launches = eng.eigvecs_batch_stats.nlaunch
    check_batch(eng, probs, np.arange(40) % 3 == 0)
    # the launches of a left call depend neither on n (below the cap) nor on nb
    eng.eigvecs_batch([ps for ps, _ in bc.mixed_problems()], np.ones(7, dtype=bool), side="L")
    assert eng.eigvecs_batch_stats.nlaunch == launches and eng.eigvecs_batch_stats.ngroups == 1


def cap_form(n, p, diag, seed, pairs):
    """evec_cases.schur_form with the strictly upper triangle outside the 2x2 blocks scaled by 0.02.  At this order the
    eigenvalues of the unscaled form (bevec_cases.case_above_cap) have s down to 1e-10: w_l' v_l is then 1e-10 beside
    rounding errors of 1e-16 in it, and cannot be constant over l to 1e-9 relative whatever computes it.  Scaled, s stays
    above 1e-3."""
    ps, _ = vc.schur_form(n, p, diag, seed=seed, pairs=pairs)
    Ts = []
    for l, t in enumerate(ps.Ts):
        t = t - 0.98 * np.triu(t, 1)
        if l == p - 1:
            for i in pairs:
                t[i, i + 1] = 0.7
        Ts.append(np.asfortranarray(t))
    return assemble(Ts, [z.copy(order="F") for z in ps.Z], pairs)


def case_above_cap(eng):
    """the single path on the flipped slices, and its root: one negative diagonal entry"""
    n, p = cap(bc.D.cap_header, bc.D.cap_macro) + 1, 2
    rs = np.random.RandomState(13)
    diag = [np.linspace(0.6, 1.9, n) * (1 + 0.2 * rs.rand(n)) for _ in range(p)]
    diag[1][9] = -diag[1][9]
    probs = _shared(("cap", n), lambda: [cap_form(n, p, diag, s, (5, 23, n - 3)) for s in (17, 7)])
    assert probs[0][0].values[9].real < 0
    select = np.zeros((2, n), dtype=bool)
    select[0] = np.arange(n) % 4 == 1  # (with the negative eigenvalue, the first pair and the last; nvec differs)
    select[1] = np.arange(n) % 8 == 0
    check_batch(eng, probs, select)
    s, _, _ = eng.eigcond_batch([ps for ps, _ in probs], select)
    assert min(x.min() for x in s) > 1e-3


# ------------------------------------------------------------------------------------------------
# 7. condition numbers
def cond_formula(ps, Vs, Ws):
    p = len(Vs)
    s = np.zeros((p, Vs[0].shape[1]))
    for l in range(p):
        l1 = (l + 1) % p
        for k in range(s.shape[1]):
            wn, vn = (Ws[l1][:, k], Vs[l][:, k]) if ps.orientation == "L" else (Ws[l][:, k], Vs[l1][:, k])
            s[l, k] = abs(np.vdot(Ws[l][:, k], Vs[l][:, k])) / (np.linalg.norm(wn) * np.linalg.norm(vn))
    return s


def case_cond_formula(eng, cplx):
    """(a) s is the formula on the returned vectors, to 1e-12 relative; both orientations"""
    probs = mixed_problems(cplx)
    for pr in (probs, [as_right(x) for x in probs]):
        pss = [ps for ps, _ in pr]
        s, Vs, Ws = eng.eigcond_batch(pss, bc.D.mixed_select)
        both = _call(eng, cplx)(pss, bc.D.mixed_select, side="B")
        for q in range(5):
            assert _same(Vs[q], both[0][q]) and _same(Ws[q], both[1][q])
            ref = cond_formula(pss[q], Vs[q], Ws[q])
            assert s[q].shape == ref.shape == (3, Vs[q][0].shape[1])
            assert np.all(np.abs(s[q] - ref) <= 1e-12 * ref), np.abs(s[q] / ref - 1).max()
            assert np.all(s[q] > 0)


def case_cond_p1(eng):
    """(b) p = 1: xTRSNA's S, against scipy's left and right eigenvectors of A_1"""
    import scipy.linalg as sl

    probs = bc._shared(("layout", (1, 5)), lambda: [bc.plain_form(5, 1, SEEDS[q], [(), (1,), (3,)][q]) for q in range(3)])
    pss = [ps for ps, _ in probs]
    s, _, _ = eng.eigcond_batch(pss, np.ones(5, dtype=bool))
    for q, (ps, As) in enumerate(probs):
        w, vl, vr = sl.eig(As[0], left=True, right=True)
        for k, lam in enumerate(ps.values):
            j = np.argmin(np.abs(w - lam))
            ref = abs(np.vdot(vl[:, j], vr[:, j])) / (np.linalg.norm(vl[:, j]) * np.linalg.norm(vr[:, j]))
            assert abs(s[q][0, k] - ref) <= 1e-9, (q, k, s[q][0, k], ref)


def _product(As, left):
    P = np.eye(As[0].shape[0], dtype=complex)
    for a in (As if left else As[::-1]):  # 'L': A_p ... A_1; 'R': A_1 ... A_p
        P = a @ P
    return P


def case_cond_perturbation(eng, cplx):
    """(c) one factor perturbed by 1e-6 E: the eigenvalue shifts of the explicit product agree with the first-order
    formula d lambda = mu^(p-1) 1e-6 w_{l+1}' E v_l / (w_1' v_1) ('R': w_l' E v_{l+1}) to 1e-3 relative"""
    n, p = (6, 4) if cplx else (7, 3)
    base = bc.zform(n, p, 7) if cplx else bc.mixed_problems()[2]  # (real: pairs at rows 2 and 5)
    for prob in (base, as_right(base)):
        ps, As = prob
        left = ps.orientation == "L"
        s, Vs, Ws = eng.eigcond_batch([ps], np.ones(n, dtype=bool))
        V, W = Vs[0], Ws[0]
        lam0 = np.linalg.eigvals(_product(As, left))
        rs = np.random.RandomState(41)
        for l in (0, p - 1):
            E = rs.randn(n, n) + (1j * rs.randn(n, n) if cplx else 0)
            Ap = [a.copy() for a in As]
            Ap[l] = Ap[l] + 1e-6 * E
            lam1 = np.linalg.eigvals(_product(Ap, left))
            l1 = (l + 1) % p
            for k, lam in enumerate(ps.values):
                mu = mu_of(lam, p)
                num = np.vdot(W[l1][:, k], E @ V[l][:, k]) if left else np.vdot(W[l][:, k], E @ V[l1][:, k])
                pred = mu ** (p - 1) * 1e-6 * num / np.vdot(W[0][:, k], V[0][:, k])
                a = lam0[np.argmin(np.abs(lam0 - lam))]
                got = lam1[np.argmin(np.abs(lam1 - a))] - a
                assert abs(got - pred) <= 1e-3 * abs(pred), (l, k, got, pred)
                # the bound the condition numbers give (one factor perturbed)
                assert abs(got / lam) <= (1 + 1e-3) * 1e-6 * np.linalg.norm(E, 2) / (abs(mu) * s[0][l, k])


def case_cond_extremes(eng):
    """(d) a near-defective problem (a Jordan-like 2x2 block of the product, diagonal gap 1e-8, off-diagonal 1):
    min_l s < 1e-5; a normal one (diagonal T_l, the same in every factor — s[l, j] is |T_l(j, j)| / |mu_j| otherwise):
    s = 1 to 1e-12"""
    rs = np.random.RandomState(3)
    Zs = [np.asfortranarray(np.linalg.qr(rs.randn(2, 2))[0]) for _ in range(2)]
    Ts = [np.asfortranarray(np.array([[1.0, 1.0], [0.0, 1.0 + 1e-8]])), np.asfortranarray(np.eye(2))]
    ps, _ = assemble(Ts, Zs)
    s, _, _ = eng.eigcond_batch([ps], [True, True])
    assert s[0].shape == (2, 2) and np.all(s[0].min(axis=0) < 1e-5) and np.all(s[0] > 0)
    n, p = 5, 3
    Zs = [np.asfortranarray(np.linalg.qr(rs.randn(n, n))[0]) for _ in range(p)]
    Ts = [np.asfortranarray(np.diag(np.linspace(1.0, 2.0, n) ** (1.0 / p))) for l in range(p)]
    ps, _ = assemble(Ts, Zs)
    s, _, _ = eng.eigcond_batch([ps], np.ones(n, dtype=bool))
    assert np.all(np.abs(s[0] - 1.0) <= 1e-12), np.abs(s[0] - 1).max()


# ------------------------------------------------------------------------------------------------
# 8. errors
def case_errors(eng, make_engine):
    probs = bc.mixed_problems()
    pss = [ps for ps, _ in probs]
    n, p = 7, 3
    for bad in ("X", "l", None, 1):
        with pytest.raises(ValueError, match="side"):
            eng.eigvecs_batch(pss, [True] * n, side=bad)
    with pytest.raises(ValueError, match="side"):
        eng.zeigvecs_batch([ps for ps, _ in bc.mixed_problems(bc.Z)], [True] * n, side="left")
    g = psd_amd.GeneralizedPeriodicSchur([True, False, True], pss[0].Ts, pss[0].Z, np.array(pss[0].values), np.ones(n),
                                         np.zeros(n, dtype=np.int32), "L", p)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.eigvecs_batch([pss[0], g], [True] * n, side="L")
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.eigcond_batch([pss[0], g], [True] * n)
    with pytest.raises(ValueError, match="argument 9"):
        eng.eigvecs_batch(pss, [True] * (n - 1), side="L")
    with pytest.raises(TypeError):
        eng.eigcond_batch(pss, [True] * n, [True] * n)
    sharded = make_engine()
    sharded.set_shard(0, 2)
    with pytest.raises(psd_amd.NotImplementedPSD):
        sharded.eigvecs_batch(pss, [True] * n, side="L")
    with pytest.raises(psd_amd.NotImplementedPSD):
        sharded.zeigvecs_batch([ps for ps, _ in bc.mixed_problems(bc.Z)], [True] * n, side="B")
    # an empty batch
    assert eng.eigvecs_batch([], [True] * n, side="L") == []
    assert eng.eigvecs_batch([], [True] * n, side="B") == ([], [])
    assert eng.eigcond_batch([], [True] * n) == ([], [], [])
    # nothing selected: no columns, no condition numbers, no launch
    s, Vs, Ws = eng.eigcond_batch(pss, np.zeros(n, dtype=bool))
    assert all(x.shape == (p, 0) for x in s) and all(W.shape == (n, 0) for Wq in Ws for W in Wq)
    assert eng.eigvecs_batch_stats.nlaunch == 0
    info, W, nvec, _, _ = raw_host(eng, pss, bc.D.mixed_select, maxvec=6)  # problem 0 has 7 columns
    assert info == -10 and nvec == bc.D.mixed_nvec
    info, W, nvec, _, _ = raw_host(eng, [ps for ps, _ in bc.mixed_problems(bc.Z)], bc.D.mixed_select, maxvec=6, cplx=True)
    assert info == -10 and nvec == bc.Z.mixed_nvec


def case_abi(eng, make_engine):
    """the device entries through the C ABI on packed blocks (in the simulation device memory is host memory): the bits of
    the host entries, and the argument codes of the six entries"""
    nb, n, p = 5, 7, 3
    dp, u8p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    lib, ctx = eng.lib, eng.ctx
    sel0 = np.ascontiguousarray(bc.D.mixed_select, dtype=np.uint8)
    blocks = {}
    for cplx in (False, True):
        pss = [ps for ps, _ in mixed_problems(cplx)]
        nvec0 = bc.Z.mixed_nvec if cplx else bc.D.mixed_nvec
        host = _call(eng, cplx)(pss, bc.D.mixed_select, side="L")
        dt = np.complex128 if cplx else np.float64
        dT = np.ascontiguousarray(np.array([pt.pack(ps.Ts, dt) for ps in pss]))
        dZ = np.ascontiguousarray(np.array([pt.pack(ps.Z, dt) for ps in pss]))
        vals = np.ascontiguousarray(np.array([np.asarray(ps.values, dtype=complex) for ps in pss]))
        if cplx:
            beta = np.ones(vals.shape)
            ev = [vals.ctypes.data_as(dp), beta.ctypes.data_as(dp), None]
        else:
            wr, wi = np.ascontiguousarray(vals.real), np.ascontiguousarray(vals.imag)
            ev = [wr.ctypes.data_as(dp), wi.ctypes.data_as(dp)]
        sel = sel0.copy()
        selp = sel.ctypes.data_as(u8p)
        nvec = (C.c_int * nb)()
        cnts = np.zeros((nb, 3), dtype=np.int32)
        st = psd_amd.BevecStats()
        info = C.c_int(0)
        bT, bZ = C.c_void_p(dT.ctypes.data), C.c_void_p(dZ.ctypes.data)
        fdev = lib.psd_z_leigvecs_batch_dev if cplx else lib.psd_d_leigvecs_batch_dev
        fhost = lib.psd_z_leigvecs_batch if cplx else lib.psd_d_leigvecs_batch
        rc = fdev(ctx, nb, n, p, bT, bZ, *ev, b"L", p, selp, 1, None, 0, nvec, cnts.ctypes.data_as(i32p), C.byref(st),
                  C.byref(info))
        assert rc == 0 and list(nvec) == nvec0
        W = np.full((nb, p, 7, n), 7.0 + 7.0j)
        rc = fdev(ctx, nb, n, p, bT, bZ, *ev, b"L", p, selp, 1, C.c_void_p(W.ctypes.data), 7, nvec,
                  cnts.ctypes.data_as(i32p), C.byref(st), C.byref(info))
        # (the launches of the right device entry — 5 real with the sub-diagonal kernel, 4 complex — and two)
        assert rc == 0 and info.value == 0 and st.nb == nb and st.ngroups == 1 and st.nlaunch == (6 if cplx else 7)
        for q in range(nb):
            for l in range(p):
                assert np.array_equal(W[q, l, :nvec[q]].T, host[q][l]) and np.all(W[q, l, nvec[q]:] == 0)
        assert all(np.array_equal(dT[q], pt.pack(pss[q].Ts, dt)) for q in range(nb))  # the inputs stay as they were
        assert all(np.array_equal(dZ[q], pt.pack(pss[q].Z, dt)) for q in range(nb))
        blocks[cplx] = (W, list(nvec))
        Tp = eng._ptrs([np.asfortranarray(t, dtype=dt) for ps in pss for t in ps.Ts])
        Zp = eng._ptrs([np.asfortranarray(z, dtype=dt) for ps in pss for z in ps.Z])

        def call(fn, T0, Z0, c_=ctx, nb_=nb, n_=n, p_=p, T_=0, Z_=0, e0=0, o=b"L", si=p, sel_=selp, V_=None, mv=0,
                 nv=nvec):
            T_, Z_ = (T0 if T_ == 0 else T_), (Z0 if Z_ == 0 else Z_)
            e = list(ev) if e0 == 0 else [None] + list(ev[1:])
            return fn(c_, nb_, n_, p_, T_, Z_, *e, o, si, sel_, 1, V_, mv, nv, None, None, None)

        for fn, T0, Z0 in ((fdev, bT, bZ), (fhost, Tp, Zp)):
            f = lambda **kw: call(fn, T0, Z0, **kw)  # noqa: E731
            assert f() == 0
            assert f(c_=None) == -1 and f(n_=0) == -2 and f(p_=0) == -3 and f(T_=None) == -4 and f(Z_=None) == -5
            assert f(e0=None) == -6 and f(o=b"X") == -7 and f(si=0) == -8 and f(si=p + 1) == -8 and f(sel_=None) == -9
            assert f(nb_=-1) == -11 and f(nv=None) == -12
            assert f(nb_=0, T_=None, Z_=None, sel_=None, nv=None) == 0  # nb == 0 touches nothing
        assert call(fdev, bT, bZ, V_=C.c_void_p(W.ctypes.data), mv=6) == -10
    # the condition numbers of the real batch: device blocks against host pointers
    pss = [ps for ps, _ in bc.mixed_problems()]
    s0, Vs, Ws = eng.eigcond_batch(pss, bc.D.mixed_select)
    W, nvec0 = blocks[False]
    V = np.zeros_like(W)
    for q in range(nb):
        for l in range(p):
            V[q, l, :nvec0[q]] = Vs[q][l].T
    nv = (C.c_int * nb)(*nvec0)
    s = np.full((nb, 7, p), 7.0)
    info = C.c_int(0)
    sp = s.ctypes.data_as(dp)
    bV, bW = C.c_void_p(V.ctypes.data), C.c_void_p(W.ctypes.data)
    assert lib.psd_eigcond_batch_dev(ctx, nb, n, p, bV, bW, b"L", 7, nv, sp, C.byref(info)) == 0 and info.value == 0
    for q in range(nb):
        assert np.array_equal(s[q, :nvec0[q]].T, s0[q]) and np.all(s[q, nvec0[q]:] == 0)
    Vp = (C.c_void_p * (nb * p))(*[V[q, l].ctypes.data for q in range(nb) for l in range(p)])
    Wp = (C.c_void_p * (nb * p))(*[W[q, l].ctypes.data for q in range(nb) for l in range(p)])
    s2 = np.full((nb, 7, p), 7.0)
    assert lib.psd_eigcond_batch(ctx, nb, n, p, Vp, Wp, b"L", 7, nv, s2.ctypes.data_as(dp), None) == 0
    assert np.array_equal(s, s2)
    sharded = make_engine()
    sharded.set_shard(0, 2)
    for fn, V0, W0 in ((lib.psd_eigcond_batch_dev, bV, bW), (lib.psd_eigcond_batch, Vp, Wp)):
        def f(c_=ctx, nb_=nb, n_=n, p_=p, V_=V0, W_=W0, o=b"L", mv=7, nv_=nv, s_=sp):
            return fn(c_, nb_, n_, p_, V_, W_, o, mv, nv_, s_, None)

        assert f() == 0
        assert f(c_=None) == -1 and f(n_=0) == -2 and f(p_=0) == -3 and f(V_=None) == -4 and f(W_=None) == -5
        assert f(o=b"X") == -7 and f(mv=0) == -10 and f(mv=6) == -10 and f(nb_=-1) == -11 and f(nv_=None) == -12
        assert f(s_=None) == -13
        assert f(nb_=0, V_=None, W_=None, nv_=None, s_=None) == 0  # nb == 0 touches nothing
        assert f(c_=sharded.ctx) == psd_amd.INFO_NOTIMPL  # a period-sharded context


# ------------------------------------------------------------------------------------------------
# 9. pipeline, device-resident (GPU tier)
def case_pipeline(eng, lr, cplx):
    import torch

    n, p, nb = 12, 3, 5
    rs = np.random.RandomState(77)
    facs = [pt.bench_factors(n, p, seed=91 + q) for q in range(nb)]
    if cplx:
        facs = [[np.asfortranarray(a + 1j * rs.randn(n, n) / np.sqrt(n)) for a in A] for A in facs]
    dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in facs])).cuda()
    T, Z, values, _ = (eng.zpschur_batch_ if cplx else eng.pschur_batch_)(dA, lr)
    si = p if lr == "L" else 1
    select = np.ones((nb, n), dtype=bool)
    select[1] = np.arange(n) % 2 == 0
    V, W, nvec = _call(eng, cplx)(T, Z, values, select, lr=lr, schurindex=si, side="B")
    assert V.is_cuda and W.is_cuda and tuple(V.shape) == tuple(W.shape) == (nb, p, n, int(max(nvec)))
    s, V2, W2, nvec2 = eng.eigcond_batch(T, Z, values, select, lr=lr, schurindex=si)
    assert V2.is_cuda and W2.is_cuda and torch.equal(V2, V) and torch.equal(W2, W) and nvec2.tolist() == nvec.tolist()
    assert isinstance(s, np.ndarray) and s.shape == (nb, p, int(max(nvec)))
    Vh, Wh, Th, Zh = V.cpu().numpy(), W.cpu().numpy(), T.cpu().numpy(), Z.cpu().numpy()
    for q in range(nb):
        ps = psd_amd.PeriodicSchur([np.asfortranarray(Th[q, l]) for l in range(p)],
                                   [np.asfortranarray(Zh[q, l]) for l in range(p)], values[q], lr, si)
        Vs = [Vh[q, l][:, :nvec[q]] for l in range(p)]
        Ws = [Wh[q, l][:, :nvec[q]] for l in range(p)]
        assert np.all(Wh[q][:, :, nvec[q]:] == 0) and np.all(s[q][:, nvec[q]:] == 0)
        lams = vc.order_values(ps, select[q])
        assert Ws[0].shape[1] == len(lams)
        assert vc.relation_ratio(facs[q], Vs, lams, left=(lr == "L")) <= vc.GATE
        r = left_ratio(ps, facs[q], Ws, lams)  # against the original factors
        assert r <= vc.GATE, (lr, q, r)
        d = np.array([[np.vdot(Ws[l][:, k], Vs[l][:, k]) for k in range(len(lams))] for l in range(p)])
        assert np.all(np.abs(d - d[0]) <= 1e-9 * np.abs(d[0]))
        ref = cond_formula(ps, Vs, Ws)
        assert np.all(np.abs(s[q][:, :nvec[q]] - ref) <= 1e-12 * ref)
    W1, nvec1 = _call(eng, cplx)(T, Z, values, select, lr=lr, schurindex=si, side="L", shifted=False)
    assert tuple(W1.shape) == (nb, 1, n, int(max(nvec))) and torch.equal(W1[:, 0], W[:, 0])
    assert nvec1.tolist() == nvec.tolist()


def case_empty_device(eng):
    import torch

    T = torch.zeros((0, 2, 3, 3), dtype=torch.float64, device="cuda")
    V, W, nvec = eng.eigvecs_batch(T, T.clone(), np.zeros((0, 3)), np.zeros((0, 3), dtype=bool), side="B")
    assert tuple(V.shape) == tuple(W.shape) == (0, 2, 3, 0) and W.dtype == torch.complex128 and W.is_cuda
    assert nvec.shape == (0,) and nvec.dtype == np.int32
    W1, _ = eng.eigvecs_batch(T, T.clone(), np.zeros((0, 3)), [True] * 3, shifted=False, side="L")
    assert tuple(W1.shape) == (0, 1, 3, 0)
    s, V, W, nvec = eng.eigcond_batch(T, T.clone(), np.zeros((0, 3)), [True] * 3)
    assert s.shape == (0, 2, 0) and tuple(W.shape) == (0, 2, 3, 0) and nvec.shape == (0,)
    st = eng.eigvecs_batch_stats
    assert isinstance(st, psd_amd.BevecStats) and st.nb == 0 and st.nlaunch == 0
    Tz = torch.zeros((0, 2, 3, 3), dtype=torch.complex128, device="cuda")
    s, V, W, nvec = eng.eigcond_batch(Tz, Tz.clone(), np.zeros((0, 3)), [True] * 3)
    assert s.shape == (0, 2, 0) and tuple(V.shape) == (0, 2, 3, 0)
