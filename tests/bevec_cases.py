"""Cases for the batched eigenvector entries of the four families — Engine.eigvecs_batch / zeigvecs_batch (right
eigenvectors by back-substitution; psd_{d,z}_eigvecs_batch[_dev], csrc/psd_bevec.h, psd_zbevec.h) and zgeigvecs_batch /
dgeigvecs_batch (geigvecs: the vectors and scalars of the signed relations; psd_{z,d}_geigvecs_batch[_dev],
csrc/psd_zgbevec.h, psd_gbevec.h): many small periodic Schur forms in one call.  Each case takes an engine and a family
(batch_common.Family); tests/test_hostsim_*eigvecs_batch.py run them on the serial simulation,
tests/test_gpu_*eigvecs_batch.py on the device.  lbevec_cases.py (left eigenvectors and condition numbers of D and Z) takes
its inputs from here.

Every gate is the project's own.  Unsigned (D, Z): evec_cases.check_columns — relation ratio <= evec_cases.GATE, agreement
with the numpy prototype backsub_ref at its atol, norm, phase and (D) conjugates.  Signed (ZG, DG): check_signed — the
relation ratio gevec_cases.relation_ratio <= GATE (1e-11), agreement with gevec_cases.prototype at atol 1e-9 and of the
scalars a at rtol 1e-13, norm within 1e-13, a real positive phase entry, a on 1 x 1 columns exactly the diagonal entries of
T_l, the partner column and scalars of a pair the exact conjugates.  The inputs are built directly as Schur forms by the
generators of the single-problem tests (evec_cases.schur_form, gevec_cases.signed_form) with the seeds of the descriptors;
Z and ZG have genuinely complex diagonals (zdiag, zgdiag), so the principal root matters.  What the prototypes and the
single calls reach on these inputs, measured: Z: backsub_ref a relation ratio of at most 4.7e-15; ZG: the prototype 6.7e-15,
the batched path 2.0e-15 at most 5.5e-12 from the prototype on the MI355X; DG: the batched path 3.0e-14, at most 1.0e-12
from the prototype and 7.3e-15 from the single geigvecs on the MI355X (FIGURES collects DG's; test_zz_figures prints them).
Both signed families count 15 perturbed pivots on the repeated eigenvalue and 5 rescaled columns on the graded problem.

A case is one body where the families differ in names, element type, inputs or constants: the descriptors below hold
those.  Where they check different things the functions stand side by side:

- A call of an unsigned family returns the vectors, one of a signed family (vectors, scalars), and their checkers differ
  (check_one); the entries take the eigenvalues as (wr, wi) for D, (alpha, beta, ascale) for Z, and a signature instead
  for the signed ones (_values, raw_host, case_dev_abi).
- The unsigned families alone have the cases of the back-substitution's special columns (case_special_negative, D only: a
  negative product with an even period; case_special_repeated, _zero, _rescale) and case_above_cap at PSD_BEV_NMAX + 1; the
  signed families alone have theirs (case_all_false, case_cap, case_zero_infinite, case_repeated, case_rescale,
  case_all_true_zg / _dg, case_pipeline_host, case_gpschur_batch).
- The device-resident pipeline of the unsigned families is pschur_batch_ -> eigvecs_batch against eigvecs_dev
  (case_pipeline); that of the signed ones goes through the reordering (case_pipeline_signed).
- An all-true signature is compared with zeigvecs_batch for ZG; for DG, which has no unsigned entry of the same output, a
  PeriodicSchur and a GeneralizedPeriodicSchur are compared with each other.

Differences between the families that nothing explains, left as they are:
- The comparison with the single call (geigvecs on the same engine: the scalars' bits, on the simulation the vectors' bits
  for n <= 16) and with its counts of special columns is made for DG only, and DG alone records FIGURES.
- The number of launches of a call is asserted as 4 (3 without the other factors) for Z, ZG and DG; for D only that it
  depends neither on nb nor on n.  p = 1 and an empty selection are counted for the signed families only.
- case_mixed asserts ngroups, nlaunch and the three counters of the stats for the signed families only.
- The device entry's launches: 5 for D, 4 for Z (no gather), 5 for the signed ones with the scalars; the size query of DG
  launches its gather, that of ZG nothing."""
import ctypes as C
from functools import partial

import numpy as np
import pytest

import batch_common as bcm
import evec_cases as vc
import gevec_cases as gc
import psd_amd
import psdtest as pt

FIGURES = {}  # DG: (tier, figure) -> worst value seen


def _shared(key, make, fam=bcm.D):
    """Inputs — lists of (decomposition, factors) — are built once, shared among the cases, and never written to."""
    def readonly():
        out = make()
        for P, As in out:
            for a in list(P.Ts) + list(P.Z) + list(As):
                a.setflags(write=False)
        return out
    return bcm.cached(("bevec", fam.name, key), readonly)


def is_sim(eng):
    return "hostsim" in eng.lib._name


def _figure(eng, fam, name, v):
    if fam is DG:
        key = ("sim" if is_sim(eng) else "gpu", name)
        FIGURES[key] = max(FIGURES.get(key, 0.0), float(v))


def print_figures():
    for key in sorted(FIGURES):
        print("dgeigvecs_batch worst %s %s: %.3e" % (key[0], key[1], FIGURES[key]))


def sig(p):
    return gc.S_ALT(p) if p < 4 else gc.S_TFFT(p)


# ------------------------------------------------------------------------------------------------
# the form builders: (decomposition, factors) of order n and period p.  One signature; a family ignores what it has not —
# pairs (rows of 2 x 2 blocks) where complex, lr and S where unsigned
def plain_form(n, p, seed, pairs=(), lr="L", S=None, diag=None):
    """an ordinary Float64 problem: every row's product of diagonals is linspace(1, 2, n)[row], distinct and moderate"""
    diag = [np.linspace(1.0, 2.0, n) ** (1.0 / p) for _ in range(p)] if diag is None else diag
    return vc.schur_form(n, p, diag, seed=seed, pairs=pairs)


def zdiag(n, p, seed):
    """per factor: moduli linspace(1, 2, n) ** (1/p) — every row's product has modulus linspace(1, 2, n)[row] — times
    phases exp(i U(-pi, pi))"""
    rs = np.random.RandomState(1000 + seed)
    return [np.linspace(1.0, 2.0, n) ** (1.0 / p) * np.exp(1j * rs.uniform(-np.pi, np.pi, n)) for _ in range(p)]


def zform(n, p, seed, pairs=(), lr="L", S=None, diag=None):
    """an ordinary ComplexF64 problem"""
    return vc.schur_form(n, p, zdiag(n, p, seed) if diag is None else diag, seed, cplx=True)


def zgdiag(n, p, seed):
    """per factor: (0.7 + 0.8 U) exp(i U(-pi, pi))"""
    rs = np.random.RandomState(2000 + seed)
    return [(0.7 + 0.8 * rs.rand(n)) * np.exp(1j * rs.uniform(-np.pi, np.pi, n)) for _ in range(p)]


def zgform(n, p, seed, pairs=(), lr="L", S=None, diag=None):
    """a signed ComplexF64 problem, signature S_ALT(p) for p < 4, else S_TFFT(p)"""
    return gc.signed_form(n, p, sig(p) if S is None else S, lr, diag=zgdiag(n, p, seed) if diag is None else diag,
                          seed=seed, cplx=True, si=1 if lr == "R" else p)


def dgform(n, p, seed, pairs=(), lr="L", S=None, diag=None):
    """a signed Float64 problem, the same signatures"""
    return gc.signed_form(n, p, sig(p) if S is None else S, lr, diag=diag, seed=seed, pairs=pairs,
                          si=1 if lr == "R" else p)


def _depth_diag(n, p):
    rs = np.random.RandomState(13)
    return [np.linspace(0.6, 1.9, n) * (1 + 0.2 * rs.rand(n)) for _ in range(p)]  # (evec_cases.case_chunks)


def layout_id(s, sep="_"):
    return "p%d%sn%d" % (s[0], sep, s[1])


# ------------------------------------------------------------------------------------------------
# the families of this role.  form: the builder above.  seeds: of the problems of a case, in order (D, Z: those of
# evec_cases' own schur_form problems; signed: 5, 7, 9, and 15, 17 where a case needs five).  layouts: (p, n[, pair rows])
# — p = 1; p = 70 (lanes own two factors; signed: r in a global buffer); n = 1; p = 5 (idle lanes inside a sub-group of 8);
# p = 32 (one sub-group per half-wave); DG: and the block widths noted there; layout_pairs: the pair rows of the three
# problems of a layout.  mixed_select / mixed_nvec / mixed_pairs: the selections of case_mixed, the columns they give (a
# Float64 selection is completed to whole pairs) and the pair rows of its five problems; indep_pairs: of the five of
# case_independence.  depth_seeds, depth_pairs, depth_diag, depth_selects: the problems of order 40 and what is selected
# there.  gate, cap_header / cap_macro: the relation gate and where the order cap of the batched kernel is defined.
# launch: (n, pair rows, batch sizes) of case_launch_count; nlaunch: the launches of a host call; dev_nlaunch: of the
# device entry in case_dev_abi; vs_single: check_signed compares with the single call and records FIGURES.
_LAYOUTS = [(1, 5), (70, 5), (3, 1), (5, 9), (32, 4)]
_DEPTH3 = [np.ones(40, dtype=bool), np.arange(40) % 3 == 0]
_SELECT_C = np.array([
    [1, 1, 1, 1, 1, 1, 1],
    [0, 1, 0, 0, 1, 0, 0],  # (D: row 1 is the SECOND member of the pair at rows 0, 1)
    [0, 0, 1, 0, 0, 0, 1],
    [1, 0, 0, 0, 0, 0, 0],
    [0, 1, 0, 0, 1, 1, 0],
], dtype=bool)
D = bcm.D.with_(form=plain_form, seeds=(5, 7, 9, 17, 23), layouts=_LAYOUTS, layout_id=layout_id,
                layout_pairs=lambda s: [(), (1,) if s[1] >= 4 else (), (s[1] - 2,) if s[1] >= 4 else ()],
                mixed_select=_SELECT_C, mixed_nvec=[7, 3, 4, 1, 5], mixed_pairs=[(), (0,), (2, 5), (4,), (1, 3)],
                indep_pairs=[(), (1,), (3,), (0, 4), (2,)], depth_seeds=(17, 7, 9), depth_pairs=(5, 23, 37),
                depth_diag=_depth_diag, depth_selects=_DEPTH3, gate=vc.GATE, cap_header="psd_bevec.h",
                cap_macro="PSD_BEV_NMAX", launch=(12, [(), (3,), (7,), (0, 9), (5,)], (3, 40)), nlaunch=None, dev_nlaunch=5)
Z = bcm.Z.with_(form=zform, seeds=D.seeds, layouts=_LAYOUTS, layout_id=layout_id, layout_pairs=lambda s: [()] * 3,
                mixed_select=_SELECT_C, mixed_nvec=[7, 2, 2, 1, 3],  # (the rows as given: nothing to complete)
                mixed_pairs=[()] * 5, indep_pairs=[()] * 5, depth_seeds=(5, 7, 9), depth_pairs=(), depth_diag=None,
                depth_selects=_DEPTH3, gate=vc.GATE, cap_header="psd_bevec.h", cap_macro="PSD_BEV_NMAX",
                launch=(12, [()] * 5, (3, 40)), nlaunch=4, dev_nlaunch=4)
ZG = bcm.ZG.with_(form=zgform, seeds=(5, 7, 9, 15, 17), layouts=_LAYOUTS, layout_id=partial(layout_id, sep="-"),
                  layout_pairs=lambda s: [()] * 3, mixed_select=_SELECT_C, mixed_nvec=Z.mixed_nvec, mixed_pairs=[()] * 5,
                  indep_pairs=[()] * 5, depth_seeds=(5, 7, 9), depth_pairs=(), depth_diag=None,
                  depth_selects=[np.arange(40) % 7 == 0], gate=gc.GATE, launch=(4, [()] * 3, (1, 70)), nlaunch=4,
                  dev_nlaunch=5, vs_single=False)
# mixed: rows 0 | (1, 2) | 3 | (4, 5) | 6.  depth: 1x1 columns through every pair, two own pairs
DG = bcm.DG.with_(form=dgform, seeds=ZG.seeds, layout_id=ZG.layout_id, layout_pairs=lambda s: [s[2]] * 3,
                  layouts=[(2, 6, (0, 3)),           # of the mixed shapes
                           (1, 5, (2,)),             # p = 1
                           (3, 2, (0,)),             # n = 2: the problem is one own 2x2 block
                           (3, 1, ()),               # n = 1
                           (70, 5, (1,)),            # lanes own two factors, r in the global buffer
                           (5, 9, (0, 4, 7)),        # idle lanes in a sub-group of 8; pairs at the top and the bottom rows
                           (32, 4, (0, 2)),          # one sub-group per half-wave; every row in a pair
                           (4, 12, (1, 5, 9)),       # sixteen units per wavefront, blocks of width 1 and 2 in one step
                           (2, 17, (15,)),           # pairs where the single path splits chunks
                           (3, 33, (15, 31))],
                  mixed_select=np.array([[1, 1, 1, 1, 1, 1, 1],   # all
                                         [0, 0, 1, 0, 0, 0, 0],   # the second member of a pair only
                                         [0, 0, 0, 0, 0, 0, 0],   # none
                                         [1, 0, 0, 1, 0, 1, 0],   # 1x1 rows and a second member
                                         [0, 1, 0, 0, 0, 0, 1]], dtype=bool),
                  mixed_nvec=[7, 2, 0, 4, 3], mixed_pairs=[(1, 4)] * 5, indep_pairs=[(0, 3)] * 5, depth_seeds=(5, 7, 9),
                  depth_pairs=(3, 16, 30, 38), depth_diag=None,
                  depth_selects=[(np.arange(40) % 7 == 0) | np.isin(np.arange(40), [17, 38])], gate=gc.GATE,
                  launch=(4, [(1,)] * 3, (1, 70)), nlaunch=4, dev_nlaunch=5, vs_single=True)


# ------------------------------------------------------------------------------------------------
# calls and checks
def run(eng, fam, Ps, select, **kw):
    return fam.method(eng, "eigvecs_batch")(Ps, select, **kw)


def vectors(fam, r):
    """the vectors of one problem's result"""
    return r[0] if fam.signed else r


def _same(fam, ra, rb):
    """two results of one problem: the same bits — the vectors and, signed, the scalars"""
    Va, Vb = vectors(fam, ra), vectors(fam, rb)
    return (len(Va) == len(Vb) and all(np.array_equal(x, y) for x, y in zip(Va, Vb))
            and (not fam.signed or np.array_equal(ra[1], rb[1])))


def completed(P, select):
    """select completed to whole pairs"""
    s = np.zeros(P.Ts[0].shape[0], dtype=bool)
    for k, m in gc._columns(P, select):
        s[k:k + m] = True
    return s


def single(eng, P, select):
    """the single call on the same engine: computed once per (engine, problem, selection)"""
    def make():
        Vs, a = eng.geigvecs(P, list(np.asarray(select, dtype=bool)))
        st = eng.eigvecs_stats
        return Vs, a, (st.nperturbed, st.nrescaled, st.nzero), eng, P  # (the engine and the problem keep their ids)
    return bcm.cached(("bevec single", id(eng), id(P), np.asarray(select, dtype=bool).tobytes()), make)[:3]


def check_signed(eng, fam, P, As, Vs, a, select, proto=True, vs_single=True):
    """the full check of one signed problem's result; prints the figures before it asserts"""
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
    _figure(eng, fam, "ratio", r)
    assert r <= fam.gate, r
    V1 = Vs[0]
    assert np.allclose(np.linalg.norm(V1, axis=0), 1.0, atol=1e-13)
    for c in range(V1.shape[1]):
        am = np.argmax(np.abs(V1[:, c]))
        assert V1[am, c].imag == 0 and V1[am, c].real > 0
    if proto and nvec:
        ref, aref = gc.prototype(P, select)
        d = max(np.abs(Vs[l] - ref[l]).max() for l in range(p))
        print("(p, n) = (%d, %d) %s: distance to the prototype %.3e" % (p, n, P.orientation, d))
        _figure(eng, fam, "proto", d)
        assert np.allclose(a, aref, rtol=1e-13, atol=0)
        for l in range(p):
            assert np.allclose(Vs[l], ref[l], rtol=0, atol=1e-9), (l, np.abs(Vs[l] - ref[l]).max())
    if fam.vs_single and vs_single and nvec:
        Vr, ar, _ = single(eng, P, select)
        d = max(np.abs(Vs[l] - Vr[l]).max() for l in range(p))
        print("(p, n) = (%d, %d) %s: distance to the single call %.3e" % (p, n, P.orientation, d))
        _figure(eng, fam, "single", d)
        assert np.array_equal(a, ar)  # the same host function
        if is_sim(eng) and n <= 16:  # one chunk of the single path: the same sums in the same order
            assert all(np.array_equal(x, y) for x, y in zip(Vs, Vr))


def check_one(eng, fam, P, As, r, select, proto=True, vs_single=True):
    """one problem's result against the family's gates"""
    if fam.signed:
        check_signed(eng, fam, P, As, r[0], r[1], select, proto, vs_single)
    else:
        assert len(r) == len(P.Ts)
        vc.check_columns(P, r, select, As)


def check_batch(eng, fam, probs, select, proto=True, vs_single=True):
    """run the batch, check every problem; returns the results"""
    Ps = [P for P, _ in probs]
    nb, n = len(Ps), Ps[0].Ts[0].shape[0]
    out = run(eng, fam, Ps, select)
    sel = np.broadcast_to(np.asarray(select, dtype=bool), (nb, n))
    assert len(out) == nb
    for q, (P, As) in enumerate(probs):
        check_one(eng, fam, P, As, out[q], sel[q], proto, vs_single)
    return out


def _values(fam, Ps):
    """the eigenvalue arrays an unsigned entry takes, [nb][n] each: (wr, wi) for D, (alpha, beta) for Z"""
    vals = np.ascontiguousarray(np.array([np.asarray(P.values, dtype=np.complex128) for P in Ps]))
    if fam.cplx:
        return vals, np.ones(vals.shape)
    return np.ascontiguousarray(vals.real), np.ascontiguousarray(vals.imag)


def _entry_args(fam, Ps, vals, ascale=None):
    """what stands between Z and orient in the family's entries: the values (Z: and ascale) or the signature"""
    if fam.signed:
        return [bcm.sarr(gc._sgn(Ps[0]))]
    dp = C.POINTER(C.c_double)
    return [v.view(np.float64).ctypes.data_as(dp) for v in vals] + ([ascale] if fam.cplx else [])


def raw_host(eng, fam, Ps, select, shifted=True, maxvec=None):
    """The family's host entry through the C ABI — the size query, then the call: (info, V [nb][nmat][maxvec][n] complex,
    a [nb][maxvec][p] complex or None, nvec, counts, stats, select as the entry left it)."""
    nb, p, n = len(Ps), len(Ps[0].Ts), Ps[0].Ts[0].shape[0]
    Ts = [np.asfortranarray(t, dtype=fam.dtype) for P in Ps for t in P.Ts]
    Zs = [np.asfortranarray(z, dtype=fam.dtype) for P in Ps for z in P.Z]
    vals = _values(fam, Ps)
    sel = np.ascontiguousarray(np.broadcast_to(np.asarray(select, dtype=bool), (nb, n)), dtype=np.uint8)
    nvec = (C.c_int * nb)()
    cnts = np.zeros((nb, 3), dtype=np.int32)
    st = psd_amd.BevecStats()
    info = C.c_int(0)
    fn = fam.entry(eng, "eigvecs_batch")
    head = [eng.ctx, nb, n, p, eng._ptrs(Ts), eng._ptrs(Zs), *_entry_args(fam, Ps, vals), Ps[0].orientation.encode(),
            Ps[0].schurindex, sel.ctypes.data_as(C.POINTER(C.c_uint8)), int(shifted)]
    tail = [nvec, cnts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st), C.byref(info)]
    fn(*head, None, 0, *([None] if fam.signed else []), *tail)  # the size query: select completed, nvec filled
    assert info.value == 0 and st.nlaunch == 0
    if maxvec is None:
        maxvec = max(nvec)
    nmat = p if shifted else 1
    V = np.full((nb, nmat, maxvec, n), 7.0 + 7.0j)  # (poisoned: the padding has to be written)
    a = np.full((nb, maxvec, p), 7.0 + 7.0j) if fam.signed else None
    Vp = (C.c_void_p * (nb * nmat))(*[V[q, l].ctypes.data for q in range(nb) for l in range(nmat)])
    rc = fn(*head, Vp, maxvec, *([a.ctypes.data_as(C.POINTER(C.c_double))] if fam.signed else []), *tail)
    assert rc == info.value
    return info.value, V, a, list(nvec), cnts, st, sel


# ------------------------------------------------------------------------------------------------
# 1. mixed batch
def mixed_problems(fam=D):
    return _shared("mixed", lambda: [fam.form(7, 3, fam.seeds[q], fam.mixed_pairs[q], "L") for q in range(5)], fam)


def case_mixed(eng, fam):
    probs = mixed_problems(fam)
    Ps = [P for P, _ in probs]
    select, nvec0 = fam.mixed_select, fam.mixed_nvec
    keep = [[x.copy() for x in list(P.Ts) + list(P.Z)] for P in Ps]
    out = check_batch(eng, fam, probs, select)
    assert [vectors(fam, r)[0].shape[1] for r in out] == nvec0
    one = run(eng, fam, Ps, select, shifted=False)
    for q in range(5):
        V1 = vectors(fam, one[q])
        assert len(V1) == 1 and np.array_equal(V1[0], vectors(fam, out[q])[0])  # bit-identical
        assert not fam.signed or np.array_equal(one[q][1], out[q][1])
        if fam is D:  # (DG: check_signed has looked)
            for V in out[q]:  # the partner of a pair is the exact conjugate
                lam = vc.order_values(Ps[q], select[q])
                for c in range(len(lam) - 1):
                    if lam[c].imag > 0:
                        assert np.array_equal(V[:, c + 1], np.conj(V[:, c]))
    assert all(np.array_equal(x, y) for P, k in zip(Ps, keep) for x, y in zip(list(P.Ts) + list(P.Z), k))
    # the blocks as the ABI leaves them: n x maxvec, the columns at and beyond nvec exactly zero, in V and in a; select
    # completed to whole pairs
    info, V, a, nvec, cnts, st, sel = raw_host(eng, fam, Ps, select)
    assert info == 0 and nvec == nvec0 and V.shape[2] == 7
    for q in range(5):
        assert np.array_equal(sel[q].astype(bool), completed(Ps[q], select[q]))
        for l in range(3):
            assert np.array_equal(V[q, l, :nvec[q]].T, vectors(fam, out[q])[l])
            assert np.all(V[q, l, nvec[q]:] == 0)
        if fam.signed:
            assert np.array_equal(a[q, :nvec[q]].T, out[q][1]) and np.all(a[q, nvec[q]:] == 0)
    assert st.nb == 5 and st.nvec_total == sum(nvec0) and not cnts.any()
    if fam.signed:
        assert st.ngroups == 1 and st.nlaunch == 4 and st.nperturbed == 0 and st.nrescaled == 0 and st.nzero == 0


# ------------------------------------------------------------------------------------------------
# 2. batch independence, bit for bit
def independence_problems(fam=D):
    lr = "R" if fam.signed else "L"
    base = _shared("indep", lambda: [fam.form(6, 2, fam.seeds[k], fam.indep_pairs[k], lr) for k in range(5)], fam)
    return [base[q % 5] for q in range(70)]  # (70 crosses any grouping of 32 or 64 units or problems)


def case_independence(eng, fam, eng_groups=None):
    """the whole batch run twice, the same problem at every place of it, a problem alone (first, middle, last), the batch
    rotated and reversed, and under PSD_BATCH_GROUP=3: the same bits"""
    probs = independence_problems(fam)
    Ps = [P for P, _ in probs]
    select = np.ones(6, dtype=bool)
    whole = run(eng, fam, Ps, select)
    again = run(eng, fam, Ps, select)
    assert all(_same(fam, x, y) for x, y in zip(whole, again))
    for q in range(5):
        check_one(eng, fam, Ps[q], probs[q][1], whole[q], select)
    for q in range(70):  # the same problem at another place
        assert _same(fam, whole[q], whole[q % 5]), q
    for pos in (0, 33, 69):
        alone = run(eng, fam, [Ps[pos]], select)
        assert _same(fam, alone[0], whole[pos]), pos
    turned = run(eng, fam, Ps[33:] + Ps[:33], select)
    assert _same(fam, turned[0], whole[33]) and _same(fam, turned[36], whole[69]) and _same(fam, turned[37], whole[0])
    turned = run(eng, fam, Ps[::-1], select)
    assert all(_same(fam, turned[69 - q], whole[q]) for q in range(70))
    if eng_groups is not None:
        parts = run(eng_groups, fam, Ps, select)
        assert eng_groups.eigvecs_batch_stats.ngroups == 24
        assert all(_same(fam, x, y) for x, y in zip(whole, parts))


# ------------------------------------------------------------------------------------------------
# 3. factor and lane layouts
def case_layout(eng, fam, shape, lr="L"):
    """the shapes of fam.layouts, three problems each, every row selected; signed: in both orientations, with a signature
    of both senses wherever p > 1"""
    p, n = shape[:2]
    assert not fam.signed or p == 1 or len(set(sig(p))) == 2
    pairs = fam.layout_pairs(shape)
    probs = _shared(("layout", shape) + ((lr,) if fam.signed else ()),
                    lambda: [fam.form(n, p, fam.seeds[q], pairs[q], lr) for q in range(3)], fam)
    out = check_batch(eng, fam, probs, np.ones(n, dtype=bool))
    assert all(vectors(fam, r)[0].shape[1] == n for r in out)


def case_all_false(eng, fam, lr):
    """signed: every factor inverted (DG: the quasi-triangular one too)"""
    p, n = 5, 9
    probs = _shared(("allfalse", lr), lambda: [fam.form(n, p, s, (0, 4, 7), lr, S=[False] * p) for s in fam.seeds[:3]], fam)
    check_batch(eng, fam, probs, np.ones(n, dtype=bool))


# ------------------------------------------------------------------------------------------------
# 4. depth and cap
def depth_problems(fam=D, lr="L"):
    n, p = 40, 3
    return _shared(("depth", lr) if fam.signed else "depth",
                   lambda: [fam.form(n, p, s, fam.depth_pairs, lr, diag=fam.depth_diag and fam.depth_diag(n, p))
                            for s in fam.depth_seeds], fam)


def case_depth(eng, fam, lr="L"):
    probs = depth_problems(fam, lr)
    for select in fam.depth_selects:
        check_batch(eng, fam, probs, select)


def case_above_cap(eng, fam):
    """unsigned: one order above the cap of the batched kernel, the per-problem fallback"""
    n, p = bcm.cap(fam.cap_header, fam.cap_macro) + 1, 2
    probs = _shared(("cap", n), lambda: [fam.form(n, p, s, (5, 23, n - 3), diag=fam.depth_diag and fam.depth_diag(n, p))
                                         for s in fam.depth_seeds[:2]], fam)
    select = np.zeros((2, n), dtype=bool)
    select[0] = np.arange(n) % 4 == 1  # (D: with the first pair and the last; nvec differs: the staging into n x maxvec)
    select[1] = np.arange(n) % 8 == 0
    check_batch(eng, fam, probs, select)


def _cap_diag(n, seed):
    rs = np.random.RandomState(2000 + seed)
    return [np.linspace(0.7, 1.6, n) ** (1 if l == 0 else -1) * np.exp(1j * rs.uniform(-np.pi, np.pi, n)) for l in range(2)]


def case_cap(eng, fam, n, lr):
    """signed.  n = 128: the largest order of the batched kernel; n = 129: the per-problem fallback.  The same gates."""
    def make():
        return [fam.form(n, 2, s, (10, 63, n - 2), lr, diag=_cap_diag(n, s) if fam.cplx else None) for s in fam.seeds[:2]]
    probs = _shared(("cap", n, lr), make, fam)
    rows, total = ([0, 63, n - 1], 6) if fam.cplx else ([0, 11, 63, n - 1], 14)  # (DG: rows 11 and n - 1 stand in pairs)
    select = np.zeros(n, dtype=bool)
    select[rows] = True
    check_batch(eng, fam, probs, select)
    assert eng.eigvecs_batch_stats.nvec_total == total
    assert (eng.eigvecs_batch_stats.nlaunch == 4) == (n <= 128)


# ------------------------------------------------------------------------------------------------
# 5. special columns inside a batch, unsigned
def case_special_negative(eng):
    """D: evec_cases.case_negative_even_p beside an ordinary problem"""
    n, p = 6, 4
    diag = [np.linspace(1.0, 2.0, n) for _ in range(p)]
    diag[1] = diag[1].copy()
    diag[1][2] = -1.3
    probs = _shared("neg", lambda: [plain_form(n, p, 7, (4,)), vc.schur_form(n, p, diag, seed=5, pairs=(4,))])
    Vs = check_batch(eng, D, probs, np.ones(n, dtype=bool))
    assert np.abs(Vs[1][0][:, 2].imag).max() < 1e-12 and np.abs(Vs[1][1][:, 2].imag).max() > 1e-3
    assert not eng.eigvecs_batch_counts.any()


def case_special_repeated(eng, fam):
    n, p = 6, 3
    probs = _shared("rep", lambda: [fam.form(n, p, 7, diag=[np.full(n, 1.5) for _ in range(p)]), fam.form(n, p, 9)], fam)
    select = np.ones(n, dtype=bool)
    Vs = run(eng, fam, [ps for ps, _ in probs], select)
    cnt = eng.eigvecs_batch_counts
    assert all(np.isfinite(V).all() for V in Vs[0]) and Vs[0][0].shape[1] == n
    assert cnt[0, 0] > 0 and cnt[0, 1] == 0 and cnt[0, 2] == 0 and not cnt[1].any()
    assert eng.eigvecs_batch_stats.nperturbed == cnt[0, 0]
    vc.check_columns(probs[1][0], Vs[1], select, probs[1][1])


def case_special_zero(eng, fam):
    n, p = 6, 3
    diag = zdiag(n, p, 9) if fam.cplx else [np.linspace(1.0, 2.0, n) for _ in range(p)]
    diag[0] = diag[0].copy()
    diag[0][3] = 0.0
    probs = _shared("zero", lambda: [fam.form(n, p, 7), fam.form(n, p, 9, diag=diag), fam.form(n, p, 5)], fam)
    select = np.ones(n, dtype=bool)
    Vs = run(eng, fam, [ps for ps, _ in probs], select)
    cnt = eng.eigvecs_batch_counts
    assert cnt[:, 2].tolist() == [0, 1, 0] and eng.eigvecs_batch_stats.nzero == 1
    assert all(np.isnan(V[:, 3]).all() for V in Vs[1])
    keep = [0, 1, 2, 4, 5]
    assert vc.relation_ratio(probs[1][1], [V[:, keep] for V in Vs[1]], np.asarray(probs[1][0].values)[keep]) <= fam.gate
    for q in (0, 2):  # the NaNs stay in their problem
        vc.check_columns(probs[q][0], Vs[q], select, probs[q][1])


def case_special_rescale(eng, fam):
    """diagonals graded over 2^+-175 inside the period (Z: with complex phases)"""
    n, p = 8, 6
    rs = np.random.RandomState(1000 + 23)
    diag = []
    for l in range(p):
        g = np.where(np.arange(n) % 2 == 1, 2.0 ** (175 if l < 3 else -175), 1.0)
        d = np.linspace(1.0, 1.7, n) ** (1.0 / p) * g
        diag.append(d * np.exp(1j * rs.uniform(-np.pi, np.pi, n)) if fam.cplx else d)
    probs = _shared("resc", lambda: [fam.form(n, p, 5), fam.form(n, p, 23, diag=diag)], fam)
    select = np.ones(n, dtype=bool)
    Vs = run(eng, fam, [ps for ps, _ in probs], select)
    cnt = eng.eigvecs_batch_counts
    assert cnt[1, 1] > 0 and cnt[0, 1] == 0 and eng.eigvecs_batch_stats.nrescaled == cnt[1, 1]
    ps, As = probs[1]
    assert all(np.isfinite(V).all() for V in Vs[1])
    assert vc.relation_ratio(As, Vs[1], np.asarray(ps.values)) <= fam.gate
    ref = vc.backsub_ref(ps, select)
    for l in range(p):
        for c in range(n):
            err = np.linalg.norm(Vs[1][l][:, c] - ref[l][:, c])
            assert err <= 1e-9 * np.linalg.norm(ref[l][:, c]), (l, c, err)
    vc.check_columns(probs[0][0], Vs[0], select, probs[0][1])


# ------------------------------------------------------------------------------------------------
# 6. special columns inside a batch, signed
def case_zero_infinite(eng, fam, lr):
    """zero diagonal entries on 1x1 rows of a forward and of an inverted factor (DG: a pair above and below them)"""
    n, p = 7, 4
    S = [True, False, True, False]
    pairs = (0, 5)
    rs = np.random.RandomState(53)
    diag = zgdiag(n, p, 7) if fam.cplx else [1.0 + rs.rand(n) for _ in range(p)]
    diag[0][2] = 0.0  # zero eigenvalue at row 2
    diag[1][4] = 0.0  # infinite eigenvalue at row 4
    probs = _shared(("zeroinf", lr), lambda: [fam.form(n, p, 5, pairs, lr, S=S),
                                              fam.form(n, p, 7, pairs, lr, S=S, diag=diag),
                                              fam.form(n, p, 9, pairs, lr, S=S)], fam)
    select = np.ones(n, dtype=bool)
    out = run(eng, fam, [P for P, _ in probs], select)
    cnt = eng.eigvecs_batch_counts.copy()
    nzero = eng.eigvecs_batch_stats.nzero
    assert cnt.tolist() == [[0, 0, 0], [0, 0, 2], [0, 0, 0]] and nzero == 2
    if fam.vs_single:
        assert single(eng, probs[1][0], select)[2][2] == 2
    for q in range(3):  # (the prototype is not used on the singular problem, as in gevec_cases.case_zero_infinite)
        check_one(eng, fam, probs[q][0], probs[q][1], out[q], select, proto=q != 1)
    Vs, a = out[1]
    As = probs[1][1]
    left = lr == "L"
    v_zero = Vs[0][:, 2] if left else Vs[1][:, 2]  # A_1 v_1 = 0 ('L'), A_1 v_2 = 0 ('R')
    assert np.linalg.norm(As[0] @ v_zero) <= fam.gate * np.linalg.norm(As[0]) * np.linalg.norm(v_zero)
    v_inf = Vs[2][:, 4] if left else Vs[1][:, 4]  # A_2 v_3 = 0 ('L'), A_2 v_2 = 0 ('R')
    assert np.linalg.norm(As[1] @ v_inf) <= fam.gate * np.linalg.norm(As[1]) * np.linalg.norm(v_inf)
    assert a[0, 2] == 0 and a[1, 4] == 0


def case_repeated(eng, fam):
    n, p = 6, 4
    probs = _shared("rep", lambda: [fam.form(n, p, 7, diag=[np.full(n, 1.5 + 0j if fam.cplx else 1.5) for _ in range(p)]),
                                    fam.form(n, p, 9, (1, 4))], fam)
    select = np.ones(n, dtype=bool)
    out = run(eng, fam, [P for P, _ in probs], select)
    cnt = eng.eigvecs_batch_counts.copy()
    nperturbed = eng.eigvecs_batch_stats.nperturbed
    assert all(np.isfinite(V).all() for V in out[0][0]) and out[0][0][0].shape[1] == n
    print("repeated eigenvalue: perturbed pivots", cnt[0, 0])
    assert cnt[0, 0] > 0 and cnt[0, 1] == 0 and cnt[0, 2] == 0 and not cnt[1].any()
    assert nperturbed == cnt[0, 0]
    if fam.vs_single:
        assert cnt[0, 0] == single(eng, probs[0][0], select)[2][0]  # counted as by the single call
    check_one(eng, fam, probs[1][0], probs[1][1], out[1], select)


def case_rescale(eng, fam, lr):
    """the graded diagonals of gevec_cases.case_rescale (2^+-175 inside the period, each row's signed product moderate;
    ZG: times random phases).  Gated on the relations alone: the prototype's SVD null vector fails on this grading."""
    n, p = 8, 6
    S = gc.S_ALT(p)
    rs = np.random.RandomState(2000 + 23)
    diag = []
    for l in range(p):
        g = np.where(np.arange(n) % 2 == 1, 2.0 ** (175 if l < 3 else -175), 1.0)
        d = np.linspace(1.0, 1.7, n) ** (1.0 / p) * g
        d = d if S[l] else 1.0 / d
        diag.append(d * np.exp(1j * rs.uniform(-np.pi, np.pi, n)) if fam.cplx else d)
    probs = _shared(("resc", lr),
                    lambda: [fam.form(n, p, 5, (2,), lr, S=S), fam.form(n, p, 23, (), lr, S=S, diag=diag)], fam)
    select = np.ones(n, dtype=bool)
    out = run(eng, fam, [P for P, _ in probs], select)
    cnt = eng.eigvecs_batch_counts.copy()
    nrescaled = eng.eigvecs_batch_stats.nrescaled
    print("rescaled columns:", cnt[:, 1].tolist())
    assert cnt[1, 1] > 0 and cnt[0, 1] == 0 and nrescaled == cnt[1, 1]
    if fam.vs_single:
        assert cnt[1, 1] == single(eng, probs[1][0], select)[2][1]  # equal to the single call's
    check_one(eng, fam, probs[1][0], probs[1][1], out[1], select, proto=False)
    check_one(eng, fam, probs[0][0], probs[0][1], out[0], select)


# ------------------------------------------------------------------------------------------------
# 7. all-true signature
def _generalized(ps):
    n = ps.Ts[0].shape[0]
    return psd_amd.GeneralizedPeriodicSchur([True] * len(ps.Ts), ps.Ts, ps.Z, np.array(ps.values), np.ones(n),
                                            np.zeros(n, dtype=np.int32), ps.orientation, ps.schurindex)


def case_all_true_zg(eng):
    """against zeigvecs_batch on ordinary problems (the gates of gevec_cases.case_vs_eigvecs); a PeriodicSchur and a
    GeneralizedPeriodicSchur with S all true give the same bits"""
    n, p = 7, 3
    probs = [zform(n, p, s) for s in ZG.seeds[:3]]
    pss = [ps for ps, _ in probs]
    select = np.ones(n, dtype=bool)
    Vb = eng.zeigvecs_batch(pss, select)
    out = eng.zgeigvecs_batch(pss, select)
    assert eng.eigvecs_batch_stats.nlaunch == 4
    outg = eng.zgeigvecs_batch([_generalized(ps) for ps in pss], select)
    for q, (ps, As) in enumerate(probs):
        Vg, a = out[q]
        check_one(eng, ZG, ps, As, out[q], select)
        d = np.abs(Vg[0] - Vb[q][0]).max()
        print("all-true q=%d: max |V_1 - V_1(zeigvecs_batch)| = %.3e" % (q, d))
        assert np.allclose(Vg[0], Vb[q][0], rtol=0, atol=1e-10), d
        for l in range(p):
            vc._parallel(Vg[l], Vb[q][l])
        assert _same(ZG, outg[q], out[q])


def case_all_true_dg(eng):
    """an all-true signature runs this path too; a PeriodicSchur and a GeneralizedPeriodicSchur with S all true give the
    same bits"""
    n, p = 7, 3
    probs = _shared("alltrue", lambda: [dgform(n, p, s, DG.mixed_pairs[0], "L", S=[True] * p) for s in DG.seeds[:3]], DG)
    select = np.ones(n, dtype=bool)
    out = check_batch(eng, DG, probs, select)
    assert eng.eigvecs_batch_stats.nlaunch == 4
    pss = [psd_amd.PeriodicSchur(P.Ts, P.Z, np.array(P.values), P.orientation, P.schurindex) for P, _ in probs]
    outp = eng.dgeigvecs_batch(pss, select)
    assert all(_same(DG, x, y) for x, y in zip(out, outp))


# ------------------------------------------------------------------------------------------------
# 8. skipped problems
def case_skipped(eng, fam):
    """every second problem of the first three (signed: four) of the mixed batch unselected"""
    probs = mixed_problems(fam)[:4 if fam.signed else 3]
    Ps = [P for P, _ in probs]
    nb = len(Ps)
    full = run(eng, fam, Ps, np.ones(7, dtype=bool))
    select = np.ones((nb, 7), dtype=bool)
    select[1::2] = False
    out = run(eng, fam, Ps, select)
    for q in range(1, nb, 2):
        assert all(V.shape == (7, 0) for V in vectors(fam, out[q])) and (not fam.signed or out[q][1].shape == (3, 0))
    for q in range(0, nb, 2):
        assert _same(fam, out[q], full[q])
        if not fam.signed:
            vc.check_columns(Ps[q], out[q], select[q], probs[q][1])
    info, V, a, nvec, cnts, st, _ = raw_host(eng, fam, Ps, select)
    assert info == 0 and nvec == [7, 0, 7, 0][:nb] and st.nvec_total == 14
    for q in range(1, nb, 2):
        assert np.all(V[q] == 0) and (a is None or np.all(a[q] == 0))
    # nothing selected anywhere: nothing is launched
    none = run(eng, fam, Ps, np.zeros(7, dtype=bool))
    assert all(V.shape == (7, 0) for r in none for V in vectors(fam, r))
    assert eng.eigvecs_batch_stats.nlaunch == 0 and eng.eigvecs_batch_stats.nvec_total == 0
    info, V, a, nvec, cnts, st, _ = raw_host(eng, fam, Ps, np.zeros(7, dtype=bool), maxvec=2)
    assert info == 0 and nvec == [0] * nb and st.nlaunch == 0 and np.all(V == 0) and (a is None or np.all(a == 0))


# ------------------------------------------------------------------------------------------------
# 9. launch count
def case_launch_count(eng, fam):
    """the launches of a call depend neither on nb nor on n (below the cap): solve, V_1, norms, the other factors — four
    with shifted and p > 1, three otherwise, none when nothing is selected (the headers of psd_zgbevec_host.inl and
    psd_gbevec_host.inl).  The unsigned batches go through the checks as well."""
    n, pairs, sizes = fam.launch
    base = _shared("launch" if not fam.signed else "launch4",
                   lambda: [fam.form(n, 3, fam.seeds[k], pairs[k], "L") for k in range(len(pairs))], fam)
    counts = []
    for probs in [[base[q % len(base)] for q in range(nb)] for nb in sizes] + [depth_problems(fam, "L")]:
        select = np.ones(probs[0][0].Ts[0].shape[0], dtype=bool)
        if fam.signed:
            run(eng, fam, [P for P, _ in probs], select)
        else:
            check_batch(eng, fam, probs, select)
        counts.append(eng.eigvecs_batch_stats.nlaunch)
        assert eng.eigvecs_batch_stats.ngroups == 1
    assert counts[0] == counts[1] == counts[2] > 0 and fam.nlaunch in (None, counts[0]), counts
    if fam.nlaunch:
        run(eng, fam, [P for P, _ in base], np.ones(n, dtype=bool), shifted=False)
        assert eng.eigvecs_batch_stats.nlaunch == 3
    if fam.signed:
        one = _shared("launchp1", lambda: [fam.form(5, 1, 5, (2,), "L")], fam)
        run(eng, fam, [one[0][0]], np.ones(5, dtype=bool))
        assert eng.eigvecs_batch_stats.nlaunch == 3  # p = 1: no other factors
        run(eng, fam, [P for P, _ in base], np.zeros(n, dtype=bool))
        assert eng.eigvecs_batch_stats.nlaunch == 0


# ------------------------------------------------------------------------------------------------
# 10. pipeline
def case_pipeline(eng, fam, lr):
    """unsigned, device-resident: pschur_batch_ -> eigvecs_batch, against eigvecs_dev problem by problem"""
    import torch

    n, p, nb = 12, 3, 5
    facs = [pt.bench_factors(n, p, seed=91 + q, dtype=fam.dtype) for q in range(nb)]
    dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in facs])).cuda()
    Td, Zd, values, _ = fam.method(eng, "pschur_batch_")(dA, lr)
    si = p if lr == "L" else 1
    select = np.ones((nb, n), dtype=bool)
    select[1] = np.arange(n) % 2 == 0
    batch = fam.method(eng, "eigvecs_batch")
    V, nvec = batch(Td, Zd, values, select, lr=lr, schurindex=si)
    if fam.cplx:
        assert nvec.tolist() == [n, n // 2, n, n, n]
    assert V.is_cuda and tuple(V.shape) == (nb, p, n, int(max(nvec)))
    Vh, Th, Zh = V.cpu().numpy(), Td.cpu().numpy(), Zd.cpu().numpy()
    for q in range(nb):
        ps = psd_amd.PeriodicSchur([np.asfortranarray(Th[q, l]) for l in range(p)],
                                   [np.asfortranarray(Zh[q, l]) for l in range(p)], values[q], lr, si)
        Vs = [Vh[q, l][:, :nvec[q]] for l in range(p)]
        assert np.all(Vh[q][:, :, nvec[q]:] == 0)
        lams = np.asarray(values[q])[select[q]] if fam.cplx else vc.order_values(ps, select[q])
        assert Vs[0].shape[1] == len(lams)
        vc.ec.ev_check(facs[q], Vs, lams, left=(lr == "L"))
        r = vc.relation_ratio(facs[q], Vs, lams, left=(lr == "L"))
        assert r <= fam.gate, (lr, q, r)
        one = eng.eigvecs_dev(Td[q].transpose(1, 2).contiguous(), Zd[q].transpose(1, 2).contiguous(), values[q],
                              select[q], lr=lr, schurindex=si)
        for l in range(p):
            d = np.abs(Vs[l] - one[l].cpu().numpy()).max()
            if fam.cplx:
                print("pipeline %s q=%d l=%d: max |V_batch - V_single| = %.3e" % (lr, q, l, d))
            assert d <= 1e-9, (lr, q, l, d)
    V1, nvec1 = batch(Td, Zd, values, select, lr=lr, schurindex=si, shifted=False)
    assert tuple(V1.shape) == (nb, 1, n, int(max(nvec))) and torch.equal(V1[:, 0], V[:, 0])
    assert nvec1.tolist() == nvec.tolist()
    if fam.cplx:
        with pytest.raises(TypeError):
            batch(Td.real.contiguous(), Zd.real.contiguous(), values, select, lr=lr, schurindex=si)
        with pytest.raises(TypeError):
            batch(Td, Zd.real.contiguous(), values, select, lr=lr, schurindex=si)
        with pytest.raises(psd_amd.NotImplementedPSD, match="zeigvecs_batch"):
            eng.eigvecs_batch(Td, Zd, values, select, lr=lr, schurindex=si)


def _represented(S, lr, Ts, Zs):
    """the factors a decomposition represents (as gevec_cases.case_end_to_end builds them)"""
    p = len(S)
    As = []
    for l in range(p):
        ln = (l + 1) % p
        fwd = bool(S[l]) == (lr == "L")
        As.append(Zs[ln] @ Ts[l] @ Zs[l].conj().T if fwd else Zs[l] @ Ts[l] @ Zs[ln].conj().T)
    return As


def _pipeline_inputs(fam, n, p, nb):
    return [pt.bench_factors(n, p, seed=191 + q, dtype=fam.dtype) for q in range(nb)]


def _lead(values):
    """the eigenvalues inside the unit circle, and the leading rows they occupy after the reordering"""
    inside = np.abs(values) < 1
    return inside, np.arange(len(values)) < inside.sum()


def case_pipeline_host(eng, fam, lr):
    """signed: gpschur_batch -> gordschur_batch_ (|lambda| < 1 first) -> geigvecs_batch on the leading rows, host forms"""
    n, p, nb = 8, 3, 6
    S = [True, False, True]
    pss = fam.method(eng, "pschur_batch")(_pipeline_inputs(fam, n, p, nb), S, lr)
    sels = [_lead(ps.values) for ps in pss]
    fam.method(eng, "ordschur_batch_")(pss, np.array([s[0] for s in sels]))
    lead = np.array([s[1] for s in sels])
    out = run(eng, fam, pss, lead)
    for q, ps in enumerate(pss):
        assert ps.S == S and out[q][0][0].shape == (n, lead[q].sum())
        assert ps.Ts[0].dtype == fam.dtype and ps.Z[0].dtype == fam.dtype
        check_one(eng, fam, ps, _represented(S, lr, ps.Ts, ps.Z), out[q], lead[q], proto=False, vs_single=False)


def case_pipeline_signed(eng, fam, lr):
    """the same, device-resident: no matrix touches the host between the three calls"""
    import torch

    n, p, nb = 8, 3, 6
    S = [True, False, True]
    si = p if lr == "L" else 1
    batch = fam.method(eng, "eigvecs_batch")
    dA = torch.from_numpy(np.array([[np.array(x) for x in A] for A in _pipeline_inputs(fam, n, p, nb)])).cuda()
    Td, Zd, values, _ = fam.method(eng, "pschur_batch_")(dA, S, lr)
    sels = [_lead(v) for v in values]
    Td, Zd, values, _ = fam.method(eng, "ordschur_batch_")(Td, Zd, np.array([s[0] for s in sels]), S=S, lr=lr, schurindex=si)
    lead = np.array([s[1] for s in sels])
    V, a, nvec = batch(Td, Zd, lead, S=S, lr=lr, schurindex=si)
    if not fam.cplx:
        assert eng.eigvecs_batch_stats.nlaunch == 5  # (the gather of the device entry, then four)
    mv = int(lead.sum(axis=1).max())
    assert nvec.tolist() == lead.sum(axis=1).tolist() and nvec.dtype == np.int32
    assert V.is_cuda and V.dtype == torch.complex128 and tuple(V.shape) == (nb, p, n, mv)
    assert a.shape == (nb, p, mv) and a.dtype == np.complex128
    Vh, Th, Zh = V.cpu().numpy(), Td.cpu().numpy(), Zd.cpu().numpy()
    for q in range(nb):
        assert np.all(Vh[q][:, :, nvec[q]:] == 0) and np.all(a[q][:, nvec[q]:] == 0)
        P = psd_amd.GeneralizedPeriodicSchur(S, [np.asfortranarray(Th[q, l]) for l in range(p)],
                                             [np.asfortranarray(Zh[q, l]) for l in range(p)], values[q], np.ones(n),
                                             np.zeros(n, dtype=np.int32), lr, si)
        got = ([Vh[q, l][:, :nvec[q]] for l in range(p)], a[q][:, :nvec[q]])
        check_one(eng, fam, P, _represented(S, lr, P.Ts, P.Z), got, lead[q], proto=False, vs_single=False)
    V1, a1, nvec1 = batch(Td, Zd, lead, S=S, lr=lr, schurindex=si, shifted=False)
    assert tuple(V1.shape) == (nb, 1, n, mv) and torch.equal(V1[:, 0], V[:, 0]) and np.array_equal(a1, a)
    assert nvec1.tolist() == nvec.tolist()
    # the other element type (DG names the entry for it)
    other = (Td.real.contiguous(), Zd.real.contiguous()) if fam.cplx else (Td.to(torch.complex128), Zd.to(torch.complex128))
    with pytest.raises(TypeError, match=None if fam.cplx else "zgeigvecs_batch"):
        batch(*other, lead, S=S, lr=lr, schurindex=si)
    with pytest.raises(psd_amd.DimensionMismatch):
        batch(Td, Zd, lead, S=S[:-1], lr=lr, schurindex=si)
    with pytest.raises(ValueError):
        batch(Td, None, lead, S=S, lr=lr, schurindex=si)
    with pytest.raises(ValueError, match="argument 9"):
        batch(Td, Zd, lead[:, :-1], S=S, lr=lr, schurindex=si)


# ------------------------------------------------------------------------------------------------
# 11. gpschur_batch end to end, signed
def case_gpschur_batch(eng, fam):
    """four pencils (A, B) of order 6 (DG: real=True): the deflating vectors of each, against the factors its decomposition
    represents"""
    n = 6
    As = [pt.bench_factors(n, 1, seed=300 + 17 * q, dtype=fam.dtype) for q in range(4)]
    Bs = [pt.bench_factors(n, 1, seed=5300 + 17 * q, dtype=fam.dtype) for q in range(4)]
    pss = eng.gpschur_batch(As, Bs) if fam.cplx else eng.gpschur_batch(As, Bs, real=True)
    select = np.ones(n, dtype=bool)
    out = run(eng, fam, pss, select)
    for q, ps in enumerate(pss):
        assert ps.period == 2 and not all(ps.S) and ps.Ts[0].dtype == fam.dtype
        check_one(eng, fam, ps, _represented(ps.S, ps.orientation, ps.Ts, ps.Z), out[q], select, proto=False,
                  vs_single=False)


# ------------------------------------------------------------------------------------------------
# 12. errors
def case_errors(eng, fam, make_engine):
    probs = mixed_problems(fam)
    Ps = [P for P, _ in probs]
    n, p = 7, 3
    batch = fam.method(eng, "eigvecs_batch")

    def variant(P, S=None, Z=None, si=None):
        Z, si = P.Z if Z is None else Z, P.schurindex if si is None else si
        if fam.signed:
            return psd_amd.GeneralizedPeriodicSchur(P.S if S is None else S, P.Ts, Z, P.alpha, P.beta, P.alphascale,
                                                    P.orientation, si)
        return psd_amd.PeriodicSchur(P.Ts, Z, P.values, P.orientation, si)

    with pytest.raises(ValueError, match="argument 9"):
        batch(Ps, [True] * (n - 1))
    with pytest.raises(ValueError, match="argument 9"):
        batch(Ps, np.ones((4, n), dtype=bool))
    with pytest.raises(ValueError, match="argument 8"):
        batch([variant(Ps[1], si=p + 1)] * 2, [True] * n)  # schurindex outside the period
    with pytest.raises(psd_amd.DimensionMismatch):
        batch([Ps[0], variant(Ps[1], si=1 if fam.signed else p + 1)], [True] * n)  # unequal schurindex
    with pytest.raises(psd_amd.DimensionMismatch):
        batch([Ps[0], fam.form(6, p, 5)[0]], [True] * n)  # unequal order
    with pytest.raises(ValueError):
        batch([variant(Ps[0], Z=[])], [True] * n)  # no Schur vectors
    g = psd_amd.GeneralizedPeriodicSchur([True, False, True], Ps[0].Ts, Ps[0].Z, np.array(Ps[0].values), np.ones(n),
                                         np.zeros(n, dtype=np.int32), "L", p)
    if fam.signed:
        with pytest.raises(psd_amd.DimensionMismatch, match="signatures"):
            batch([Ps[0], variant(Ps[1], S=[True, True, False])], [True] * n)  # unequal S
        with pytest.raises(psd_amd.DimensionMismatch):
            batch([variant(Ps[0], S=[True, False])] * 2, [True] * n)  # S length
        other = gc.signed_form(n, p, [True, False, True], "L", seed=3, cplx=not fam.cplx)[0]
        with pytest.raises(TypeError, match="zgeigvecs_batch"):
            batch([other], [True] * n)  # the other element type
        with pytest.raises(TypeError):
            batch(Ps, [True] * n, [True] * n)
        if not fam.cplx:
            with pytest.raises(TypeError, match="use geigvecs per problem for a Float64 decomposition"):
                eng.zgeigvecs_batch(Ps, [True] * n)  # (the complex entry's message stays)
        with pytest.raises(psd_amd.NotImplementedPSD):
            (Z if fam.cplx else D).method(eng, "eigvecs_batch")(Ps, [True] * n)  # the unsigned entry refuses a signed one
        assert batch([], [True] * n) == []
        assert eng.eigvecs_batch_stats.nb == 0 and eng.eigvecs_batch_counts.shape == (0, 3)
    else:
        with pytest.raises(psd_amd.DimensionMismatch):
            batch([Ps[0], fam.form(n, 2, 5)[0]], [True] * n)  # unequal period
        if fam.cplx:
            real = plain_form(n, p, 5)[0]
            with pytest.raises(TypeError, match="eigvecs_batch"):
                batch([real], [True] * n)  # Float64: the real entry
            with pytest.raises(psd_amd.NotImplementedPSD, match="zeigvecs_batch"):
                eng.eigvecs_batch([Ps[0]], [True] * n)  # ... which still refuses ComplexF64, naming this one
            mixed = vc._clone(Ps[0])
            mixed.Z = [np.asfortranarray(z.real) for z in mixed.Z]
            with pytest.raises(TypeError):
                batch([mixed], [True] * n)  # complex T with real Z
            mixed = vc._clone(real)
            mixed.Z = [z.astype(np.complex128) for z in mixed.Z]
            with pytest.raises(TypeError):
                batch([mixed], [True] * n)  # real T with complex Z
            # an all-true signature is the plain decomposition (alpha / beta * 2^ascale its eigenvalues)
            gt = psd_amd.GeneralizedPeriodicSchur([True] * p, Ps[0].Ts, Ps[0].Z, 0.5 * np.array(Ps[0].values),
                                                  np.full(n, 2.0), np.full(n, 2, dtype=np.int32), "L", p)
            sel = [True, False, True, False, False, True, True]
            assert _same(fam, batch([gt], sel)[0], batch([Ps[0]], sel)[0])
        else:
            with pytest.raises(psd_amd.NotImplementedPSD):
                batch([vc.schur_form(n, p, [np.linspace(1.0, 2.0, n)] * p, seed=5, cplx=True)[0]], [True] * n)
            bad = vc._clone(Ps[0])
            bad.Z = [z.astype(np.complex128) for z in bad.Z]
            with pytest.raises(TypeError):
                batch([bad], [True] * n)
        with pytest.raises(psd_amd.NotImplementedPSD):
            batch([Ps[0], g], [True] * n)
        assert batch([], [True] * n) == []
    info, V, a, nvec, _, _, _ = raw_host(eng, fam, Ps, fam.mixed_select, maxvec=6)  # problem 0 has 7 columns
    assert info == -10 and nvec == fam.mixed_nvec
    sharded = make_engine()
    sharded.set_shard(0, 2)
    with pytest.raises(psd_amd.NotImplementedPSD):
        fam.method(sharded, "eigvecs_batch")(Ps, [True] * n)


# ------------------------------------------------------------------------------------------------
# 13. both entries through the C ABI (simulated tier)
def case_dev_abi(eng, fam):
    """The family's device entry through the C ABI on packed blocks (in the simulation device memory is host memory): the
    same bits as the host entry, its launches (fam.dev_nlaunch; signed: one for the gather of the scalars), and the
    argument codes of both entries."""
    probs = mixed_problems(fam)
    Ps = [P for P, _ in probs]
    nb, n, p = 5, 7, 3
    select, nvec0 = fam.mixed_select, fam.mixed_nvec
    host = run(eng, fam, Ps, select)
    dT = np.ascontiguousarray(np.array([pt.pack(P.Ts, fam.dtype) for P in Ps]))
    dZ = np.ascontiguousarray(np.array([pt.pack(P.Z, fam.dtype) for P in Ps]))
    vals = _values(fam, Ps)
    sc = np.zeros((nb, n), dtype=np.int32)
    sel = np.ascontiguousarray(select, dtype=np.uint8)
    done = np.array([completed(P, s) for P, s in zip(Ps, select)], dtype=np.uint8)
    dp, u8p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    nvec = (C.c_int * nb)()
    cnts = np.zeros((nb, 3), dtype=np.int32)
    st = psd_amd.BevecStats()
    info = C.c_int(0)
    ctx, selp = eng.ctx, sel.ctypes.data_as(u8p)
    mid = _entry_args(fam, Ps, vals, sc.ctypes.data_as(i32p))
    dev, hst = fam.entry(eng, "eigvecs_batch_dev"), fam.entry(eng, "eigvecs_batch")
    bT, bZ = C.c_void_p(dT.ctypes.data), C.c_void_p(dZ.ctypes.data)
    tail = [nvec, cnts.ctypes.data_as(i32p), C.byref(st), C.byref(info)]

    def scal(a):
        """the scalars' place in a signed entry's arguments"""
        return [a] if fam.signed else []
    rc = dev(ctx, nb, n, p, bT, bZ, *mid, b"L", p, selp, 1, None, 0, *scal(None), *tail)  # the size query
    assert rc == 0 and list(nvec) == nvec0 and np.array_equal(sel, done)  # select completed in place
    if fam.signed:
        assert st.nlaunch == (0 if fam.cplx else 1)  # (DG: the gather alone)
    V = np.full((nb, p, 7, n), 7.0 + 7.0j)
    a = np.full((nb, 7, p), 7.0 + 7.0j)
    rc = dev(ctx, nb, n, p, bT, bZ, *mid, b"L", p, selp, 1, C.c_void_p(V.ctypes.data), 7, *scal(a.ctypes.data_as(dp)), *tail)
    assert rc == 0 and info.value == 0 and st.nb == nb and st.ngroups == 1 and st.nlaunch == fam.dev_nlaunch
    assert st.ms_kernels >= st.ms_solve >= 0
    for q in range(nb):
        for l in range(p):
            assert np.array_equal(V[q, l, :nvec[q]].T, vectors(fam, host[q])[l]) and np.all(V[q, l, nvec[q]:] == 0)
        if fam.signed:
            assert np.array_equal(a[q, :nvec[q]].T, host[q][1]) and np.all(a[q, nvec[q]:] == 0)
    if fam.signed:
        # without the scalars (ZG: no gather; DG, shifted = 0: the gather, then three).  (S = NULL: all true, another
        # problem; the launches are what is looked at)
        V2 = np.full((nb, p, 7, n), 7.0 + 7.0j)
        rc = dev(ctx, nb, n, p, bT, bZ, None, b"L", p, selp, 1 if fam.cplx else 0, C.c_void_p(V2.ctypes.data), 7, None,
                 *tail)
        assert rc == 0 and st.nlaunch == 4
    if fam is DG:
        sel0 = np.zeros((nb, n), dtype=np.uint8)  # nothing selected: no launch, the gather included
        rc = dev(ctx, nb, n, p, bT, bZ, *mid, b"L", p, sel0.ctypes.data_as(u8p), 1, C.c_void_p(V2.ctypes.data), 7,
                 a.ctypes.data_as(dp), *tail)
        assert rc == 0 and st.nlaunch == 0 and not any(nvec) and np.all(V2 == 0) and np.all(a == 0)
    for q in range(nb):  # the inputs stay as they were
        assert np.array_equal(dT[q], pt.pack(Ps[q].Ts, fam.dtype)) and np.array_equal(dZ[q], pt.pack(Ps[q].Z, fam.dtype))
    assert all(np.array_equal(x, y) for x, y in zip(vals, _values(fam, Ps)))

    Tp = eng._ptrs([np.asfortranarray(t, dtype=fam.dtype) for P in Ps for t in P.Ts])
    Zp = eng._ptrs([np.asfortranarray(z, dtype=fam.dtype) for P in Ps for z in P.Z])

    def entry(fn, T0, Z0):
        def f(c_=ctx, nb_=nb, n_=n, p_=p, T_=T0, Z_=Z0, mid_=mid, o=b"L", si=p, sel_=selp, V_=None, mv=0, nv=nvec):
            return fn(c_, nb_, n_, p_, T_, Z_, *mid_, o, si, sel_, 1, V_, mv, *scal(None), nv, None, None, None)
        return f
    dev_, host_ = entry(dev, bT, bZ), entry(hst, Tp, Zp)
    for f in (dev_, host_):
        assert f() == 0
        assert f(c_=None) == -1 and f(n_=0) == -2 and f(p_=0) == -3 and f(T_=None) == -4 and f(Z_=None) == -5
        for k in range(0 if fam.signed else 2):  # (wr / alpha, wi / beta)
            if fam.cplx or k == 0:
                assert f(mid_=mid[:k] + [None] + mid[k + 1:]) == -6
        assert f(o=b"X") == -7 and f(si=0) == -8 and f(si=p + 1) == -8
        assert f(sel_=None) == -9 and f(nb_=-1) == -11 and f(nv=None) == -12
        none = mid if fam.signed else [None, None] + mid[2:]
        assert f(nb_=0, T_=None, Z_=None, mid_=none, sel_=None, nv=None) == 0  # nb == 0 touches nothing
    assert dev_(V_=C.c_void_p(V.ctypes.data), mv=6) == -10
    Vp = (C.c_void_p * (nb * p))(*[V[q, l].ctypes.data for q in range(nb) for l in range(p)])
    assert host_(V_=Vp, mv=6) == -10
    # a period-sharded context keeps a slice of Z: both entries refuse it
    sharded = psd_amd.Engine(libpath=eng.lib._name)
    sharded.set_shard(0, 2)
    assert dev_(c_=sharded.ctx) == psd_amd.INFO_NOTIMPL and host_(c_=sharded.ctx) == psd_amd.INFO_NOTIMPL
