"""Cases for the batched reordering of the four families — Engine.[z|zg|dg]ordschur_batch_ / ordschur_batch
(psd_{d,z}_[g]ordschur_batch and ..._dev; csrc/psd_bord.h, psd_zbord.h, psd_zgbord.h, psd_gbord.h): many small periodic
Schur forms reordered in one call.  Each case takes an engine and a family (batch_common.Family);
tests/test_hostsim_*ordschur_batch.py run them on the serial simulation, tests/test_gpu_*ordschur_batch.py on the device.

Inputs are the family's pschur_batch results of pt.bench_factors — one signature per shape for the signed families,
reversed for 'L' — with the eigenvalues at or below the median modulus selected (row 2 alone for n = 2, where the median
rule selects both rows); they are computed once per library (the engines of a tier differ in knobs that leave
pschur_batch's bits alone: batch_cases.case_groups) and only cloned.  The oracle accepts every swap of every problem it
runs on (asserted): all of them for the unsigned families, the first six of a shape for the signed ones.

A case is one body where the families differ in names, element type, shapes, bounds or the presence of S: the
descriptors below hold those.  Where they check different things the functions stand side by side:

- Float64 results hold conjugate pairs as 2 x 2 blocks, which a selection has to take whole: closed_select, has_pair,
  the real structure checks of check_problem (batch_cases.real_form for DG), case_pairs (D), case_pairs_reference (DG),
  case_selections_d, and the rows of case_selections that select one member of a pair (DG).
- An all-true signature is the call of zordschur_batch_ for ZG (the same bits) and stays on the signed kernels for DG
  (the scaled form, the eigenvalues of ordschur_batch_ to 1e-9): case_all_true_zg, case_all_true_dg.
- The problem whose swap is rejected (one_fails_inputs): equal eigenvalues for the unsigned families; for ZG an exactly
  zero row of the Sylvester system, since under a signed S the system of an equal pair can be consistent; for DG small
  integers with a 2 x 2 block, which keeps the single call on the real driver and contraction out of the outcome — so DG
  alone asserts the code 3000, SingularException and factors left bit for bit.
- Above the cap the DG single call promotes a problem with a real spectrum to the complex kernel: those problems go
  through check_problem, the others get the single call's bits as in every other family (case_above_cap).
- The device-resident chain ends in eigvecs_batch for D alone, and DG alone gets the host entry's bits from it (the others
  1e-12: contraction may differ between the kernels of the two entries).

Differences between the families that nothing explains, left as they are:
- case_against_serial is run for Z and ZG only (the test files of D and DG have no such test).
- The window the engine chooses is asserted against expected_window for the signed families only; there is no model of
  the unsigned kernels' LDS use here.
- check_problem compares with the single call (1e-9 max|lambda|) for D and DG only, and prints the figure for DG only.
- That every single problem moves is asserted for D, Z and ZG; for DG per shape (problem 2 of the pencil needs no swap
  in 'L').
- test_gpu_ordschur_batch.py does not run case_dev_abi."""
import ctypes as C

import numpy as np
import pytest

import batch_cases as bc
import batch_common as bcm
import psd_amd
import psdtest as pt
from batch_cases import real_form
from batch_common import SIG22, SIG70, F, T, shape_id, sig  # noqa: F401 (used by the test files)
from engine_cases import _clone


def median_select(lam):
    n = len(lam)
    return np.abs(lam) <= np.sort(np.abs(lam))[n // 2]


def select_for(shape, lam):
    if shape[1] == 2:  # (the median rule selects both rows of an order-2 problem: nothing would move)
        return np.array([False, True])
    return median_select(lam)


def closed_select(lam0, select):
    """the selection closed under conjugation, as the device closes it"""
    closed = np.array(select, dtype=bool).copy()
    for i in range(len(lam0) - 1):
        if lam0[i].imag > 0 and (select[i] or select[i + 1]):
            closed[i] = closed[i + 1] = True
    return closed


def has_pair(ps):
    return bool(np.any(ps.values.imag != 0))


def gclone(ps):
    return psd_amd.GeneralizedPeriodicSchur(list(ps.S), [t.copy(order="F") for t in ps.Ts], [z.copy(order="F") for z in ps.Z],
                                            ps.alpha.copy(), ps.beta.copy(), ps.alphascale.copy(), ps.orientation,
                                            ps.schurindex)


def _zg_lds_bytes(p, w):
    """zgord_lds_bytes (csrc/psd_engine.cpp)"""
    return p * w * (w + 1) * 16 + 15 * p * 16 + (p + 2) * 8 + p * 4 + 64


def _dg_lds_bytes(p, w):
    """rord_lds_bytes (csrc/psd_engine.cpp) with psd_rord_tree_doubles (csrc/psd_rord.h)"""
    tree = (2 * p + 8) * 36 + 4 * 104 + 4 * 12 + (7 * p + 16 + 32 + 1) // 2 + 8
    return (p * w * (w + 1) + p * (96 + 52) + 4 + 192 + tree) * 8 + p * 5 + 80


def _equal_eigenvalues(dtype):
    """n = 4, p = 2: the problem of engine_cases.case_rordschur_edge / case_zordschur_edge — equal eigenvalues, the swap is
    rejected"""
    n, p = 4, 2
    Ts = [np.asfortranarray(np.triu(np.ones((n, n))).astype(dtype)) for _ in range(p)]
    Z = [np.asfortranarray(np.eye(n, dtype=dtype)) for _ in range(p)]
    return psd_amd.PeriodicSchur(Ts, Z, np.ones(n, dtype=complex), "R", 1)


def _singular_zg(seed=0):
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


def _singular_dg():
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


# ------------------------------------------------------------------------------------------------
# the families of this role.  windows: (nb, n, p[, S for 'R']) and what each covers; narrow: with PSD_BORD_W=6, several
# narrow windows at a small order; group: the group loop under PSD_BATCH_GROUP=4; cap: PSD_BORD_NMAX=16 at order 20; chain:
# the shape of the ABI, argument and device-resident cases.  seed: of the factors of problem q (DG takes those of
# batch_cases.DG).  clone: a writable copy of a decomposition.  units / group_tol / single_tol / say_single: the bounds of
# check_problem — the checker's residual in units of eps at n <= 32, the selected and unselected eigenvalue groups and the
# single call in max|lambda| — and whether it prints the last.  noracle: the oracle runs on the first so many problems of
# a shape.  each_moves: every problem of a window shape needs a swap.  lds_bytes, wcands, wmax: what expected_window
# models.  bad: the problem of one_fails_inputs; fail_exc, fail_exact: how its rejection shows.  only, sister: the words
# in which a signed entry refuses the other element type, and the family it names.
_SHAPES4 = [(3, 48, 3), (2, 40, 22), (2, 30, 70), (33, 12, 3)]
_SIGNED = [
    (3, 48, 3, (T, F, T)),       # several windows (ZG: W = 32 < n; DG: W = 25), all off-window roles on both sides
    (2, 40, 22, SIG22),          # ZG: W = 20; DG: W = 24
    (2, 30, 70, SIG70),          # ZG: W = 10, window image near the LDS limit; DG: W = 6, the per-factor scratch near it
    (33, 12, 3, (T, F, T)),      # more problems than a 32-wide chunk, n < W
    (3, 5, 2, (T, F)),           # a pencil (DG: problem 2 needs no swap in 'L')
    (4, 2, 2, (T, F)),           # smallest window; row 2 alone is selected (DG: real spectra only)
    (3, 1, 3, (T, F, T)),        # n = 1: no swap
    (3, 33, 4, (T, T, F, T)),    # signature class: a positive factor beside a negative one
    (3, 20, 4, (T, F, F, T)),    # signature class: adjacent negative factors
]
_EITHER = (psd_amd.SingularException, psd_amd.IllConditionedException)

# several windows at the widest W; narrow W from a large p (two of them); more problems than a 32-wide chunk
D = bcm.D.with_(windows=_SHAPES4, narrow=(3, 20, 3), group=(6, 20, 3), cap=(2, 20, 3), chain=(5, 12, 3),
                seed=lambda q, n, p: 90 + n + p + 1000 * q, clone=_clone, group_tol=1e-8, single_tol=1e-9, say_single=False,
                noracle=None, each_moves=True, bad=lambda: _equal_eigenvalues(np.float64), fail_exc=_EITHER,
                fail_exact=False, chain_exact=False)
Z = bcm.Z.with_(windows=_SHAPES4 + [
                    (3, 5, 1),    # p = 1: the p == 1 branch of the swap, where H_{m-1} is H_m
                    (4, 2, 2),    # smallest window; row 2 alone is selected
                    (3, 1, 3),    # n = 1: no swap
                ], narrow=(3, 20, 3), group=(6, 20, 3), cap=(2, 20, 3), chain=(5, 12, 3),
                seed=lambda q, n, p: 9500 + 131 * q + 7 * n + p, clone=_clone, group_tol=1e-9, single_tol=None,
                say_single=False, noracle=None, each_moves=True, bad=lambda: _equal_eigenvalues(np.complex128),
                fail_exc=_EITHER, fail_exact=False, chain_exact=False)
ZG = bcm.ZG.with_(windows=_SIGNED, narrow=(3, 20, 3, (T, F, T)), group=(6, 20, 3, (T, T, F)), cap=(2, 20, 3, (T, F, T)),
                  chain=(5, 12, 3, (T, F, T)), seed=lambda q, n, p: 9700 + 131 * q + 7 * n + p, clone=gclone, units=100,
                  group_tol=1e-9, single_tol=None, say_single=False, noracle=6, each_moves=True, bad=_singular_zg,
                  fail_exc=_EITHER, fail_exact=False, chain_exact=False, lds_bytes=_zg_lds_bytes,
                  wcands=(32, 24, 20, 16, 12, 10, 8, 6, 4), wmax=32, only="ComplexF64 only")
# units: 400 as engine_cases.case_gordschur_pairs_random; wmax: PSD_BORD_SPAN1 (csrc/psd_bord_host.inl, bord_real::window)
DG = bcm.DG.with_(windows=_SIGNED + [(4, 7, 5, (T, F, T, F, T))],  # odd order, alternating signature
                  narrow=ZG.narrow, group=ZG.group, cap=ZG.cap, chain=ZG.chain, clone=gclone, units=400, group_tol=1e-8,
                  single_tol=1e-9, say_single=True, noracle=6, each_moves=False, bad=_singular_dg,
                  fail_exc=psd_amd.SingularException, fail_exact=True, chain_exact=True, lds_bytes=_dg_lds_bytes,
                  wcands=(32, 24, 20, 16, 12, 10, 8, 6), wmax=25, only="Float64 only")
ZG.sister, DG.sister = DG, ZG


def expected_window(fam, n, p):
    """The window of a signed family's driver: of its candidates that fit the LDS (fam.lds_bytes, rounded up to 16, within
    155 KB) the smallest that holds the whole problem, otherwise the widest, and at most fam.wmax."""
    W = 0
    for w in fam.wcands:
        if (fam.lds_bytes(p, w) + 15) // 16 * 16 > 155 * 1024:
            continue
        if W == 0 or w >= n:
            W = w
    return min(W, fam.wmax)


def factors(fam, shape):
    """The factors of a shape: built once, shared, never written to."""
    nb, n, p = shape[:3]
    if fam is DG:
        return bc.problems(bc.DG, shape)
    return bcm.factors(fam.dtype, [fam.seed(q, n, p) for q in range(nb)], n, p)


def inputs(eng, fam, shape, lr):
    """(factors, decompositions, selections) of a shape and orientation: computed once per library and only cloned."""
    def make():
        probs = factors(fam, shape)
        ps0 = fam.method(eng, "pschur_batch")(probs, *(fam.sargs(sig(shape, lr)) if fam.signed else ()), lr)
        return probs, ps0, np.array([select_for(shape, ps.values) for ps in ps0])
    return bcm.cached(("ord inputs", fam.name, eng.lib._name, shape, lr), make)


def single(eng, fam, shape, lr, q):
    """ordschur_ of problem q on `eng` (the serial or the default single driver): computed once, never written to."""
    def make():
        probs, ps0, sels = inputs(eng, fam, shape, lr)
        return eng.ordschur_(fam.clone(ps0[q]), sels[q]), eng  # (the engine lives as long as its entry: its id stays its)
    return bcm.cached(("ord single", fam.name, id(eng), shape, lr, q), make)[0]


def oracle(fam, ps0, select):
    if fam.signed:
        po0 = pt.GPSD(ps0.S, [t.copy() for t in ps0.Ts], [z.copy() for z in ps0.Z], ps0.alpha, ps0.beta, ps0.alphascale,
                      ps0.orientation, ps0.schurindex)
        return pt.oracle_gordschur(po0, select)
    return pt.oracle_ordschur(pt.PSD(ps0.Ts, ps0.Z, ps0.values, ps0.orientation, ps0.schurindex), select)


def decomposes(fam, A, ps, S=None):
    """ps is a decomposition of A, by the family's checker at its default bounds"""
    if fam.signed:
        fam.check(A, S, ps)
    else:
        pt.pschur_check(A, ps, check_lam=False, real=not fam.cplx)


def check_problem(fam, A, ps0, ps1, select, oracle_run=True, nswaps=None, one=None, what=None):
    """The checks of engine_cases.case_rordschur_windows / case_zordschur_windows / case_gordschur_windows /
    case_gordschur_pairs_random with their bounds, for one problem; returns the swap count."""
    n = A[0].shape[0]
    lam0 = ps0.values
    r = max(1.0, np.sqrt(n / 32))
    if fam.signed:
        assert ps1.S == ps0.S
        fam.check(A, ps0.S, ps1, tol=fam.units * r, qtol=10 * r)
        assert np.array_equal(ps1.values, pt.gvalues(ps1.alpha, ps1.beta, ps1.alphascale))
    else:
        ok, err = pt.checkpsd(ps1, A, thresh=100 * r)  # (strict: zero strict lower triangles)
        assert ok, err
    if fam is ZG:
        for t in ps1.Ts:
            assert np.all(np.tril(t, -1) == 0)  # (every factor stays triangular)
    elif fam is DG:
        real_form(ps1, what)
    elif fam is D:
        for i in range(n - 1):  # structure: sub-diagonal entries only inside conjugate pairs
            if ps1.values[i].imag == 0 or ps1.values[i].imag < 0:
                assert ps1.T1[i + 1, i] == 0
    closed = select if fam.cplx else closed_select(lam0, select)
    m = int(closed.sum())
    sc = abs(lam0).max()
    assert pt.match_eigs(lam0[closed], ps1.values[:m]) < fam.group_tol * sc
    assert pt.match_eigs(lam0[~closed], ps1.values[m:]) < fam.group_tol * sc
    if fam.cplx:  # the order inside the selected / unselected groups is preserved (stable bubbling)
        assert np.allclose(ps1.values[:m], lam0[select], rtol=1e-7, atol=1e-9 * sc)
        assert np.allclose(ps1.values[m:], lam0[~select], rtol=1e-7, atol=1e-9 * sc)
    if oracle_run:
        po = oracle(fam, ps0, select)
        assert po.info == 0 and ps1.stats.nsweeps == po.nswaps, (what, ps1.stats.nsweeps, po.nswaps)
    if nswaps is not None:
        assert ps1.stats.nsweeps == nswaps, (what, ps1.stats.nsweeps, nswaps)
    if one is not None and fam.single_tol is not None:
        err = pt.match_eigs(one.values, ps1.values)
        if fam.say_single:
            print(f"{what}: |lam - single call| = {err:.3e} (bound {fam.single_tol * sc:.3e}), {ps1.stats.nsweeps} swaps")
        assert err < fam.single_tol * sc, (what, err)
    return ps1.stats.nsweeps


def _same(a, b):
    """T, Z, the values and — where the decompositions carry them — alpha, beta and the scaling, bit for bit"""
    def arrays(ps):
        return ps.Ts + ps.Z + [ps.values] + [getattr(ps, k) for k in ("alpha", "beta", "alphascale") if hasattr(ps, k)]
    return all(np.array_equal(x, y) for x, y in zip(arrays(a), arrays(b)))


def bits_differ(a, b):
    """The number of entries of T, Z and the values whose bits differ."""
    return sum(int((x != y).sum()) for x, y in zip(a.Ts + a.Z + [a.values], b.Ts + b.Z + [b.values]))


# ------------------------------------------------------------------------------------------------
# 1. reference shapes
def case_reference(eng, fam, lr):
    """engine_cases.case_rordschur_reference_real / case_zordschur_reference / case_gordschur_reference per problem of a
    batch: (nb, n) = (4, 7), p = 3 (signed: p = 5 with an alternating signature), spectrum 4^j; the 2 smallest and the 2
    largest selected, against the oracle's swap counts and eigenvalues."""
    nb, n, nsel = 4, 7, 2
    if fam.signed:
        p = 5
        S = [True] * p
        for l in range(0, p - 1, 2):
            S[l] = False
        probs = [pt.gord_test_factors(n, p, S, seed=31 + 37 * q, cplx=fam.cplx) for q in range(nb)]
        if lr == "R":
            probs, S = [A[::-1] for A in probs], S[::-1]
    else:
        p, S = 3, None
        probs = [pt.ord_test_factors(n, p, seed=4000 + p + 37 * q, dtype=fam.dtype) for q in range(nb)]
        if lr == "R":
            probs = [A[::-1] for A in probs]
    ps0 = fam.method(eng, "pschur_batch")(probs, *fam.sargs(S), lr)
    for q in range(nb):
        if fam.signed:
            decomposes(fam, probs[q], ps0[q], S)
        else:
            assert np.allclose(np.sort(np.abs(ps0[q].values)), [4.0 ** (j + 1) for j in range(n)], rtol=1e-8)
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
        out = fam.method(eng, "ordschur_batch_")([fam.clone(ps) for ps in ps0], np.array(sels))
        assert fam.method(eng, "ordschur_batch_stats").nlaunch_step == 1
        for q in range(nb):
            decomposes(fam, probs[q], out[q], S)
            if fam is DG:
                real_form(out[q], (lr, which, q))
            for j in range(nsel):
                assert np.any(np.isclose(out[q].values[:nsel], ps0[q].values[idxs[q][j]], rtol=1e-8))
            po = oracle(fam, ps0[q], sels[q])
            assert po.info == 0 and out[q].stats.nsweeps == po.nswaps
            assert pt.match_eigs(po.values, out[q].values) < 1e-9 * abs(po.values).max()
            if fam is Z:
                assert np.allclose(out[q].values, po.values, rtol=1e-10, atol=0)


def case_pairs(eng):
    """D: engine_cases.case_rordschur_pairs as one batch: mkrps (3, 7, 2), pairs at rows 3:4 and 6:7, against the oracle."""
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


def case_pairs_reference(eng):
    """DG: engine_cases.case_gordschur_pairs_reference as ONE batch: mkrps(7, 5, [3, 6], alt=True) with its six selection
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
# 2. windows
def case_windows(eng, fam, shape, lr, expect_window=None):
    nb, n, p = shape[:3]
    probs, ps0, sels = inputs(eng, fam, shape, lr)
    batch_ = fam.method(eng, "ordschur_batch_")
    out = batch_([fam.clone(ps) for ps in ps0], sels)
    st = fam.method(eng, "ordschur_batch_stats")
    assert len(out) == nb and st.nlaunch_step == 1 and st.nsweeps == sum(ps.stats.nsweeps for ps in out)
    assert list(fam.method(eng, "ordschur_batch_nswaps")) == [ps.stats.nsweeps for ps in out]
    if expect_window is not None:
        assert st.window == expect_window and st.nwindows > nb  # (several windows per problem)
    elif fam.signed:
        assert st.window == expected_window(fam, n, p), (st.window, expected_window(fam, n, p))
    noz = batch_([fam.clone(ps) for ps in ps0], sels, wantZ=False)
    total = 0
    for q in range(nb):
        one = single(eng, fam, shape, lr, q)
        nsw = check_problem(fam, probs[q], ps0[q], out[q], sels[q], oracle_run=fam.noracle is None or q < fam.noracle,
                            nswaps=one.stats.nsweeps, one=one, what=(shape_id(shape), lr, q))
        assert not fam.each_moves or (nsw > 0) == (n > 1)
        total += nsw
        sc = abs(ps0[q].values).max()
        # wantZ = false leaves Z untouched and gives the same T
        assert all(np.array_equal(a, b) for a, b in zip(noz[q].Z, ps0[q].Z))
        assert max(np.abs(a - b).max() for a, b in zip(noz[q].Ts, out[q].Ts)) < 1e-12 * sc
    assert (total > 0) == (n > 1)
    if fam is DG:
        if n == 2:
            assert not any(has_pair(ps) for ps in ps0)
        elif n > 2:  # real eigenvalues and pairs side by side: the 1x1 and the 2x2 signed swaps
            assert any(has_pair(ps) for ps in ps0) and any(np.any(ps.values.imag == 0) for ps in ps0)


# ------------------------------------------------------------------------------------------------
# 3. against the serial single driver
def case_against_serial(make_engine, fam, shape, lr, exact):
    """The single driver with PSD_ORD_PIPE=0 moves one eigenvalue at a time through the same windows with the same
    arithmetic as the batched kernel; the row and column roles of a window touch disjoint entries, so the order of the
    items cannot matter.  exact: bit for bit (the simulation is built with -ffp-contract=off); otherwise 1e-12 * scale
    (contraction may differ between kernels; signed: the bound of the all-true sister kernel, which runs the same kind
    of bodies).  Returns the number of entries whose bits differ."""
    nb, n, p = shape[:3]
    ser = make_engine({"PSD_ORD_PIPE": "0"})
    probs, ps0, sels = inputs(ser, fam, shape, lr)
    out = fam.method(ser, "ordschur_batch_")([fam.clone(ps) for ps in ps0], sels)
    differ = 0
    for q in range(nb):
        one = single(ser, fam, shape, lr, q)
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
def case_independence(eng, fam, shape, lr="R"):
    """A problem alone in a batch of one gets, bit for bit, what it gets inside the batch."""
    nb, n, p = shape[:3]
    probs, ps0, sels = inputs(eng, fam, shape, lr)
    batch_ = fam.method(eng, "ordschur_batch_")
    out = batch_([fam.clone(ps) for ps in ps0], sels)
    for q in sorted({0, nb - 2, nb - 1} & set(range(nb))):
        alone = batch_([fam.clone(ps0[q])], sels[q:q + 1])
        assert _same(alone[0], out[q]), (shape_id(shape), q)


def case_groups(make_engine, fam):
    """PSD_BATCH_GROUP=4: a batch worked through in two groups equals one group bit for bit."""
    nb, n, p = fam.group[:3]
    ref = make_engine({})
    eng = make_engine({"PSD_BATCH_GROUP": "4"})
    probs, ps0, sels = inputs(ref, fam, fam.group, "L")
    whole = fam.method(ref, "ordschur_batch_")([fam.clone(ps) for ps in ps0], sels)
    assert fam.method(ref, "ordschur_batch_stats").nlaunch_step == 1
    parts = fam.method(eng, "ordschur_batch_")([fam.clone(ps) for ps in ps0], sels)
    assert fam.method(eng, "ordschur_batch_stats").nlaunch_step == 2
    for q in range(nb):
        assert _same(whole[q], parts[q]), q
        assert whole[q].stats.nsweeps == parts[q].stats.nsweeps > 0


# ------------------------------------------------------------------------------------------------
# 5. all-true signature: ComplexF64 takes the call of zordschur_batch_, Float64 stays on the signed kernels
def _plain(ps0, lr):
    return [psd_amd.PeriodicSchur([t.copy(order="F") for t in ps.Ts], [z.copy(order="F") for z in ps.Z], ps.values.copy(),
                                  lr, ps.schurindex) for ps in ps0]


def _raw_null_signatures(eng, fam, lr, ps0, sels):
    """the C entry of a signed family on plain copies of ps0, with a NULL and with an all-true S: (copies, values, swaps)"""
    nb, p, n = len(ps0), len(ps0[0].Ts), len(ps0[0].values)
    for Sarr in (None, bcm.sarr([True] * p)):
        work = _plain(ps0, lr)
        flatT, flatZ = [t for ps in work for t in ps.Ts], [z for ps in work for z in ps.Z]
        vals = (np.zeros((nb, n), dtype=np.complex128), np.zeros((nb, n)), np.zeros((nb, n), dtype=np.int32))
        nsw = (C.c_int * nb)()
        rc = raw(eng, fam, fam.entry(eng, "ordschur_batch"), nb, n, p, eng._ptrs(flatT), eng._ptrs(flatZ), Sarr, lr.encode(),
                 ps0[0].schurindex, np.ascontiguousarray(sels, dtype=np.uint8), 1, vals, None, nsw)
        assert rc == 0
        yield work, [pt.gvalues(*(v[q] for v in vals)) for q in range(nb)], list(nsw)


def case_all_true_zg(eng):
    """A null or all-true S is the call of zordschur_batch_: the same bits, through the C entry and the Python method."""
    nb, n, p = ZG.chain[:3]
    probs = factors(ZG, ZG.chain)
    for lr in "RL":
        ps0 = eng.zpschur_batch(probs, lr)
        sels = np.array([median_select(ps.values) for ps in ps0])
        ref = eng.zordschur_batch_(_plain(ps0, lr), sels)
        rst = eng.zordschur_batch_stats
        assert rst.nsweeps > 0
        gen = [psd_amd.GeneralizedPeriodicSchur([True] * p, ps.Ts, ps.Z, ps.values.copy(), np.ones(n),
                                                np.zeros(n, dtype=np.int32), lr, ps.schurindex) for ps in _plain(ps0, lr)]
        out = eng.zgordschur_batch_(gen, sels)
        st = eng.zgordschur_batch_stats
        assert st.nsweeps == rst.nsweeps and st.window == rst.window and st.nlaunch_step == rst.nlaunch_step
        for q in range(nb):
            assert bits_differ(ref[q], out[q]) == 0 and out[q].stats.nsweeps == ref[q].stats.nsweeps
            assert np.array_equal(out[q].values, pt.gvalues(out[q].alpha, out[q].beta, out[q].alphascale))
        for work, values, nsw in _raw_null_signatures(eng, ZG, lr, ps0, sels):
            for q in range(nb):
                assert nsw[q] == ref[q].stats.nsweeps
                assert np.array_equal(values[q], ref[q].values)
                assert all(np.array_equal(a, b) for a, b in zip(work[q].Ts + work[q].Z, ref[q].Ts + ref[q].Z))


def case_all_true_dg(eng):
    """A null or all-true S is accepted and stays on the signed kernels: the result is in the scaled form, with the swap
    counts of ordschur_batch_ on the same factors and its eigenvalues to 1e-9 * scale."""
    nb, n, p = DG.chain[:3]
    probs = factors(DG, DG.chain)
    for lr in "RL":
        ps0 = eng.dgpschur_batch(probs, None, lr)
        assert all(ps.S == [True] * p for ps in ps0)
        sels = np.array([median_select(ps.values) for ps in ps0])
        ref = eng.ordschur_batch_(_plain(ps0, lr), sels)
        assert eng.ordschur_batch_stats.nsweeps > 0
        out = eng.dgordschur_batch_([gclone(ps) for ps in ps0], sels)
        assert eng.dgordschur_batch_stats.nsweeps == eng.ordschur_batch_stats.nsweeps
        for q in range(nb):
            sc = abs(ps0[q].values).max()
            assert out[q].stats.nsweeps == ref[q].stats.nsweeps
            assert np.array_equal(out[q].values, pt.gvalues(out[q].alpha, out[q].beta, out[q].alphascale))
            assert pt.match_eigs(ref[q].values, out[q].values) < 1e-9 * sc
            check_problem(DG, probs[q], ps0[q], out[q], sels[q], oracle_run=False, what=("all-true", lr, q))
        for work, values, nsw in _raw_null_signatures(eng, DG, lr, ps0, sels):
            for q in range(nb):
                assert nsw[q] == ref[q].stats.nsweeps
                assert np.array_equal(values[q], out[q].values)
                assert all(np.array_equal(a, b) for a, b in zip(work[q].Ts + work[q].Z, out[q].Ts + out[q].Z))


# ------------------------------------------------------------------------------------------------
# 6. per-problem selections
def case_selections_d(eng):
    """D: all-false, all-true, one member of a conjugate pair, and the median rule side by side in one batch"""
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
    check_problem(D, A, ps0, out[2], sels[2])
    check_problem(D, A, ps0, out[3], sels[3])
    one = eng.ordschur_batch_([_clone(ps0) for _ in range(3)], sels[3])  # one row for every problem
    assert all(_same(o, out[3]) for o in one)


def case_selections(eng, fam):
    """Z, ZG, DG: all-false, all-true and the median rule — DG: and each member of a pair alone — side by side in one
    batch; one row for every problem"""
    shape = (1, 8, 3) + (((T, F, T),) if fam.signed else ())
    n = shape[1]
    probs, ps0, _ = inputs(eng, fam, shape, "R")
    A, ps0 = probs[0], ps0[0]
    lam0 = ps0.values
    S = ps0.S if fam.signed else None
    sels = np.zeros((3 if fam.cplx else 5, n), dtype=bool)
    sels[1] = True
    sels[2] = median_select(lam0)
    if not fam.cplx:
        pairs = [i for i in range(1, n - 1) if lam0[i].imag > 0]  # (a pair that does not stand at the top)
        assert pairs
        sels[3, pairs[-1]] = True      # the first member of a pair alone
        sels[4, pairs[-1] + 1] = True  # the second member alone
    batch_ = fam.method(eng, "ordschur_batch_")
    out = batch_([fam.clone(ps0) for _ in range(len(sels))], sels)
    assert out[0].stats.nsweeps == 0 and out[1].stats.nsweeps == 0
    for o in out[:2]:
        assert all(np.array_equal(a, b) for a, b in zip(o.Ts + o.Z, ps0.Ts + ps0.Z))  # untouched bit for bit
        assert np.allclose(o.values, lam0, rtol=1e-13, atol=0)  # (recomputed from the same diagonals / diagonal blocks)
    decomposes(fam, A, out[1], S)
    assert pt.match_eigs(lam0, out[1].values) < 1e-9 * abs(lam0).max()
    assert check_problem(fam, A, ps0, out[2], sels[2], what="median") > 0
    if not fam.cplx:
        for q in (3, 4):  # one member of a pair takes its partner along
            assert check_problem(fam, A, ps0, out[q], sels[q], what="pair member") > 0
            assert pt.match_eigs(out[q].values[:2], lam0[pairs[-1]:pairs[-1] + 2]) < 1e-8 * abs(lam0).max()
        assert _same(out[3], out[4])
    one = batch_([fam.clone(ps0) for _ in range(3)], sels[2])  # one row for every problem
    assert all(_same(o, out[2]) for o in one)


# ------------------------------------------------------------------------------------------------
# 7. one problem fails
def one_fails_inputs(eng, fam):
    """three good problems of n = 4, p = 2 (signed: S = (T, F)) around the family's problem whose swap is rejected"""
    shape = (3, 4, 2) + (((T, F),) if fam.signed else ())
    if fam is D:  # (its good problems are those of the shape, decomposed by the single call)
        good = factors(D, shape)
        ps0 = [eng.pschur(A, "R") for A in good]
        gsel = [median_select(ps.values) for ps in ps0]
    else:
        good, ps0, gsel = inputs(eng, fam, shape, "R")
    bad = fam.bad()
    probs = [good[0], [t.copy() for t in bad.Ts], good[1], good[2]]
    work = [ps0[0], bad, ps0[1], ps0[2]]
    sels = np.array([gsel[0], [False, True, False, False], gsel[1], gsel[2]])
    return probs, work, sels


def case_one_fails(eng, fam):
    probs, work, sels = one_fails_inputs(eng, fam)
    batch_ = fam.method(eng, "ordschur_batch_")
    with pytest.raises(fam.fail_exc):
        eng.ordschur_(fam.clone(work[1]), sels[1])  # (the single call on the same engine rejects it: the yardstick)
    infos = []
    out = batch_([fam.clone(ps) for ps in work], sels, infos_out=infos)
    assert len(infos) == 4 and infos[0] == 0 and infos[2] == 0 and infos[3] == 0, infos
    assert infos[1] == 3000 or (not fam.fail_exact and 2000 <= infos[1] < 3000), infos
    for q in (0, 2, 3):
        check_problem(fam, probs[q], work[q], out[q], sels[q], what=("one fails", q))
    # the failed problem is still a decomposition of its product, Z_j' A_j Z_{j+1} = T_j, with its old values
    if fam.fail_exact:  # (the rejected swap left the factors as they were, and Z = I)
        assert all(np.array_equal(a, b) for a, b in zip(out[1].Ts + out[1].Z, work[1].Ts + work[1].Z))
        for l in range(2):
            assert np.array_equal(out[1].Z[l] @ out[1].Ts[l] @ out[1].Z[1 - l].T, probs[1][l])
    else:
        decomposes(fam, probs[1], out[1], work[1].S if fam.signed else None)
    assert np.array_equal(out[1].values, work[1].values)
    assert not fam.signed or np.array_equal(out[1].alpha, work[1].alpha)
    again = [fam.clone(ps) for ps in work]
    with pytest.raises(fam.fail_exc):  # raised after all four have run
        batch_(again, sels)
    for q in (0, 2, 3):
        assert _same(again[q], out[q])


# ------------------------------------------------------------------------------------------------
# 8. fallback above the cap
def case_above_cap(make_engine, fam):
    """PSD_BORD_NMAX=16 at order 20: the single driver problem by problem on the batch buffers — the single calls' bits.
    DG: for a problem that contains a pair; one with a real spectrum, which the single call promotes to the complex kernel,
    goes through check_problem."""
    nb, n, p = fam.cap[:3]
    eng = make_engine({"PSD_BORD_NMAX": "16"})
    for lr in "RL":
        probs, ps0, sels = inputs(eng, fam, fam.cap, lr)
        out = fam.method(eng, "ordschur_batch_")([fam.clone(ps) for ps in ps0], sels)
        assert fam.method(eng, "ordschur_batch_stats").nlaunch_step > 1
        for q in range(nb):
            one = eng.ordschur_(fam.clone(ps0[q]), sels[q])
            assert one.stats.nsweeps == out[q].stats.nsweeps > 0
            if fam is DG:
                check_problem(fam, probs[q], ps0[q], out[q], sels[q], nswaps=one.stats.nsweeps, one=one, what=("cap", lr, q))
            if fam is not DG or has_pair(ps0[q]):
                assert _same(one, out[q]), (lr, q)


# ------------------------------------------------------------------------------------------------
# 9. C ABI and arguments
def raw(eng, fam, fn, nb, n, p, Tp, Zp, S, orient, si, sel, wantZ, vals, infos=None, nsw=None, st=None):
    """A reordering entry of the family.  vals: the value arrays — (wr, wi) for D, (alpha, beta, scale) otherwise —, each
    an array or None; S (an array or None) is passed where the family is signed."""
    info = C.c_int(0)

    def at(a):
        if a is None:
            return None
        if a.dtype == np.int32:
            return a.ctypes.data_as(C.POINTER(C.c_int32))
        return a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))
    rc = fn(eng.ctx, nb, n, p, Tp, Zp, *fam.sargs(S), orient, si,
            sel.ctypes.data_as(C.POINTER(C.c_uint8)) if sel is not None else None, wantZ, *[at(v) for v in vals],
            infos, nsw, C.byref(st) if st is not None else None, C.byref(info))
    assert rc == info.value
    return rc


def value_arrays(fam, *shape):
    if fam is D:
        return np.zeros(shape), np.zeros(shape)
    return np.zeros(shape, dtype=np.complex128), np.zeros(shape), np.zeros(shape, dtype=np.int32)


def values_of(fam, vals):
    return vals[0] + 1j * vals[1] if fam is D else pt.gvalues(*vals)


def case_argument_codes(eng, fam):
    shape = fam.chain
    nb, n, p = shape[:3]
    probs, ps0, sels = inputs(eng, fam, shape, "R")
    w = fam.clone(ps0[0])
    Tp, Zp = eng._ptrs(w.Ts), eng._ptrs(w.Z)
    buf = np.zeros((p, n, n), dtype=fam.dtype)
    sel = np.ascontiguousarray(sels[0], dtype=np.uint8)
    vals = value_arrays(fam, n)
    Sok = bcm.sarr(sig(shape, "R")) if fam.signed else None  # (T, F, T)
    Sbad, Slast = bcm.sarr((F, T, T)), bcm.sarr((T, T, F))

    def places(e):
        return ((fam.entry(e, "ordschur_batch"), Tp, Zp),
                (fam.entry(e, "ordschur_batch_dev"), C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data)))
    for fn, Tq, Zq in places(eng):
        def f(nb_=1, n_=n, p_=p, T_=Tq, Z_=Zq, S_=Sok, o=b"R", si=1, sel_=sel, wz=1, v_=vals):
            return raw(eng, fam, fn, nb_, n_, p_, T_, Z_, S_, o, si, sel_, wz, v_)
        assert f(n_=0) == -2 and f(p_=0) == -3 and f(T_=None) == -4 and f(Z_=None) == -5 and f(o=b"X") == -6
        assert f(si=2) == -7 and f(si=0) == -7 and f(si=p + 1) == -7  # strictly inside, or outside, the period
        assert f(sel_=None) == -8 and f(nb_=-1) == -11
        for k in range(len(vals)):
            assert f(v_=vals[:k] + (None,) + vals[k + 1:]) == -9
        if fam.signed:
            # the entry of S that lands first in working order is that of the Schur factor: slot schurindex of the user's
            assert f(S_=Sbad) == -10 and f(S_=Sbad, o=b"L") == -10
            assert f(S_=Slast, si=p) == -10 and f(S_=Slast, o=b"L", si=p) == -10
            assert f(nb_=0, S_=Sbad) == 0
        assert f(nb_=0) == 0 and f(nb_=0, T_=None) == 0
        info = C.c_int(0)
        assert fn(None, 1, n, p, Tq, Zq, *fam.sargs(Sok), b"R", 1, sel.ctypes.data_as(C.POINTER(C.c_uint8)), 1,
                  *[None] * len(vals), None, None, None, C.byref(info)) == -1
    # a period-sharded context keeps a slice of Z: the batched entries refuse it (an engine of its own, let go afterwards)
    sharded = psd_amd.Engine(libpath=eng.lib._name)
    sharded.set_shard(0, 2)
    for fn, Tq, Zq in places(sharded):
        assert raw(sharded, fam, fn, 1, n, p, Tq, Zq, Sok, b"R", 1, sel, 1, vals) == psd_amd.INFO_NOTIMPL
        assert raw(sharded, fam, fn, 0, n, p, Tq, Zq, Sok, b"R", 1, sel, 1, vals) == 0
    with pytest.raises(psd_amd.NotImplementedPSD):
        fam.method(sharded, "ordschur_batch_")([fam.clone(ps0[0])], sels[:1])
    sharded.set_shard(0, 1)
    assert fam.method(sharded, "ordschur_batch_")([fam.clone(ps0[0])], sels[:1])[0].stats.nsweeps > 0  # (whole again)
    # (no refused call touched anything)
    assert _same(w, ps0[0]) and not buf.any() and not any(v.any() for v in vals)


def case_python_errors(eng, fam):
    shape = fam.chain
    nb, n, p = shape[:3]
    S = list(shape[3]) if fam.signed else None
    probs, ps0, sels = inputs(eng, fam, shape, "R")
    batch, batch_ = fam.method(eng, "ordschur_batch"), fam.method(eng, "ordschur_batch_")
    clone = fam.clone

    def decomposed(n_, seed, lr, dtype=fam.dtype, S_=S):
        """the single call's decomposition of bench factors"""
        A = pt.bench_factors(n_, p, seed=seed, dtype=dtype)
        return eng.pschur_(A, lr, S=S_) if fam.signed else eng.pschur(A, lr)
    with pytest.raises(psd_amd.DimensionMismatch):
        batch([ps0[0], decomposed(9, 3, "R")], np.zeros(n, dtype=bool))  # unequal order
    left = decomposed(n, 4, "L") if fam.signed else eng.pschur(probs[1], "L")
    with pytest.raises(psd_amd.DimensionMismatch):
        batch([ps0[0], left], sels[:2])  # unequal orientation
    if fam.signed:
        with pytest.raises(psd_amd.DimensionMismatch, match="signatures"):
            batch([ps0[0], decomposed(n, 5, "R", S_=[True, True, False])], sels[:2])  # unequal S
    with pytest.raises(psd_amd.DimensionMismatch):
        batch(ps0[:2], np.zeros((2, n - 1), dtype=bool))  # select rows of the wrong length
    with pytest.raises(psd_amd.DimensionMismatch):
        batch(ps0[:2], np.zeros((3, n), dtype=bool))  # ... or the wrong number of them
    if fam.signed:
        # the entries without a signature keep refusing signed problems
        plain = Z if fam.cplx else D
        for fn in (plain.method(eng, "ordschur_batch"), plain.method(eng, "ordschur_batch_")):
            with pytest.raises(psd_amd.NotImplementedPSD, match="use ordschur_ per problem"):
                fn([clone(ps0[0])], sels[:1])
        # each signed entry names the other one for a problem of the other element type
        sis = fam.sister
        for fn in (sis.method(eng, "ordschur_batch"), sis.method(eng, "ordschur_batch_")):
            with pytest.raises(psd_amd.NotImplementedPSD, match=f"{sis.only}.*{fam.prefix}ordschur_batch"):
                fn([clone(ps0[0])], sels[:1])
        other = decomposed(n, 3, "R", dtype=sis.dtype)
        assert np.iscomplexobj(other.Ts[0]) != fam.cplx
        for fn in (batch, batch_):
            with pytest.raises(psd_amd.NotImplementedPSD, match=f"{fam.only}.*{sis.prefix}ordschur_batch"):
                fn([other], sels[:1])
    else:
        # ordschur_batch refuses ComplexF64 and zordschur_batch refuses Float64, naming the other; both refuse signed ones
        if fam.cplx:
            cx, rl = ps0[0], eng.pschur(pt.bench_factors(n, p, seed=3), "R")
        else:
            cx = psd_amd.PeriodicSchur([t.astype(np.complex128) for t in ps0[0].Ts],
                                       [z.astype(np.complex128) for z in ps0[0].Z], ps0[0].values, "R", 1)
            rl = ps0[0]
        for fn in (eng.ordschur_batch, eng.ordschur_batch_):
            with pytest.raises(psd_amd.NotImplementedPSD):
                fn([_clone(cx)], sels[:1])
        for fn in (eng.zordschur_batch, eng.zordschur_batch_):
            with pytest.raises(psd_amd.NotImplementedPSD, match="ordschur_batch"):
                fn([_clone(rl)], sels[:1])
        Sg = [True] * p
        Sg[1] = False
        signed = psd_amd.GeneralizedPeriodicSchur(Sg, ps0[0].Ts, ps0[0].Z, ps0[0].values, np.ones(n),
                                                  np.zeros(n, dtype=np.int32), "R", 1)
        with pytest.raises(psd_amd.NotImplementedPSD):
            batch([signed], sels[:1])
    notf = clone(ps0[0])
    notf.Ts[1] = np.ascontiguousarray(notf.Ts[1])
    with pytest.raises(TypeError):
        batch_([notf], sels[:1])  # in place needs Fortran order
    ro = clone(ps0[0])
    ro.Z[0].setflags(write=False)
    with pytest.raises(TypeError):
        batch_([ro], sels[:1])  # ... and writable arrays
    mid = clone(ps0[0])
    mid.schurindex = 2
    with pytest.raises(ValueError):
        batch_([mid], sels[:1])  # interior schurindex (rordschur.jl:25, ordschur.jl:32)
    if fam.signed:
        neg = clone(ps0[0])
        neg.S = [False, True, True]
        with pytest.raises(ValueError):
            batch_([neg], sels[:1])  # the Schur factor's entry of S is false
    assert batch_([], sels) == [] and batch([], sels[0]) == []
    infos = [7]
    assert batch_([], sels, infos_out=infos) == [] and infos == []
    keep = clone(ps0[0])
    got = batch([ps0[0]], sels[:1])  # the copying form leaves its input alone
    assert _same(keep, ps0[0]) and got[0].stats.nsweeps > 0 and (not fam.signed or got[0].S == S)
    assert got[0].Ts[0].dtype == fam.dtype and not _same(got[0], ps0[0])


def _placed(fam, ps, si):
    """a copy of ps in the alignment `si` of its orientation: the same factors (and signature) written shifted by one slot,
    so that the Schur factor goes from the first slot to the last, or back.  Only the bits matter here."""
    q = fam.clone(ps)
    if si != ps.schurindex:
        rot = (lambda x: x[1:] + x[:1]) if si == len(ps.Ts) else (lambda x: x[-1:] + x[:-1])
        q.Ts, q.Z = rot(q.Ts), rot(q.Z)
        if fam.signed:
            q.S = rot(q.S)
        q.schurindex = si
    return q


def case_dev_abi(eng, fam, launches=1, device=False):
    """The family's ordschur_batch_dev entry through the C ABI on packed [nb][p][n][n] column-major blocks — numpy arrays in
    the simulation, where device memory is host memory, torch CUDA tensors through data_ptr() on the GPU (device=True): the
    same bits as the host entry, for both alignments of each orientation.
    `launches`: the groups the engine's PSD_BATCH_GROUP cuts the batch into (the shifted alignments are then gathered a
    group at a time as well)."""
    shape = fam.chain
    nb, n, p = shape[:3]
    for lr in "RL":
        probs, ps0, sels = inputs(eng, fam, shape, lr)
        si0 = ps0[0].schurindex
        for si in (si0, p + 1 - si0):
            host = fam.method(eng, "ordschur_batch_")([_placed(fam, ps, si) for ps in ps0], sels)
            hst = fam.method(eng, "ordschur_batch_stats")
            src = [_placed(fam, ps, si) for ps in ps0]
            Sarr = bcm.sarr(src[0].S) if fam.signed else None
            dT = np.ascontiguousarray(np.array([pt.pack(ps.Ts, fam.dtype) for ps in src]))
            dZ = np.ascontiguousarray(np.array([pt.pack(ps.Z, fam.dtype) for ps in src]))
            if device:
                import torch

                gT, gZ = torch.from_numpy(dT).cuda(), torch.from_numpy(dZ).cuda()
                assert gT.is_contiguous() and gZ.is_contiguous()
                torch.cuda.synchronize()
                pT, pZ = C.c_void_p(gT.data_ptr()), C.c_void_p(gZ.data_ptr())
            else:
                pT, pZ = C.c_void_p(dT.ctypes.data), C.c_void_p(dZ.ctypes.data)
            vals = value_arrays(fam, nb, n)
            infos, nsw = (C.c_int * nb)(), (C.c_int * nb)()
            st = psd_amd.Stats()
            sel = np.ascontiguousarray(sels, dtype=np.uint8)
            rc = raw(eng, fam, fam.entry(eng, "ordschur_batch_dev"), nb, n, p, pT, pZ, Sarr, lr.encode(), si, sel, 1, vals,
                     infos, nsw, st)
            if device:  # (the entry returns with its stream drained)
                dT, dZ = gT.cpu().numpy(), gZ.cpu().numpy()
            assert rc == 0 and not any(infos) and st.nlaunch_step == hst.nlaunch_step == launches and st.window == hst.window
            assert st.nsweeps == hst.nsweeps == sum(nsw) > 0 and st.ms_total >= 0
            values = values_of(fam, vals)
            for q in range(nb):
                assert nsw[q] == host[q].stats.nsweeps
                assert np.array_equal(values[q], host[q].values)
                for j in range(p):
                    assert np.array_equal(dT[q, j].T, host[q].Ts[j]) and np.array_equal(dZ[q, j].T, host[q].Z[j]), (lr, si, q, j)


# ------------------------------------------------------------------------------------------------
# 10. device-resident chain (GPU tier)
def case_device_chain(eng, fam, lr):
    """pschur_batch_ -> ordschur_batch_ (D: -> eigvecs_batch) of the family without a matrix touching the host"""
    import torch

    shape = fam.chain
    nb, n, p = shape[:3]
    Skw = {"S": sig(shape, lr)} if fam.signed else {}
    probs = factors(fam, shape)
    si = p if lr == "L" else 1
    batch, batch_ = fam.method(eng, "ordschur_batch"), fam.method(eng, "ordschur_batch_")
    tdtype = torch.complex128 if fam.cplx else torch.float64

    def form(Tq, Zq, values):
        Ts, Zs = [np.asfortranarray(Tq[j]) for j in range(p)], [np.asfortranarray(Zq[j]) for j in range(p)]
        if fam.signed:
            return psd_amd.GeneralizedPeriodicSchur(Skw["S"], Ts, Zs, values, np.ones(n), np.zeros(n, dtype=np.int32), lr,
                                                    si)
        return psd_amd.PeriodicSchur(Ts, Zs, values, lr, si)
    dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in probs])).cuda()
    T0, Z0, values, _ = fam.method(eng, "pschur_batch_")(dA, *Skw.values(), lr)
    assert T0.dtype == tdtype and Z0.dtype == tdtype
    sels = np.array([median_select(v) for v in values])
    ps0 = [form(T0[q].cpu().numpy(), Z0[q].cpu().numpy(), values[q].copy()) for q in range(nb)]
    host = batch_([fam.clone(ps) for ps in ps0], sels)
    T1, Z1, values1, st = batch_(T0, Z0, sels, lr=lr, schurindex=si, **Skw)
    assert T1.data_ptr() == T0.data_ptr() and Z1.data_ptr() == Z0.data_ptr()  # in place
    assert T1.stride() == T0.stride() and Z1.stride() == Z0.stride()
    assert st.nlaunch_step == 1 and tuple(T1.shape) == (nb, p, n, n) and T1.dtype == tdtype
    Th, Zh = T1.cpu().numpy(), Z1.cpu().numpy()
    for q in range(nb):
        if fam.chain_exact:  # (the same kernels on the same bits)
            assert np.array_equal(values1[q], host[q].values)
            for j in range(p):
                assert np.array_equal(Th[q, j], host[q].Ts[j]) and np.array_equal(Zh[q, j], host[q].Z[j]), (lr, q, j)
        else:
            sc = max(np.linalg.norm(a, 2) for a in probs[q])
            assert np.abs(values1[q] - host[q].values).max() <= 1e-12 * np.abs(host[q].values).max()
            for j in range(p):
                assert np.abs(Th[q, j] - host[q].Ts[j]).max() <= 1e-12 * sc, (lr, q, j)
                assert np.abs(Zh[q, j] - host[q].Z[j]).max() <= 1e-12, (lr, q, j)
        ps1 = form(Th[q], Zh[q], values1[q])
        ps1.stats = psd_amd.Stats()
        ps1.stats.nsweeps = int(fam.method(eng, "ordschur_batch_nswaps")[q])
        check_problem(fam, probs[q], ps0[q], ps1, sels[q], nswaps=host[q].stats.nsweeps, what=("chain", lr, q))
    if fam is D:
        _chain_eigvecs(eng, lr, si, probs, values, sels, T1, Z1, values1)
    # any other layout is copied first: the input stays as it was
    Tc = T1.contiguous()
    keep = Tc.clone()
    T2, Z2, v2, _ = batch_(Tc, Z1.contiguous(), np.ones((nb, n), dtype=bool), lr=lr, schurindex=si, **Skw)
    assert T2.data_ptr() != Tc.data_ptr() and torch.equal(Tc, keep) and torch.equal(T2, Tc)
    Tn, Zn, vn, _ = batch(T1, None, sels, lr=lr, schurindex=si, wantZ=False, **Skw)  # copying form, no Z
    assert Zn is None and Tn.data_ptr() != T1.data_ptr() and torch.equal(T1.cpu(), torch.from_numpy(Th))
    with pytest.raises(psd_amd.DimensionMismatch):
        batch_(T1[:, :, :, :5], None, sels, lr=lr, schurindex=si, wantZ=False, **Skw)
    if fam.signed:
        with pytest.raises(psd_amd.DimensionMismatch):
            batch_(T1, None, sels, S=Skw["S"][:-1], lr=lr, schurindex=si, wantZ=False)
    # the other element type is refused, by an unsigned entry also where the tensor is the other unsigned entry's
    other = T1.real.contiguous() if fam.cplx else T1.to(torch.complex128)
    with pytest.raises(psd_amd.NotImplementedPSD):
        batch_(other, None, sels, lr=lr, schurindex=si, wantZ=False, **Skw)
    if not fam.signed:
        with pytest.raises(psd_amd.NotImplementedPSD):
            (D if fam.cplx else Z).method(eng, "ordschur_batch_")(T1, None, sels, lr=lr, schurindex=si, wantZ=False)
    if p > 2:
        with pytest.raises(ValueError):
            batch_(T1, Z1, sels, lr=lr, schurindex=2, **Skw)
    # an empty batch is returned as it is and describes itself like any other call
    infos = [7]
    Te, Ze, v0, st0 = batch_(T1[:0], Z1[:0], sels[:0], lr=lr, schurindex=si, infos_out=infos, **Skw)
    assert Te.shape[0] == 0 and v0.shape == (0, n) and infos == [] and st0.nlaunch_step == 0
    assert fam.method(eng, "ordschur_batch_stats").nsweeps == 0 and len(fam.method(eng, "ordschur_batch_nswaps")) == 0


def _chain_eigvecs(eng, lr, si, probs, values, sels, T1, Z1, values1):
    """D: the leading group's eigenvectors — the columns of the invariant subspace just moved to the top"""
    import evec_cases as vc

    nb, n = sels.shape
    p = len(probs[0])
    lead = np.zeros((nb, n), dtype=bool)
    for q in range(nb):
        lead[q, :int(closed_select(values[q], sels[q]).sum())] = True
    V, nvec = eng.eigvecs_batch(T1, Z1, values1, lead, lr=lr, schurindex=si)
    Vh, Th, Zh = V.cpu().numpy(), T1.cpu().numpy(), Z1.cpu().numpy()
    for q in range(nb):
        ps1 = psd_amd.PeriodicSchur([np.asfortranarray(Th[q, j]) for j in range(p)],
                                    [np.asfortranarray(Zh[q, j]) for j in range(p)], values1[q], lr, si)
        Vs = [Vh[q, l][:, :nvec[q]] for l in range(p)]
        lams = vc.order_values(ps1, lead[q])
        assert Vs[0].shape[1] == len(lams) == int(lead[q].sum())
        vc.ec.ev_check(probs[q], Vs, lams, left=(lr == "L"))
        assert vc.relation_ratio(probs[q], Vs, lams, left=(lr == "L")) <= vc.GATE, (lr, q)
