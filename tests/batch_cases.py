"""Cases for the batched Schur entries of the four families — Engine.[z|zg|dg]phessenberg_batch_ / pschur_batch_ /
pschur_batch / pschur_hess_batch_, gpschur_batch and zpschur_batch(..., S=...): many small problems of one shape (and, for
the signed families, one signature) in one call.  Each case takes an engine and a family (batch_common.Family);
tests/test_hostsim_*pschur_batch.py run them on the serial simulation, tests/test_gpu_*pschur_batch.py on the device.

Factors come from pt.bench_factors, I + G / (2 sqrt(n)): every factor is safely invertible, so every eigenvalue of a signed
product is finite, and random real factors give both real eigenvalues and conjugate pairs.

A case is one body where the families differ in names, element type, constants or the presence of S.  Where they check
different things the functions stand side by side: the Float64 family is compared with the single call on the same engine
(case_full_d, check_d) and has the (wr, wi) C ABI (case_abi_codes_d, case_dev_abi); the holes and the all-true signature
differ between real and complex."""
import ctypes as C

import numpy as np
import pytest

import batch_common as bcm
import engine_cases as ec
import psd_amd
import psdtest as pt
from batch_common import SIG22, SIG70, F, T, same_bits, sarr, shape_id, sig, work  # noqa: F401 (used by the test files)

# (nb, n, p).  (2, 33, 2) crosses the 8-row strip and the 4-column block of the update bodies and goes past one wavefront.
HESS_SHAPES = [(3, 2, 1), (3, 5, 1), (4, 9, 2), (2, 33, 2)]
# p >= 3: the single call of the device build takes the look-ahead form (other rounding); the simulation the one-stream form
HESS_SHAPES_P3 = [(3, 12, 3), (2, 17, 5)]
# (33, 6, 3) crosses the 32-problem chunk of the iteration
FULL_SHAPES = [(33, 6, 3), (5, 1, 4), (4, 2, 2), (3, 24, 1), (6, 20, 3), (2, 40, 8)]

# (nb, n, p) and the edge of the kernels each one covers
Z_SHAPES = [
    (3, 1, 3),    # n = 1: no sweep at all
    (4, 2, 2),    # smallest window
    (3, 5, 1),    # p = 1: H_{m-1} is H_m
    (5, 12, 3),   # one window, n < W
    (3, 40, 4),   # n > W = 32: several windows per sweep, off-window roles on all three sides
    (2, 30, 22),  # p >= 20: zero-shift pass first (st.ziter = -1), W = 20 < n
    (2, 14, 70),  # W = 10, window image ~ 123 KB: the LDS limit path
    (300, 3, 2),  # more workgroups than compute units
    (6, 20, 3),   # the group loop under PSD_BATCH_GROUP=4
]

# (nb, n, p, S for 'R') and the edge of the kernels each one covers; for 'L' the signature is reversed (true entry last)
ZG_SHAPES = [
    (3, 1, 3, (T, F, T)),       # n = 1: no sweep at all
    (4, 2, 2, (T, F)),          # smallest window, a pencil
    (5, 12, 3, (T, F, T)),      # one window
    (3, 40, 4, (T, F, F, T)),   # n > W; adjacent negative factors: both neighbour sides of stage 1, with and without the flip
    (3, 33, 4, (T, T, F, T)),   # a non-flipped factor with a flipped neighbour
    (2, 30, 22, SIG22),         # p >= 20: zero-shift pass first
    (2, 14, 70, SIG70),         # W = 10: the LDS limit path
    (300, 3, 2, (T, F)),        # more workgroups than compute units
    (6, 20, 3, (T, T, F)),      # the group loop under PSD_BATCH_GROUP=4
]
DG_SHAPES = [
    (3, 1, 3, (T, F, T)),       # n = 1: no sweep at all
    (4, 2, 2, (T, F)),          # the smallest problem: a single 2 x 2 block of a pencil
    (5, 12, 3, (T, F, T)),      # one window
    (3, 40, 4, (T, F, F, T)),   # n > W; adjacent negative factors: both neighbour sides of stage 1, with and without the flip
    (3, 33, 4, (T, T, F, T)),   # a non-flipped factor with a flipped neighbour, odd order
    (2, 30, 22, SIG22),         # p >= 20: zero-shift pass first, window below 32
    (2, 20, 70, SIG70),         # W = 16 for 8-byte elements: the LDS limit path, n above it
    (300, 3, 2, (T, F)),        # more workgroups than compute units
    (6, 20, 3, (T, T, F)),      # the group loop under PSD_BATCH_GROUP=4
]

# holes.  Z: (n, p, factor, index); ZG: (n, p, S, factor, index); DG: (S, factor, index) at n = p = 5
Z_HOLES = [(5, 3, 2, 3), (32, 4, 2, 3), (40, 4, 3, 20)]
ZG_HOLES = [(5, 5, tuple(S), l, j) for (S, l, j) in ec.RG_HOLES] + [(32, 4, (T, F, T, F), 2, 3), (40, 4, (T, T, F, T), 3, 30)]
DG_HOLES = [(tuple(S), l, j) for (S, l, j) in ec.RG_HOLES]

ONE_FAILS_SHAPE = (4, 24, 3, (T, F, T))
ONE_FAILS_MAXITFAC = 2


def problems(fam, shape):
    """The factors of a shape: built once, shared, never written to."""
    nb, n, p = shape[:3]
    return bcm.factors(fam.dtype, [fam.seed + 131 * q + 7 * n + p for q in range(nb)], n, p)


def reference_z(shape, q, lr):
    """(||P||_2, numpy's eigenvalues of the product, the oracle's eigenvalues) of problem q: computed once."""
    def make():
        A = problems(Z, shape)[q]
        P = pt.product(A, lr == "L")
        po = pt.oracle_zpschur(work(Z, A), lr)
        assert po.info == 0
        return (np.linalg.norm(P, 2), np.linalg.eigvals(P), po.values.copy())
    return bcm.cached(("ref", "Z", shape, q, lr), make)


def reference_g(fam, shape, q, lr, S=None):
    """The oracle's decomposition of problem q of a signed shape: computed once."""
    S = sig(shape, lr) if S is None else list(S)

    def make():
        po = pt.oracle_gpschur(work(fam, problems(fam, shape)[q]), S, lr)
        assert po.info == 0
        return po
    return bcm.cached(("ref", fam.name, shape[:3], tuple(S), q, lr), make)


def real_form(ps, what):
    """What the real entries promise beyond the complex ones: real Ts and Z, T at schurindex quasi-triangular with a zero
    sub-diagonal wherever the eigenvalue is real, the others triangular, the values of a 2 x 2 block exact conjugates."""
    n = ps.Ts[0].shape[0]
    assert all(t.dtype == np.float64 for t in ps.Ts) and all(z.dtype == np.float64 for z in ps.Z), what
    assert isinstance(ps, psd_amd.GeneralizedPeriodicSchur), what
    js = ps.schurindex - 1
    for l, t in enumerate(ps.Ts):
        assert np.all(np.tril(t, -2 if l == js else -1) == 0), (what, l)
    sub = np.diag(ps.Ts[js], -1) if n > 1 else np.zeros(0)
    i = 0
    while i < n:
        if i + 1 < n and sub[i] != 0:
            assert i + 2 >= n or sub[i + 1] == 0, (what, i)  # (blocks do not overlap)
            assert ps.values[i].imag != 0 and ps.values[i + 1] == np.conj(ps.values[i]), (what, i, ps.values[i:i + 2])
            i += 2
        else:
            assert ps.values[i].imag == 0 or not np.isfinite(ps.values[i]), (what, i, ps.values[i])
            i += 1


# ------------------------------------------------------------------------------------------------
# the checks of one problem
def check_d(A, ps, lr, single_values=None):
    """The checks of engine_cases.case_pschur_hess_batch, for a general Float64 problem in orientation lr."""
    n = A[0].shape[0]
    pt.pschur_check(A, ps, tol=100 * max(1.0, np.sqrt(n / 32)), check_lam=False)
    P = pt.product(A, lr == "L")
    sc = np.linalg.norm(P, 2)
    assert pt.match_eigs(np.linalg.eigvals(P), ps.values) <= 1e-10 * sc * max(1.0, np.linalg.cond(P) * 1e-6)
    if single_values is not None:
        assert pt.match_eigs(single_values, ps.values) <= 1e-10 * sc
    return sc


def check_problem_d(shape, q, ps, lr, A=None, S=None, ref=True):
    check_d(problems(D, shape)[q] if A is None else A, ps, lr)


def check_problem_z(shape, q, ps, lr, A=None, S=None, ref=True):
    nb, n, p = shape
    A = problems(Z, shape)[q] if A is None else A
    assert ps.orientation == lr and ps.schurindex == (p if lr == "L" else 1)
    pt.pschur_check(A, ps, tol=100 * max(1.0, np.sqrt(n / 32)), check_lam=False, real=False)
    if ref:
        sc, lam_np, lam_or = reference_z(shape, q, lr)
        e_np, e_or = pt.match_eigs(lam_np, ps.values), pt.match_eigs(lam_or, ps.values)
        print(f"{shape} {lr} q={q}: |lam - numpy| = {e_np:.3e}, |lam - oracle| = {e_or:.3e} (bound {1e-10 * sc:.3e})")
        assert e_np <= 1e-10 * sc, (shape, lr, q, e_np)
        assert e_or <= 1e-10 * sc, (shape, lr, q, e_or)
    for j, Tj in enumerate(ps.Ts):
        if j != ps.schurindex - 1:
            assert np.all(np.diag(Tj).imag == 0) and np.all(np.diag(Tj).real >= 0), (shape, lr, q, j)


def check_problem_g(fam, shape, q, ps, lr, A=None, S=None, ref=True):
    """a signed problem: the family's checker (and the real form), the eigenvalues against the oracle's"""
    nb, n, p = shape[:3]
    A = problems(fam, shape)[q] if A is None else A
    S = sig(shape, lr) if S is None else S
    what = (shape_id(shape), lr, q)
    assert ps.orientation == lr and ps.schurindex == (p if lr == "L" else 1) and ps.S == list(S), what
    out = fam.check(A, S, ps, tol=100 * max(1.0, np.sqrt(n / 32)), qtol=10 * max(1.0, np.sqrt(n / 32)))
    if not fam.cplx:
        real_form(ps, what)
    if ref:
        po = reference_g(fam, shape, q, lr, S)
        err = pt.match_eigs(po.values, ps.values)
        bound = 1e-8 * max(1.0, abs(po.values).max())
        if fam.cplx:
            print(f"{shape_id(shape)} {lr} q={q}: resid {max(out['resid']):.2f} eps n, orth {max(out['orth']):.2f} eps n, "
                  f"|lam - oracle| = {err:.3e} (bound {bound:.3e})")
        else:
            print(f"{shape_id(shape)} {lr} q={q}: |lam - oracle| = {err:.3e} (bound {bound:.3e}), "
                  f"{int((ps.values.imag > 0).sum())} pairs")
        assert err < bound, (what, err)


# ------------------------------------------------------------------------------------------------
# the eigenvalues of a problem against the family's own references, at the family's own bounds
def eigs_d(eng, A, values, S=None, shape=None, q=None):
    """Float64: against the single call on the same engine, 1e-10 ||P||_2"""
    assert pt.match_eigs(eng.pschur(A, "R").values, values) <= 1e-10 * np.linalg.norm(pt.product(A), 2)


def eigs_z(eng, A, values, S=None, shape=None, q=None):
    """ComplexF64: against numpy and the oracle (those of a shape's problem computed once), 1e-10 ||P||_2"""
    if shape is not None:
        sc, lam_np, lam_or = reference_z(shape, q, "R")
    else:
        P = pt.product(A)
        sc, lam_np, lam_or = np.linalg.norm(P, 2), np.linalg.eigvals(P), pt.oracle_zpschur(work(Z, A), "R").values
    assert pt.match_eigs(lam_np, values) <= 1e-10 * sc
    assert pt.match_eigs(lam_or, values) <= 1e-10 * sc


def eigs_g(fam, eng, A, values, S=None, shape=None, q=None):
    """signed: against the oracle (that of a shape's problem computed once), 1e-8 max(1, |lambda|max)"""
    po = reference_g(fam, shape, q, "R") if shape is not None else pt.oracle_gpschur(work(fam, A), S, "R")
    assert po.info == 0
    assert pt.match_eigs(po.values, values) < 1e-8 * max(1.0, abs(po.values).max())


# the bound of case_flags on the distance between the eigenvalues with and without Z
def flags_bound_d(shape, q, lr, values):
    return 1e-10 * np.linalg.norm(pt.product(problems(D, shape)[q], lr == "L"), 2)


def flags_bound_z(shape, q, lr, values):
    return 1e-10 * reference_z(shape, q, lr)[0]


def flags_bound_zg(shape, q, lr, values):
    return 1e-8 * max(1.0, abs(reference_g(ZG, shape, q, lr).values).max())


def flags_bound_dg(shape, q, lr, values):
    return 1e-9 * abs(values).max()  # (the bound of engine_cases.case_rg_fast_paths)


# ------------------------------------------------------------------------------------------------
# the families of this role.  seed: of problems(); small / group: the shapes of the flags, ABI and device-resident cases and
# of the group loop; check_problem: the checks of one problem of a shape; wrong: the other element type, which every entry
# refuses with wrong_exc (and a message that matches wrong_match); iter_single: the single iteration the simulation
# compares bit for bit; alone: case_full also runs first, last-but-one and last problem alone in a batch of one;
# hb_out_code: the code of a NULL output array at the pschur_hess_batch entry; eigs, flags_bound: the functions above;
# no_z: the device-resident call without Z, in the spelling of each family's own case
D = bcm.D.with_(shapes=FULL_SHAPES, hess_shapes=HESS_SHAPES, hess_shapes_p3=HESS_SHAPES_P3, seed=7000, small=(5, 12, 3),
                group=(6, 20, 3), check_problem=check_problem_d, wrong=np.complex128, wrong_exc=psd_amd.NotImplementedPSD,
                wrong_match=None, eigs=eigs_d, flags_bound=flags_bound_d,
                no_z=lambda eng, dA, S: eng.pschur_batch(dA, "R", wantZ=False))
Z = bcm.Z.with_(shapes=Z_SHAPES, holes=Z_HOLES, seed=9000, small=(5, 12, 3), group=(6, 20, 3), check_problem=check_problem_z,
                wrong=np.float64, wrong_exc=TypeError, wrong_match=None, eigs=eigs_z, flags_bound=flags_bound_z,
                no_z=lambda eng, dA, S: eng.zpschur_batch(dA, "R", wantZ=False),
                iter_single="zpschur_hess_", alone=True, hb_out_code=-10)
ZG = bcm.ZG.with_(shapes=ZG_SHAPES, holes=ZG_HOLES, seed=7000, small=ZG_SHAPES[2], group=ZG_SHAPES[8],
                  check_problem=lambda *a, **kw: check_problem_g(ZG, *a, **kw), eigs=lambda *a, **kw: eigs_g(ZG, *a, **kw),
                  flags_bound=flags_bound_zg, no_z=lambda eng, dA, S: eng.zpschur_batch(dA, "R", wantZ=False, S=S),
                  wrong=np.float64, wrong_exc=TypeError, wrong_match="ComplexF64 only",
                  iter_single="zpschur_hess_", alone=True, hb_out_code=-11)
DG = bcm.DG.with_(shapes=DG_SHAPES, holes=DG_HOLES, seed=9000, small=DG_SHAPES[2], group=DG_SHAPES[8],
                  check_problem=lambda *a, **kw: check_problem_g(DG, *a, **kw), eigs=lambda *a, **kw: eigs_g(DG, *a, **kw),
                  flags_bound=flags_bound_dg, no_z=lambda eng, dA, S: eng.dgpschur_batch_(dA, S, "R", wantZ=False),
                  wrong=np.complex128, wrong_exc=TypeError, wrong_match="Float64 only",
                  iter_single="gpschur_hess_", alone=False, hb_out_code=-11)


def hess_args(W):
    """(H_1, [H_2 ... H_p]) per problem, as pschur_hess_batch_ takes them"""
    return [(w[0], w[1:]) for w in W]


# ------------------------------------------------------------------------------------------------
# 1. reduction
def case_reduction_bits(eng, fam, shape, single_eng=None):
    """phessenberg_batch_ against the single reduction problem by problem: the same bodies in the same order.  Unsigned:
    phessenberg_ on the same engine — the packed H (reflectors below the diagonal included) and tau are equal bit for
    bit.  Signed (simulation): gphessenberg_ on `single_eng` with the serial stage 2 (PSD_HESS_SERIAL=1 in the
    environment of the single call) — H and Q are equal bit for bit."""
    nb, n, p = shape[:3]
    S = fam.sargs(sig(shape, "R")) if fam.signed else ()
    probs = problems(fam, shape)
    Wb = [work(fam, A) for A in probs]
    out, st = fam.method(eng, "phessenberg_batch_")(Wb, *S)
    assert len(out) == nb
    for q in range(nb):
        W1 = work(fam, probs[q])
        if fam.signed:
            H1, second = single_eng.gphessenberg_(W1, *S)
        else:
            H1, second, _ = eng.phessenberg_(W1)
            assert np.array_equal(second, out[q][1]), (shape, q)  # tau
        for j in range(p):
            assert np.array_equal(H1[j], out[q][0][j]), (shape_id(shape), q, j)
            if fam.signed:
                assert np.array_equal(second[j], out[q][1][j]), (shape_id(shape), q, j)  # Q
            else:
                assert np.array_equal(W1[j], Wb[q][j]), (shape, q, j)


def _q_from_reflectors(Apacked, tau, first):
    """Q = H_1 ... H_{n-1} from LAPACK-style storage, H_c = I - tau_c v v' (householder.jl:190-205): the reflector of
    column c acts on rows c + first ... n - 1 (first = 1 for the Hessenberg factor, 0 for the triangular ones).  A real
    reflector of a single row is the identity; a complex one is not."""
    n = Apacked.shape[0]
    last = n - 1 if np.iscomplexobj(Apacked) else n - 2
    Q = np.eye(n, dtype=Apacked.dtype)
    for c in range(n - 2, -1, -1):
        r0 = c + first
        if r0 > last:
            continue
        v = np.zeros(n, dtype=Apacked.dtype)
        v[r0] = 1.0
        v[r0 + 1:] = Apacked[r0 + 1:, c]
        Q -= tau[c] * np.outer(v, v.conj() @ Q)
    return Q


def case_reduction_close(eng, fam, shape):
    """For shapes whose single call rounds differently (look-ahead form, p >= 3 on the device): triu parts equal to
    1e-13 ||A||, the Q_j of the batched reduction orthogonal (unitary), and Q_j' A_j Q_{j+1} = H_j.

    Bounds: orthogonality 10 eps n as pt.pschur_check demands of Z; residual 10 n eps ||A_j||_F — n - 1 reflectors from
    either side, each a backward error of a few eps ||A_j||_F (Higham, Accuracy and Stability, Lemma 19.3)."""
    nb, n, p = shape
    probs = problems(fam, shape)
    Wb = [work(fam, A) for A in probs]
    out, st = fam.method(eng, "phessenberg_batch_")(Wb)
    for q in range(nb):
        A = probs[q]
        W1 = work(fam, A)
        H1, tau1, _ = eng.phessenberg_(W1)
        anorm = max(np.linalg.norm(a, 2) for a in A)
        Hb, taub = out[q]
        for j in range(p):
            d = np.abs(Hb[j] - H1[j]).max()
            print(f"{shape} q={q} j={j}: |H_batch - H_single| = {d:.3e} (bound {1e-13 * anorm:.3e})")
            assert d <= 1e-13 * anorm, (shape, q, j, d)
        Qs = [_q_from_reflectors(Wb[q][j], taub[j], 1 if j == 0 else 0) for j in range(p)]
        for j in range(p):
            orth = np.linalg.norm(Qs[j].conj().T @ Qs[j] - np.eye(n))
            assert orth < 10 * pt.EPS * n, (shape, q, j, orth)
            res = np.linalg.norm(Qs[j].conj().T @ A[j] @ Qs[(j + 1) % p] - Hb[j])
            assert res < 10 * n * pt.EPS * np.linalg.norm(A[j]), (shape, q, j, res)


def case_reduction(eng, fam, shape):
    """[zg|dg]phessenberg_batch_: pt.sg_hess_check per problem with the bounds of engine_cases.case_zg_phessenberg /
    case_rg_phessenberg for the order (20 max(1, n/8) and 10 max(1, n/16)); wantQ=False gives the same H."""
    nb, n, p = shape[:3]
    S = sig(shape, "R")
    probs = problems(fam, shape)
    hess = fam.method(eng, "phessenberg_batch_")
    Wb = [work(fam, A) for A in probs]
    out, st = hess(Wb, S)
    assert len(out) == nb
    for q in range(nb):
        Hs, Qs = out[q]
        assert all(Hs[j] is Wb[q][j] for j in range(p))  # in place
        assert all(h.dtype == fam.dtype for h in Hs) and all(x.dtype == fam.dtype for x in Qs)
        pt.sg_hess_check(probs[q], S, Hs, Qs, tol=20 * max(1, n / 8), qtol=10 * max(1, n / 16))
    noq, _ = hess([work(fam, A) for A in probs], S, wantQ=False)
    for q in range(nb):
        assert noq[q][1] == [] and all(np.array_equal(noq[q][0][j], out[q][0][j]) for j in range(p))


# ------------------------------------------------------------------------------------------------
# 2. full decomposition
def case_full_d(eng, shape, lr):
    """Float64: every problem against the single call on the same engine"""
    nb, n, p = shape
    probs = problems(D, shape)
    batch = eng.pschur_batch(probs, lr)
    assert len(batch) == nb
    for q in range(nb):
        assert batch[q].orientation == lr and batch[q].schurindex == (p if lr == "L" else 1)
        single = eng.pschur(work(D, probs[q]), lr)
        check_d(probs[q], batch[q], lr, single.values)
    # a problem does not depend on its neighbours: alone in a batch of one it gives the same spectrum
    for q in sorted({0, nb - 2, nb - 1} & set(range(nb))):
        alone = eng.pschur_batch([probs[q]], lr)
        sc = np.linalg.norm(pt.product(probs[q], lr == "L"), 2)
        assert pt.match_eigs(alone[0].values, batch[q].values) <= 1e-10 * sc, (shape, lr, q)


def case_full(eng, fam, shape, lr):
    nb, n, p = shape[:3]
    S = fam.sargs(sig(shape, lr)) if fam.signed else ()
    probs = problems(fam, shape)
    batch = fam.method(eng, "pschur_batch")(probs, *S, lr)
    assert len(batch) == nb
    for q in range(nb):
        fam.check_problem(shape, q, batch[q], lr)
    if fam.alone:
        # nothing is shared between the problems of a batch: alone in a batch of one a problem gives the same bits
        for q in sorted({0, nb - 2, nb - 1} & set(range(nb))):
            alone = fam.method(eng, "pschur_batch")([probs[q]], *S, lr)[0]
            same_bits(alone, batch[q], p, (shape_id(shape), lr, q))
    assert all(not a.flags.writeable for A in probs for a in A)  # (the copying form left its input alone)


def case_above_cap(eng, fam, n):
    """an order above the cap (nb = 2, p = 2): the single call's reduction and iteration, problem by problem on the batch
    buffer.  (The reduction's own checks run for the Float64 family alone: the family's parent case.)"""
    shape = (2, n, 2, (T, F))
    case_full(eng, fam, shape, "R")
    if not fam.cplx:
        case_reduction(eng, fam, shape)


# ------------------------------------------------------------------------------------------------
# 3. against the single call (simulation: built without contraction, the same bodies give the same bits)
def case_iteration_bits(eng, fam, single_eng, shape):
    """pschur_hess_batch_ on the reduced problems against the single iteration, problem by problem: T, Z, the values
    (alpha, beta and the scaling) and the sums of the counters.

    single_eng, ComplexF64: created with PSD_C3=0.  The batched kernel chases a window with the one-wave chain
    (psd_zq_sweep_window without the rotation table), factor after factor; the single call's default is the scan chase of
    psd_zchase3.h, which forms the rotations of all factors of a position from a chain of 2 x 2 products and agrees with
    the one-wave chain to rounding only.  With the scan chase off, and the trains off, the single call runs the same
    bodies as the batched kernel, and the bits are equal.
    single_eng, signed: with the signed trains off (and, Float64, the single-wave sweep: PSD_GSCAN=0)."""
    nb, n, p = shape[:3]
    probs = problems(fam, shape)
    one = getattr(single_eng, fam.iter_single)
    if fam.signed:
        S = sig(shape, "R")
        red, _ = fam.method(eng, "phessenberg_batch_")([work(fam, A) for A in probs], S)
        reduced = [work(fam, H) for H, _ in red]
        assert single_eng.get_train_g() == 0
        singles = [one(work(fam, H)[0], work(fam, H)[1:], S) for H in reduced]
        counters = ("nsweeps", "nrqpass", "ndefl2", "ndefl1", "nwindows", "reserved", "niter")
    else:
        S = None
        reduced = []
        for A in probs:
            Hs, _, _ = eng.phessenberg_(work(fam, A))
            reduced.append([np.asfortranarray(h) for h in Hs])
        keep = single_eng.get_train_z()
        single_eng.set_train_z(0)
        try:
            singles = [one(work(fam, H)[0], work(fam, H)[1:]) for H in reduced]
        finally:
            single_eng.set_train_z(keep)
        counters = ("nsweeps", "nrqpass", "ndefl2", "ndefl1", "nwindows")
    Wb = [work(fam, H) for H in reduced]
    batch = fam.method(eng, "pschur_hess_batch_")(hess_args(Wb), *fam.sargs(S))
    for q in range(nb):
        same_bits(singles[q], batch[q], p, (shape_id(shape), q))
        assert not fam.signed or batch[q].S == list(S)
    st = batch[0].stats
    for name in counters:
        assert getattr(st, name) == sum(getattr(s.stats, name) for s in singles), (shape_id(shape), name)
    if fam.signed:
        assert st.nsweeps > 0 or n <= (1 if fam.cplx else 2)
        if p >= 20:
            assert st.nrqpass > 0  # (the zero-shift pass came first)


def case_full_bits(eng, single_eng, shape, lr):
    """dgpschur_batch against pschur_(..., S=S) in the same form (trains off, serial stage 2, single-wave sweep)"""
    nb, n, p = shape[:3]
    S = sig(shape, lr)
    probs = problems(DG, shape)
    batch = eng.dgpschur_batch(probs, S, lr)
    for q in range(nb):
        one = single_eng.pschur_(work(DG, probs[q]), lr, S=S)
        same_bits(one, batch[q], p, (shape_id(shape), lr, q))


# ------------------------------------------------------------------------------------------------
# 4. place independence (Float64 signed)
def case_places(eng, shape):
    """Nothing is shared between the problems of a batch: one problem at several positions of one batch, and in batches
    of other sizes, gives the same bits."""
    nb, n, p = shape[:3]
    probs = problems(DG, shape)
    A, B = probs[0], probs[nb - 1]
    for lr in ("R", "L"):
        S = sig(shape, lr)
        alone = eng.dgpschur_batch([A], S, lr)[0]
        mixed = eng.dgpschur_batch([A, B, A, B, B, A], S, lr)
        for q in (0, 2, 5):
            same_bits(alone, mixed[q], p, (shape_id(shape), lr, q))
        for q in (3, 4):
            same_bits(mixed[1], mixed[q], p, (shape_id(shape), lr, q))
        pair = eng.dgpschur_batch([B, A], S, lr)
        same_bits(alone, pair[1], p, (shape_id(shape), lr, "pair"))
        same_bits(mixed[1], pair[0], p, (shape_id(shape), lr, "pair"))


# ------------------------------------------------------------------------------------------------
# 5. all-true and NULL signatures: ComplexF64 takes the path of zpschur_batch, Float64 stays on the signed kernels
def case_all_true_zg(eng, shape=(5, 12, 3, (T, T, T))):
    """An all-true signature takes the path of zpschur_batch: the same bits, through every entry."""
    nb, n, p = shape[:3]
    probs = problems(ZG, shape)
    for lr in ("R", "L"):
        ref = eng.zpschur_batch(probs, lr)
        for got in (eng.zgpschur_batch(probs, [True] * p, lr), eng.zpschur_batch(probs, lr, S=[True] * p)):
            for q in range(nb):
                same_bits(ref[q], got[q], p, (lr, q))
    red, _ = eng.zphessenberg_batch_([work(ZG, A) for A in probs])
    Ha, Hb = [work(ZG, H) for H, _ in red], [work(ZG, H) for H, _ in red]
    a = eng.zpschur_hess_batch_(hess_args(Ha))
    b = eng.zgpschur_hess_batch_(hess_args(Hb), [True] * p)
    for q in range(nb):
        same_bits(a[q], b[q], p, ("hess", q))
    # and S dispatches to the signed path when it has a negative entry
    S = [True, False, True]
    g = eng.zpschur_batch(probs, "R", S=S)
    h = eng.zgpschur_batch(probs, S, "R")
    for q in range(nb):
        assert isinstance(g[q], psd_amd.GeneralizedPeriodicSchur) and g[q].S == S
        same_bits(g[q], h[q], p, ("dispatch", q))


def case_all_true_dg(eng, shape=(5, 12, 3, (T, T, T))):
    """An all-true signature and none at all run the signed kernels: GeneralizedPeriodicSchur in the real form, the checks
    of case_full; both spellings give the same bits, through every entry."""
    nb, n, p = shape[:3]
    probs = problems(DG, shape)
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for lr in ("R", "L"):
        a = eng.dgpschur_batch(probs, [True] * p, lr)
        b = eng.dgpschur_batch(probs, None, lr)
        for q in range(nb):
            DG.check_problem(shape, q, a[q], lr)
            same_bits(a[q], b[q], p, (lr, q))
        # a NULL S at the C entry
        Wb = [work(DG, A) for A in probs]
        flat = [w for W in Wb for w in W]
        Zs = [np.zeros((n, n), order="F") for _ in range(nb * p)]
        al, be, sc = np.zeros((nb, n), dtype=np.complex128), np.zeros((nb, n)), np.zeros((nb, n), dtype=np.int32)
        si, info = C.c_int(0), C.c_int(0)
        rc = eng.lib.psd_d_gpschur_batch(eng.ctx, nb, n, p, eng._ptrs(flat), None, lr.encode(), 1, 1, 120, eng._ptrs(Zs),
                                         al.view(np.float64).ctypes.data_as(dp), be.ctypes.data_as(dp),
                                         sc.ctypes.data_as(i32p), None, C.byref(si), None, C.byref(info))
        assert rc == 0 and info.value == 0 and si.value == (p if lr == "L" else 1)
        for q in range(nb):
            assert np.array_equal(al[q], a[q].alpha) and np.array_equal(be[q], a[q].beta)
            assert all(np.array_equal(Wb[q][j], a[q].Ts[j]) and np.array_equal(Zs[q * p + j], a[q].Z[j]) for j in range(p))
    red, _ = eng.dgphessenberg_batch_([work(DG, A) for A in probs], None)
    red2, _ = eng.dgphessenberg_batch_([work(DG, A) for A in probs], [True] * p)
    Ha, Hb = [work(DG, H) for H, _ in red], [work(DG, H) for H, _ in red2]
    x = eng.dgpschur_hess_batch_(hess_args(Ha), None)
    y = eng.dgpschur_hess_batch_(hess_args(Hb), [True] * p)
    for q in range(nb):
        same_bits(x[q], y[q], p, ("hess", q))
        assert x[q].S == [True] * p


# ------------------------------------------------------------------------------------------------
# 6. flags
def case_flags(eng, fam):
    """wantZ=False and wantT=False, wantZ=False against the full run: the eigenvalues within the family's bound — 1e-10
    ||P||_2 unsigned, 1e-8 max(1, |lambda|max of the oracle) signed ComplexF64, 1e-9 |lambda|max signed Float64 (the
    bound of engine_cases.case_rg_fast_paths) —; a batch of one in place."""
    shape = fam.small
    nb, n, p = shape[:3]
    probs = problems(fam, shape)
    batch, batch_ = fam.method(eng, "pschur_batch"), fam.method(eng, "pschur_batch_")
    for lr in ("R", "L"):
        S = sig(shape, lr) if fam.signed else None
        Sa = fam.sargs(S)
        full = batch(probs, *Sa, lr)
        noz = batch(probs, *Sa, lr, wantZ=False)
        not_ = batch(probs, *Sa, lr, wantZ=False, wantT=False)
        for q in range(nb):
            assert noz[q].Z == [] and not_[q].Z == []
            e1, e2 = pt.match_eigs(full[q].values, noz[q].values), pt.match_eigs(full[q].values, not_[q].values)
            bound = fam.flags_bound(shape, q, lr, full[q].values)
            print(f"flags {lr} q={q}: {e1:.3e}, {e2:.3e} (bound {bound:.3e})")
            if fam.signed:
                assert e1 < bound and e2 < bound
            else:
                assert e1 <= bound and e2 <= bound
            for ps in (full[q], noz[q], not_[q]):
                assert ps.schurindex == (1 if lr == "R" else p) and ps.orientation == lr
                assert not fam.signed or ps.S == S
            js = full[q].schurindex - 1
            for j in range(p if fam.signed else 0):  # (without Z the factors still are the T factors)
                assert np.all(np.tril(noz[q].Ts[j], -2 if j == js and not fam.cplx else -1) == 0)
        W = work(fam, probs[0])
        b1 = batch_([W], *Sa, lr)
        assert b1[0].Ts[0] is W[0]  # in place
        if fam is D:  # a batch of one equals the plain call
            s1 = eng.pschur(probs[0], lr)
            check_d(probs[0], b1[0], lr, s1.values)
    # the copying form leaves its input alone (the shared factors are read-only: a write would have raised)
    assert all(not a.flags.writeable for A in probs for a in A)


# ------------------------------------------------------------------------------------------------
# 7. holes (Cases II and III): the three families build, bound and count them differently
def hole_id(h):
    """ZG: (n, p, S, factor, index); DG: (S, factor, index)"""
    if len(h) == 5:
        return "n%d_p%d_%s_f%d_i%d" % (h[0], h[1], "".join("T" if s else "F" for s in h[2]), h[3], h[4])
    return "%s_f%d_i%d" % ("".join("T" if s else "F" for s in h[0]), h[1], h[2])


def _zhole_problems(n, p, seed, shifted):
    def make(sd):
        A = ec.zhess_ut(n, p, sd)
        if shifted:
            A = [np.asfortranarray(a + 2 * np.eye(n)) if k > 0 else a for k, a in enumerate(A)]
        return A
    return [make(seed + 1000), make(seed), make(seed + 2000)]


def case_holes_z(eng, hole):
    """An exact zero on the diagonal of a triangular factor (engine_cases.case_zholes), in a batch between two untouched
    problems of the same shape."""
    n, p, fac, idx = hole
    probs = _zhole_problems(n, p, 80 + p + n, n > 32)
    probs[1][fac - 1][idx - 1, idx - 1] = 0
    Wb = [work(Z, A) for A in probs]
    out = eng.zpschur_hess_batch_(hess_args(Wb))
    case2 = 0
    for q in range(3):
        pt.gpschur_check(probs[q], [True] * p, out[q], tol=100 * max(1, n / 32))
        po = pt.oracle_zpschur_hess(probs[q][0], probs[q][1:], [True] * p)
        fin = np.isfinite(po.values)
        err = pt.match_eigs(po.values[fin], out[q].values[fin])
        print(f"{hole} q={q}: |lam - oracle| = {err:.3e} (bound {1e-10 * abs(po.values[fin]).max():.3e})")
        assert err <= 1e-10 * abs(po.values[fin]).max(), (hole, q, err)
        nq = int((po.sweeplog[:, 0] == 2).sum())
        if q == 1:
            assert nq == 1, (hole, nq)  # (the oracle's count at the holed problem)
        case2 += nq
    # the call's stats are sums over its problems: the holed problem's count is what the untouched ones leave of it
    assert out[0].stats.ndefl2 == case2, (hole, out[0].stats.ndefl2, case2)


def case_holes_zg(eng, hole):
    """An exact zero on the diagonal of a triangular factor — of a +1 factor (Case II, a zero eigenvalue) or of a -1
    factor (Case III, an infinite one: beta == 0) — built as engine_cases.case_zg_holes builds it, in a batch between two
    untouched problems of the same shape.  The counts of finite values and of Cases II / III equal the oracle's, and the
    call's stats are the sums over the three problems."""
    n, p, S, fac, idx = hole
    S = list(S)
    probs = _zhole_problems(n, p, 1900 if n == 5 else 140 + n + p, n > 5)
    probs[1][fac - 1][idx - 1, idx - 1] = 0.0
    Wb = [work(ZG, A) for A in probs]
    out = eng.zgpschur_hess_batch_(hess_args(Wb), S)
    c2 = c3 = 0
    for q in range(3):
        pt.gpschur_check(probs[q], S, out[q], tol=100 * max(1, n / 32))
        po = pt.oracle_zpschur_hess(probs[q][0], probs[q][1:], S)
        assert po.info == 0
        fin, gfin = np.isfinite(po.values), np.isfinite(out[q].values)
        assert fin.sum() == gfin.sum(), (hole, q)
        rtol = 1e-9 if n == 5 else 1e-8
        err = pt.match_eigs(po.values[fin], out[q].values[gfin])
        print(f"{hole_id(hole)} q={q}: finite {fin.sum()}/{n}, |lam - oracle| = {err:.3e} "
              f"(bound {rtol * max(1.0, abs(po.values[fin]).max()):.3e})")
        assert err < rtol * max(1.0, abs(po.values[fin]).max()), (hole, q, err)
        n2, n3 = int((po.sweeplog[:, 0] == 2).sum()), int((po.sweeplog[:, 0] == 3).sum())
        if q == 1:
            assert n2 + n3 >= 1, hole
            if S[fac - 1]:  # a zero in a +1 factor: a zero eigenvalue
                assert n2 >= 1 and np.any(out[q].values == 0), hole
            else:           # a zero in a -1 factor: an infinite eigenvalue
                assert n3 >= 1 and (out[q].beta == 0).sum() >= 1 and gfin.sum() < n, hole
        c2 += n2
        c3 += n3
    st = out[0].stats
    assert (st.reserved % 1000, st.reserved // 1000) == (c2, c3), (hole, st.reserved, c2, c3)
    assert st.ndefl2 == c2


def case_holes_dg(eng, hole):
    """An exact zero on the diagonal of a triangular factor — of a +1 factor (Case II) or of a -1 factor (Case III) — in
    Hessenberg-triangular inputs as engine_cases.rg_hess_ut makes them (n = p = 5, the RG_HOLES table), in a batch
    between two hole-free problems.  Finite eigenvalues match pt.oracle_gpschur_hess within 1e-9 max(1, |lambda|max)
    (engine_cases._rg_match_oracle) and as many are infinite; `reserved` is the sum of the oracle's Case II and III counts;
    the hole-free neighbours give the bits they give in a batch without the hole."""
    S, fac, idx = hole
    S = list(S)
    n = p = 5
    probs = [ec.rg_hess_ut(n, p, 1900), ec.rg_hess_ut(n, p, 900), ec.rg_hess_ut(n, p, 2900)]
    probs[1][fac - 1][idx - 1, idx - 1] = 0.0
    Wb = [work(DG, A) for A in probs]
    out = eng.dgpschur_hess_batch_(hess_args(Wb), S)
    c2 = c3 = 0
    for q in range(3):
        pt.rgpschur_check(probs[q], S, out[q])
        real_form(out[q], (hole_id(hole), q))
        po = pt.oracle_gpschur_hess(probs[q][0], probs[q][1:], S)
        assert po.info == 0
        fin, gfin = np.isfinite(po.values), np.isfinite(out[q].values)
        assert fin.sum() == gfin.sum(), (hole, q)
        err = pt.match_eigs(po.values[fin], out[q].values[gfin])
        bound = 1e-9 * max(1.0, abs(po.values[fin]).max())
        print(f"{hole_id(hole)} q={q}: finite {fin.sum()}/{n}, |lam - oracle| = {err:.3e} (bound {bound:.3e})")
        assert err < bound, (hole, q, err)
        if q == 1:
            assert po.counters["case2"] + po.counters["case3"] >= 1, hole
        c2 += po.counters["case2"]
        c3 += po.counters["case3"]
    st = out[0].stats
    assert (st.reserved % 1000, st.reserved // 1000) == (c2, c3), (hole, st.reserved, c2, c3)
    Wc = [work(DG, probs[0]), work(DG, probs[2])]
    clean = eng.dgpschur_hess_batch_(hess_args(Wc), S)
    same_bits(clean[0], out[0], p, (hole_id(hole), "left neighbour"))
    same_bits(clean[1], out[2], p, (hole_id(hole), "right neighbour"))


# ------------------------------------------------------------------------------------------------
# 8. one failing problem
def one_fails_problems(fam, n=24, p=3):
    """Three problems whose product needs a handful of sweeps — triangular factors with one 3 x 3 block in A_1 (already
    Hessenberg-triangular: every reflector of the reduction is the identity) — around one full random problem."""
    def easy(seed):
        A = [np.triu(a) for a in pt.bench_factors(n, p, seed=seed, dtype=fam.dtype)]
        full = pt.bench_factors(n, 1, seed=seed + 977, dtype=fam.dtype)[0]
        for k in (9, 10):
            A[0][k + 1, k] = full[k + 1, k]
        return [np.asfortranarray(a) for a in A]
    return [easy(41), pt.bench_factors(n, p, seed=42, dtype=fam.dtype), easy(43), easy(44)]


def case_one_fails(eng, fam, single_pattern=False):
    """maxitfac = 2 (2 n sweeps, PSD.jl:471,891-893; signed: S = (T, F, T)): the full problem cannot deflate 24
    eigenvalues within its budget of 48 iterations and ends alone; the three nearly triangular ones are complete and
    correct.  The reference does the same on these inputs — ComplexF64: the oracle's codes are (0, 15, 0, 0) after 34,
    48, 32 and 33 of 48 iterations; signed ComplexF64: (0, 16, 0, 0), after 36, 48, 32 and 33 iterations; for the signed
    families the oracle's codes with this maxitfac are asserted here: non-zero for the second problem alone.
    single_pattern (Float64, simulation): the single call with the same maxitfac fails for exactly that one."""
    S = list(ONE_FAILS_SHAPE[3]) if fam.signed else None
    Sa = fam.sargs(S)
    probs = one_fails_problems(fam)
    n = probs[0][0].shape[0]
    if single_pattern:
        for q, A in enumerate(probs):
            if q == 1:
                with pytest.raises(psd_amd.ConvergenceError):
                    eng.pschur(A, "R", maxitfac=ONE_FAILS_MAXITFAC)
            else:
                eng.pschur(A, "R", maxitfac=ONE_FAILS_MAXITFAC)
    if fam.signed:
        codes = [pt.oracle_gpschur(work(fam, A), S, "R", maxitfac=ONE_FAILS_MAXITFAC).info for A in probs]
        assert codes[1] != 0 and codes[0] == codes[2] == codes[3] == 0, codes
    infos = []
    out = fam.method(eng, "pschur_batch")(probs, *Sa, "R", maxitfac=ONE_FAILS_MAXITFAC, infos_out=infos)
    assert len(infos) == 4 and infos[0] == 0 and infos[2] == 0 and infos[3] == 0, infos
    assert psd_amd.INFO_NOCONV < infos[1] <= psd_amd.INFO_NOCONV + n, infos  # PSD_INFO_NOCONV + level
    for q in (0, 2, 3):  # complete and correct, by the family's own yardsticks
        fam.check_problem(ONE_FAILS_SHAPE[:3 + fam.signed], None, out[q], "R", A=probs[q], S=S, ref=False)
        if fam is not D:  # (Float64 has compared with the product's eigenvalues; its single call got maxitfac = 2 above)
            fam.eigs(eng, probs[q], out[q].values, S)
    Ws = [work(fam, A) for A in probs]
    with pytest.raises(psd_amd.ConvergenceError):  # raised after all four have run
        fam.method(eng, "pschur_batch_")(Ws, *Sa, "R", maxitfac=ONE_FAILS_MAXITFAC)
    for q in (0, 2, 3):  # ... so the in-place factors of the others are their T factors
        if fam is D:
            assert np.all(np.tril(Ws[q][0], -2) == 0) and all(np.all(np.tril(w, -1) == 0) for w in Ws[q][1:])
            assert pt.match_eigs(out[q].values, np.linalg.eigvals(pt.product(Ws[q]))) <= 1e-10 * np.linalg.norm(pt.product(probs[q]), 2)
        elif fam.cplx:
            assert all(np.all(np.tril(w, -1) == 0) for w in Ws[q])
        assert all(np.array_equal(Ws[q][j], out[q].Ts[j]) for j in range(3))


# ------------------------------------------------------------------------------------------------
# 9. gpschur_batch: pencils and longer pair sequences, ComplexF64 (the default) and real=True
def _pairs(fam, nb, n, ph, seed):
    As = [pt.bench_factors(n, ph, seed=seed + 17 * q, dtype=fam.dtype) for q in range(nb)]
    Bs = [pt.bench_factors(n, ph, seed=seed + 17 * q + 5000, dtype=fam.dtype) for q in range(nb)]
    return As, Bs


def case_gpschur_batch(eng):
    """One pair: the QZ problem of the pencil (A, B), against numpy's eigenvalues of B^-1 A at n = 6.  Bound
    1e-10 max(1, |lambda|max): both methods are backward stable (errors of a few n eps in A and B), B = I + G / (2 sqrt n)
    has a condition number below 10 and the eigenvalues of such a pencil condition numbers of order 10, so the
    difference is of order 1e-13; three digits are left for an unlucky draw.  Three pairs: against Engine.gpschur
    problem by problem within 1e-8 max(1, |lambda|max), the bound of engine_cases.case_zg_full (the single call runs
    trains and the pipelined stage 2, so it rounds differently)."""
    n = 6
    As, Bs = _pairs(ZG, 4, n, 1, 300)
    out = eng.gpschur_batch(As, Bs)
    assert len(out) == 4
    for q in range(4):
        lam = np.linalg.eigvals(np.linalg.solve(Bs[q][0], As[q][0]))
        err = pt.match_eigs(lam, out[q].values)
        print(f"pencil q={q}: |lam - numpy| = {err:.3e} (bound {1e-10 * max(1.0, abs(lam).max()):.3e})")
        assert err < 1e-10 * max(1.0, abs(lam).max()), (q, err)
        assert out[q].S == [True, False] and out[q].period == 2
    As, Bs = _pairs(ZG, 3, n, 3, 400)
    out = eng.gpschur_batch(As, Bs)
    for q in range(3):
        one = eng.gpschur(As[q], Bs[q])
        err = pt.match_eigs(one.values, out[q].values)
        print(f"three pairs q={q}: |lam - gpschur| = {err:.3e}")
        assert err < 1e-8 * max(1.0, abs(one.values).max()), (q, err)
        assert out[q].S == one.S and out[q].period == 6
        # the interleaving is gpschur's: the factors decompose the same sequence
        Cs = [As[q][2], Bs[q][1], As[q][1], Bs[q][0], As[q][0], Bs[q][2]]
        pt.gpschur_check(Cs, out[q].S, out[q])
    assert eng.gpschur_batch([], []) == []
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.gpschur_batch(As, Bs[:2])
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.gpschur_batch([As[0], As[1][:2]], [Bs[0], Bs[1][:2]])


def case_gpschur_batch_real(eng):
    """real=True against the loop of Engine.gpschur per pair: real output, eigenvalues within 1e-8 max(1, |lambda|max) (the
    bound of engine_cases.case_rg_full_sizes: the single call runs trains and the pipelined stage 2, so it rounds
    differently); the factors decompose gpschur's interleaving.  The default stays the ComplexF64 path."""
    n = 6
    for nb, ph, seed in ((4, 1, 300), (3, 3, 400)):
        As, Bs = _pairs(DG, nb, n, ph, seed)
        out = eng.gpschur_batch(As, Bs, real=True)
        assert len(out) == nb
        for q in range(nb):
            one = eng.gpschur(As[q], Bs[q])
            err = pt.match_eigs(one.values, out[q].values)
            print(f"{ph} pairs q={q}: |lam - gpschur| = {err:.3e}")
            assert err < 1e-8 * max(1.0, abs(one.values).max()), (q, err)
            assert out[q].S == one.S == [True, False] * ph and out[q].period == 2 * ph
            real_form(out[q], (ph, q))
            if ph == 1:
                Cs = [As[q][0], Bs[q][0]]
            else:
                Cs = [As[q][2], Bs[q][1], As[q][1], Bs[q][0], As[q][0], Bs[q][2]]
            pt.rgpschur_check(Cs, out[q].S, out[q])
    dflt = eng.gpschur_batch(As, Bs)
    assert all(t.dtype == np.complex128 for t in dflt[0].Ts)  # (the default is untouched)
    assert eng.gpschur_batch([], [], real=True) == []
    with pytest.raises(TypeError):
        eng.gpschur_batch([[a.astype(np.complex128) for a in As[0]]], [Bs[0]], real=True)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.gpschur_batch(As, Bs[:2], real=True)


# ------------------------------------------------------------------------------------------------
# 10. argument errors
def case_argument_errors(eng, fam):
    batch, batch_ = fam.method(eng, "pschur_batch"), fam.method(eng, "pschur_batch_")
    hess = fam.method(eng, "phessenberg_batch_")
    hessb = fam.method(eng, "pschur_hess_batch_") if fam is not D else None
    if fam.signed:
        A = problems(fam, fam.shapes[2])   # n = 12, p = 3
        B = problems(fam, fam.shapes[1])   # n = 2, p = 2
        S3, S2 = [T, F, T], [T, F]
        unequal_order = [A[0], B[0] + B[0][:1]]
    else:
        A = problems(fam, (3, 5, 1))
        B = problems(fam, (4, 9, 2) if fam is D else (4, 2, 2))
        S3 = S2 = None
        unequal_order = [A[0], B[0][:1]]
    a3, a2 = fam.sargs(S3), fam.sargs(S2)
    with pytest.raises(psd_amd.DimensionMismatch):
        batch(unequal_order, *a3)  # unequal order
    with pytest.raises(psd_amd.DimensionMismatch):
        batch([B[0], B[1][:1]], *a2)  # unequal period
    if fam.signed:
        with pytest.raises(psd_amd.DimensionMismatch):
            batch(A, S2)  # one entry of S per factor
        with pytest.raises(psd_amd.DimensionMismatch):
            hess([work(fam, a) for a in A], S2)
        with pytest.raises(psd_amd.DimensionMismatch):
            hessb(hess_args([work(fam, a) for a in A]), S2)
        with pytest.raises(psd_amd.DimensionMismatch):
            batch([[a[:, :5] for a in A[0]]], S3)  # not square
        with pytest.raises(ValueError):
            batch(A, [F, T, T], "R")  # the leftmost entry must be true
        with pytest.raises(ValueError):
            batch(A, [T, T, F], "L")
        with pytest.raises(ValueError):
            hess([work(fam, a) for a in A], [F, T, T])
        with pytest.raises(ValueError):
            hessb(hess_args([work(fam, a) for a in A]), [F, T, T])
        if fam.cplx:
            with pytest.raises(ValueError):
                eng.zpschur_batch(A, "R", S=[F, T, T])
    else:
        with pytest.raises(psd_amd.DimensionMismatch):
            hess([work(fam, B[0]), work(fam, A[0])])
        if hessb is not None:
            with pytest.raises(psd_amd.DimensionMismatch):
                hessb(hess_args([work(fam, B[0]), work(fam, A[0])]))
    inplace = A if fam.signed else B
    with pytest.raises(TypeError):
        batch_([[np.ascontiguousarray(a) for a in inplace[0]]], *a3)  # in place needs Fortran order
    with pytest.raises(ValueError):
        batch(A, *a3, "X")
    # the wrong family
    other = [[np.asfortranarray(a.astype(fam.wrong) if fam.wrong is np.complex128 else a.real.copy()) for a in A[0]]]
    entries = [batch, batch_] if fam is D else [batch, batch_, hess]
    for f in entries:
        with pytest.raises(fam.wrong_exc, match=fam.wrong_match):
            f(other, *a3)
    if hessb is not None:
        with pytest.raises(fam.wrong_exc, match=fam.wrong_match):
            hessb([(other[0][0], other[0][1:])], *a3)
    assert batch([], *a3) == [] and batch_([], *a3, "L") == []
    if hessb is not None:
        assert hessb([], *a3) == [] and hess([], *a3)[0] == []
    infos = [7]
    assert batch([], *a3, infos_out=infos) == [] and infos == []
    if fam is Z:  # the real family still refuses complex input
        with pytest.raises(psd_amd.NotImplementedPSD):
            eng.pschur_batch([A[0]])
        with pytest.raises(psd_amd.NotImplementedPSD):
            eng.pschur_batch_([work(fam, A[0])])


# ------------------------------------------------------------------------------------------------
# 11. the C ABI.  Float64: eigenvalues as (wr, wi) and the reduction's tau; the other families (alpha, beta, scale)
def case_abi_codes_d(eng, shape=(5, 12, 3)):
    """The argument codes of the four C entries of the Float64 family: the return value and *info agree, code by code.
    Every call ends in the argument checks, so the pointers are never followed (the packed host block stands in for a
    device buffer)."""
    nb, n, p = shape
    probs = problems(D, shape)
    lib, ctx = eng.lib, eng.ctx
    dp = C.POINTER(C.c_double)
    A = work(D, probs[0])
    ptrs = eng._ptrs(A)
    dA = np.ascontiguousarray(np.array([pt.pack(A)]))
    buf = C.c_void_p(dA.ctypes.data)
    tau, w = np.zeros((p, n)), np.zeros(n)
    wp, tp = w.ctypes.data_as(dp), tau.ctypes.data_as(dp)

    def both(call):
        """the code of a call, returned and stored alike"""
        info = C.c_int(12345)
        rc = call(C.byref(info))
        assert rc == info.value, (rc, info.value)
        return rc

    def hess(c=ctx, nb_=1, n_=n, p_=p, A_=ptrs, tau_=tp):
        return both(lambda ip: lib.psd_d_phessenberg_batch(c, nb_, n_, p_, A_, tau_, None, ip))

    def host_(c=ctx, nb_=1, n_=n, p_=p, A_=ptrs, o=b"R", mi=30, wz=0, Z_=None, wr_=wp, wi_=wp):
        return both(lambda ip: lib.psd_d_pschur_batch(c, nb_, n_, p_, A_, o, 1, wz, mi, Z_, wr_, wi_, None, None, None, ip))

    def dev_(c=ctx, nb_=1, n_=n, p_=p, A_=buf, o=b"R", mi=30, wz=0, Z_=None, wr_=wp, wi_=wp):
        return both(lambda ip: lib.psd_d_pschur_batch_dev(c, nb_, n_, p_, A_, o, 1, wz, mi, Z_, wr_, wi_, None, None, None, ip))

    def hb_(c=ctx, nb_=1, n_=n, p_=p, H_=ptrs, mi=30, wz=0, Q_=None, wr_=wp, wi_=wp):
        return both(lambda ip: lib.psd_d_pschur_hess_batch(c, nb_, n_, p_, H_, Q_, 1, wz, mi, wr_, wi_, None, None, ip))

    assert hess(c=None) == -1 and hess(nb_=0) == -2 and hess(n_=0) == -3 and hess(p_=0) == -4
    assert hess(A_=None) == -5 and hess(tau_=None) == -6
    for f in (host_, dev_):
        assert f(c=None) == -1 and f(nb_=0) == -2 and f(nb_=-3) == -2 and f(n_=0) == -3 and f(p_=0) == -4
        assert f(A_=None) == -5 and f(o=b"X") == -6 and f(mi=0) == -9 and f(wz=1) == -10
        assert f(wr_=None) == -11 and f(wi_=None) == -11
    assert hb_(c=None) == -1 and hb_(nb_=0) == -2 and hb_(nb_=33) == -2  # (at most 32 problems side by side)
    assert hb_(n_=0) == -3 and hb_(p_=0) == -4  # (returned and stored alike: the codes of psd_z_pschur_hess_batch)
    assert hb_(H_=None) == -5 and hb_(wz=1) == -6 and hb_(mi=0) == -9 and hb_(wr_=None) == -10 and hb_(wi_=None) == -10
    # the first bad argument decides
    assert hb_(nb_=33, n_=0) == -2 and hb_(n_=0, p_=0) == -3 and host_(nb_=0, n_=0) == -2 and dev_(p_=0, A_=None) == -4
    # a null info is allowed
    assert lib.psd_d_pschur_hess_batch(ctx, 1, 0, p, ptrs, None, 1, 0, 30, wp, wp, None, None, None) == -3
    assert lib.psd_d_pschur_batch(ctx, 0, n, p, ptrs, b"R", 1, 0, 30, None, wp, wp, None, None, None, None) == -2


def case_dev_abi(eng, shape=(5, 12, 3)):
    """psd_d_pschur_batch_dev through the C ABI on packed [nb][p][n][n] column-major blocks (in the simulation device
    memory is host memory): the same bits as the host entry, and the argument codes of all three entries."""
    nb, n, p = shape
    probs = problems(D, shape)
    dp = C.POINTER(C.c_double)
    for lr in ("R", "L"):
        host = eng.pschur_batch(probs, lr)
        dA = np.ascontiguousarray(np.array([pt.pack(A) for A in probs]))
        dZ = np.zeros_like(dA)
        wr, wi = np.zeros((nb, n)), np.zeros((nb, n))
        infos = (C.c_int * nb)()
        si, info = C.c_int(0), C.c_int(0)
        st = psd_amd.Stats()
        rc = eng.lib.psd_d_pschur_batch_dev(eng.ctx, nb, n, p, C.c_void_p(dA.ctypes.data), lr.encode(), 1, 1, 30,
                                            C.c_void_p(dZ.ctypes.data), wr.ctypes.data_as(dp), wi.ctypes.data_as(dp),
                                            infos, C.byref(si), C.byref(st), C.byref(info))
        assert rc == 0 and info.value == 0 and si.value == (p if lr == "L" else 1) and not any(infos)
        assert st.ms_total >= st.ms_hess >= 0 and st.nsweeps > 0
        for q in range(nb):
            assert np.array_equal(wr[q] + 1j * wi[q], host[q].values)
            for j in range(p):
                assert np.array_equal(dA[q, j].T, host[q].Ts[j]) and np.array_equal(dZ[q, j].T, host[q].Z[j])
    lib, ctx = eng.lib, eng.ctx
    A = work(D, probs[0])
    ptrs = eng._ptrs(A)
    tau = np.zeros((p, n))
    w = np.zeros(n)
    wp, tp = w.ctypes.data_as(dp), tau.ctypes.data_as(dp)
    buf = C.c_void_p(dA.ctypes.data)

    def hess(nb_=1, n_=n, p_=p, A_=ptrs, tau_=tp):
        return lib.psd_d_phessenberg_batch(ctx, nb_, n_, p_, A_, tau_, None, None)

    def host_(nb_=1, n_=n, p_=p, A_=ptrs, o=b"R", mi=30, wz=0, Z_=None, wr_=wp):
        return lib.psd_d_pschur_batch(ctx, nb_, n_, p_, A_, o, 1, wz, mi, Z_, wr_, wp, None, None, None, None)

    def dev_(nb_=1, n_=n, p_=p, A_=buf, o=b"R", mi=30, wz=0, Z_=None, wr_=wp):
        return lib.psd_d_pschur_batch_dev(ctx, nb_, n_, p_, A_, o, 1, wz, mi, Z_, wr_, wp, None, None, None, None)

    assert hess(nb_=0) == -2 and hess(n_=0) == -3 and hess(p_=0) == -4 and hess(A_=None) == -5 and hess(tau_=None) == -6
    for f in (host_, dev_):
        assert f(nb_=0) == -2 and f(n_=0) == -3 and f(p_=0) == -4 and f(A_=None) == -5 and f(o=b"X") == -6
        assert f(mi=0) == -9 and f(wz=1) == -10 and f(wr_=None) == -11
    assert lib.psd_d_pschur_batch(None, 1, n, p, ptrs, b"R", 1, 0, 30, None, wp, wp, None, None, None, None) == -1


def case_abi_codes(eng, fam, devbuf=None):
    """The argument codes of the four C entries, and (simulation, where device memory is host memory: `devbuf` None)
    pschur_batch_dev on packed blocks against the host entry, bit for bit.  `devbuf`: the address of one packed problem
    in device memory for the calls of the device entry that go through."""
    shape = fam.small
    nb, n, p = shape[:3]
    probs = problems(fam, shape)
    dp = C.POINTER(C.c_double)
    i32p = C.POINTER(C.c_int32)
    lib, ctx, mi0 = eng.lib, eng.ctx, fam.maxitfac
    fhess, fhost = fam.entry(eng, "phessenberg_batch"), fam.entry(eng, "pschur_batch")
    fdev, fhb = fam.entry(eng, "pschur_batch_dev"), fam.entry(eng, "pschur_hess_batch")

    def sg(S):
        """the signature where the entries of the family take one"""
        return (S,) if fam.signed else ()

    for lr in ("R", "L") if devbuf is None else ():
        S = sarr(sig(shape, lr)) if fam.signed else None
        host = fam.method(eng, "pschur_batch")(probs, *fam.sargs(sig(shape, lr) if fam.signed else None), lr)
        dA = np.ascontiguousarray(np.array([pt.pack(A, fam.dtype) for A in probs]))
        dZ = np.zeros_like(dA)
        alpha, beta = np.zeros((nb, n), dtype=np.complex128), np.zeros((nb, n))
        sc = np.zeros((nb, n), dtype=np.int32)
        infos = (C.c_int * nb)()
        si, info = C.c_int(0), C.c_int(0)
        st = psd_amd.Stats()
        rc = fdev(ctx, nb, n, p, C.c_void_p(dA.ctypes.data), *sg(S), lr.encode(), 1, 1, mi0, C.c_void_p(dZ.ctypes.data),
                  alpha.view(np.float64).ctypes.data_as(dp), beta.ctypes.data_as(dp), sc.ctypes.data_as(i32p), infos,
                  C.byref(si), C.byref(st), C.byref(info))
        assert rc == 0 and info.value == 0 and si.value == (p if lr == "L" else 1) and not any(infos)
        assert st.ms_total >= st.ms_hess >= 0 and st.nsweeps > 0
        for q in range(nb):
            assert np.array_equal(pt.gvalues(alpha[q], beta[q], sc[q]), host[q].values)
            if fam.signed:
                assert np.array_equal(alpha[q], host[q].alpha) and np.array_equal(beta[q], host[q].beta)
                assert np.array_equal(sc[q], host[q].alphascale)
            for j in range(p):
                assert np.array_equal(dA[q, j].T, host[q].Ts[j]) and np.array_equal(dZ[q, j].T, host[q].Z[j])
    A = work(fam, probs[0])
    ptrs = eng._ptrs(A)
    tau = np.zeros((p, n), dtype=np.complex128)
    al, be, sc1 = np.zeros(n, dtype=np.complex128), np.zeros(n), np.zeros(n, dtype=np.int32)
    ap, bp, sp = al.view(np.float64).ctypes.data_as(dp), be.ctypes.data_as(dp), sc1.ctypes.data_as(i32p)
    tp = tau.view(np.float64).ctypes.data_as(dp)
    buf = C.c_void_p(dA.ctypes.data if devbuf is None else devbuf)
    SR, SL = sarr([T, F, T]), sarr([F, T, T])  # SL: leftmost in working order true for 'L' only

    def hess(nb_=1, n_=n, p_=p, A_=ptrs, S_=SR, tau_=tp):
        if fam.signed:
            return fhess(ctx, nb_, n_, p_, A_, S_, None, None, None)
        return fhess(ctx, nb_, n_, p_, A_, tau_, None, None)

    def host_(nb_=1, n_=n, p_=p, A_=ptrs, S_=SR, o=b"R", mi=mi0, wz=0, Z_=None, al_=ap, be_=bp, sc_=sp):
        return fhost(ctx, nb_, n_, p_, A_, *sg(S_), o, 1, wz, mi, Z_, al_, be_, sc_, None, None, None, None)

    def dev_(nb_=1, n_=n, p_=p, A_=buf, S_=SR, o=b"R", mi=mi0, wz=0, Z_=None, al_=ap, be_=bp, sc_=sp):
        return fdev(ctx, nb_, n_, p_, A_, *sg(S_), o, 1, wz, mi, Z_, al_, be_, sc_, None, None, None, None)

    def hb_(nb_=1, n_=n, p_=p, H_=ptrs, S_=SR, mi=mi0, wz=0, Q_=None, al_=ap, be_=bp, sc_=sp):
        return fhb(ctx, nb_, n_, p_, H_, *sg(S_), Q_, 1, wz, mi, al_, be_, sc_, None, None, None)

    assert hess(nb_=0) == -2 and hess(n_=0) == -3 and hess(p_=0) == -4 and hess(A_=None) == -5
    assert hess() == 0
    if fam.signed:
        assert hess(S_=SL) == -7
        assert fam.cplx or hess(S_=None) == 0  # (a NULL signature is legal at the Float64 signed entries only)
    else:
        assert hess(tau_=None) == -6
    out = fam.hb_out_code
    for f in (host_, dev_):
        assert f(nb_=0) == -2 and f(n_=0) == -3 and f(p_=0) == -4 and f(A_=None) == -5 and f(o=b"X") == -6
        if fam.signed:
            assert f(S_=SL) == -7 and f(S_=SR, o=b"L") == 0 and f(S_=sarr([T, T, F]), o=b"L") == -7
        assert f(mi=0) == -9 and f(wz=1) == -10 and f(al_=None) == -11 and f(be_=None) == -11 and f(sc_=None) == -11
        assert f() == 0
        assert not fam.signed or fam.cplx or f(S_=None) == 0
    assert hb_(nb_=0) == -2 and hb_(n_=0) == -3 and hb_(p_=0) == -4 and hb_(H_=None) == -5 and hb_(wz=1) == -6
    assert not fam.signed or hb_(S_=SL) == -7
    assert hb_(mi=0) == -9 and hb_(al_=None) == out and hb_(be_=None) == out and hb_(sc_=None) == out
    if fam.signed:
        assert fhess(None, 1, n, p, ptrs, SR, None, None, None) == -1
    else:
        assert fhess(None, 1, n, p, ptrs, tp, None, None) == -1
    assert fhost(None, 1, n, p, ptrs, *sg(SR), b"R", 1, 0, mi0, None, ap, bp, sp, None, None, None, None) == -1
    assert fdev(None, 1, n, p, buf, *sg(SR), b"R", 1, 0, mi0, None, ap, bp, sp, None, None, None, None) == -1
    assert fhb(None, 1, n, p, ptrs, *sg(SR), None, 1, 0, mi0, ap, bp, sp, None, None, None) == -1


def case_abi_codes_gpu(eng, fam):
    """case_abi_codes with the device entry's problem in device memory"""
    import torch

    dA = torch.from_numpy(np.ascontiguousarray(pt.pack(problems(fam, fam.small)[0], fam.dtype))).cuda()
    torch.cuda.synchronize()
    case_abi_codes(eng, fam, devbuf=dA.data_ptr())


# ------------------------------------------------------------------------------------------------
# 12. groups
def case_groups(make_engine, fam):
    """A host entry whose batch does not fit the device at once works through it in groups (PSD_BATCH_GROUP lowers the
    group size): the same bits as in one group, problem by problem, and the same counters."""
    shape = fam.group
    nb, n, p = shape[:3]
    probs = problems(fam, shape)
    ref = make_engine({})
    eng = make_engine({"PSD_BATCH_GROUP": "4"})
    SL = fam.sargs(sig(shape, "L")) if fam.signed else ()
    SR = fam.sargs(sig(shape, "R")) if fam.signed else ()
    name = fam.prefix + "pschur_batch"
    if fam is D:  # one list of matrices through the loop (no Z), bit for bit
        for a, b in zip(ref.pschur_batch(probs, "L", wantZ=False), eng.pschur_batch(probs, "L", wantZ=False)):
            same_bits(a, b, p, "no Z")
    whole = getattr(ref, name)(probs, *SL, "L")
    parts = getattr(eng, name)(probs, *SL, "L")
    for q in range(nb):
        same_bits(whole[q], parts[q], p, q)
    for cnt in ("nsweeps", "nwindows", "ndefl1", "ndefl2", "niter") if fam.signed else ():
        assert getattr(whole[0].stats, cnt) == getattr(parts[0].stats, cnt), cnt
    Wb, Wp = [work(fam, A) for A in probs], [work(fam, A) for A in probs]
    ob, _ = getattr(ref, fam.prefix + "phessenberg_batch_")(Wb, *SR)
    op, _ = getattr(eng, fam.prefix + "phessenberg_batch_")(Wp, *SR)
    for q in range(nb):
        if fam.signed:  # (H, Q)
            assert all(np.array_equal(ob[q][0][j], op[q][0][j]) and np.array_equal(ob[q][1][j], op[q][1][j]) for j in range(p))
        else:           # (the packed H in place, tau)
            assert np.array_equal(ob[q][1], op[q][1]) and all(np.array_equal(Wb[q][j], Wp[q][j]) for j in range(p))
    Hb, Hp = [work(fam, o[0]) for o in ob], [work(fam, o[0]) for o in op]
    if fam is D:
        # the reduced factors through pschur_hess_batch_, bit for bit: H and Q both go up and come down (Q_j on entry: any
        # orthogonal matrices, the same for both engines)
        rng = np.random.default_rng(20)
        Qs = [[np.asfortranarray(np.linalg.qr(rng.standard_normal((n, n)))[0]) for _ in range(p)] for _ in range(nb)]
        infos_w, infos_p = [], []
        hb = ref.pschur_hess_batch_([(H[0], H[1:], Q) for H, Q in zip(Hb, [work(D, Q) for Q in Qs])], infos_out=infos_w)
        hp = eng.pschur_hess_batch_([(H[0], H[1:], Q) for H, Q in zip(Hp, [work(D, Q) for Q in Qs])], infos_out=infos_p)
        assert infos_w == infos_p == [0] * nb
        assert hb[0].stats.nsweeps > 0 and hp[0].stats.nsweeps > 0
    else:
        hb = getattr(ref, fam.prefix + "pschur_hess_batch_")(hess_args(Hb), *SR)
        hp = getattr(eng, fam.prefix + "pschur_hess_batch_")(hess_args(Hp), *SR)
    for q in range(nb):
        same_bits(hb[q], hp[q], p, ("hess", q))
        assert all(np.array_equal(Hb[q][j], Hp[q][j]) for j in range(p))  # (in place)


# ------------------------------------------------------------------------------------------------
# 13. the device-resident entry (GPU)
def case_device_resident(eng, fam):
    """One torch [nb, p, n, n] tensor through pschur_batch_dev: T, Z and the values equal the host entry's — bit for bit
    for the signed families, to 1e-12 relative for the unsigned ones (the same kernels on the same data; the entries
    differ in the copies alone)."""
    import torch

    shape = fam.small
    nb, n, p = shape[:3]
    probs = problems(fam, shape)
    batch = fam.method(eng, "pschur_batch")
    tdtype = torch.complex128 if fam.cplx else torch.float64
    for lr in ("R", "L"):
        Sa = fam.sargs(sig(shape, lr)) if fam.signed else ()
        host = batch(probs, *Sa, lr)
        dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in probs])).cuda()
        assert dA.dtype == tdtype
        keep = dA.clone()
        Tt, Zt, values, st = batch(dA, *Sa, lr)
        assert isinstance(Tt, torch.Tensor) and Tt.is_cuda and Zt.is_cuda and tuple(Tt.shape) == (nb, p, n, n)
        assert Tt.dtype == Zt.dtype == tdtype
        assert torch.equal(dA, keep)  # the input stays as it was
        Th, Zh = Tt.cpu().numpy(), Zt.cpu().numpy()
        for q in range(nb):
            if fam.signed:
                assert np.array_equal(values[q], host[q].values), (lr, q)
                for j in range(p):
                    assert np.array_equal(Th[q, j], host[q].Ts[j]), (lr, q, j)
                    assert np.array_equal(Zh[q, j], host[q].Z[j]), (lr, q, j)
                continue
            sc = max(np.linalg.norm(a, 2) for a in probs[q])
            assert np.abs(values[q] - host[q].values).max() <= 1e-12 * np.abs(host[q].values).max()
            for j in range(p):
                assert np.abs(Th[q, j] - host[q].Ts[j]).max() <= 1e-12 * sc, (lr, q, j)
                assert np.abs(Zh[q, j] - host[q].Z[j]).max() <= 1e-12, (lr, q, j)
            ps = psd_amd.PeriodicSchur([np.asfortranarray(Th[q, j]) for j in range(p)],
                                       [np.asfortranarray(Zh[q, j]) for j in range(p)], values[q], lr,
                                       p if lr == "L" else 1)
            fam.check_problem(shape, q, ps, lr)
    SR = sig(shape, "R") if fam.signed else None
    Tn, Zn, vn, _ = fam.no_z(eng, dA, SR)
    assert Zn is None
    for q in range(nb):
        fam.eigs(eng, probs[q], vn[q], SR, shape, q)
    with pytest.raises(psd_amd.DimensionMismatch):
        batch(dA[:, :, :, :5], *fam.sargs(SR))
    with pytest.raises(fam.wrong_exc, match=fam.wrong_match):
        batch(dA.to(torch.complex128) if fam.wrong is np.complex128 else dA.real.contiguous(), *fam.sargs(SR))
    if fam is DG:
        empty = torch.zeros((0, 2, 3, 3), dtype=torch.float64, device="cuda")
        infos = [7]
        Te, Ze, ve, ste = eng.dgpschur_batch_(empty, [True, False], infos_out=infos)
        assert tuple(Te.shape) == (0, 2, 3, 3) and ve.shape == (0, 3) and infos == [] and ste.niter == 0
