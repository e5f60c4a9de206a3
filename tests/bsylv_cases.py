"""Engine.psylvester_batch and Engine.subspacecond_batch (psd_?_psylv_batch[_dev], psd_?_subcond_batch[_dev],
csrc/psd_bsylv.h): periodic Sylvester solves on the off-diagonal block of many small periodic Schur forms, and the
periodic form of xTRSEN's S and SEP — the cases shared by the simulated tier (test_hostsim_psylvester_batch.py) and the
device tier (test_gpu_psylvester_batch.py).

The reference is the dense Kronecker matrix K of the operator S(X)_l = T11_l X_b(l) - X_a(l) T22_l on the p stacked
m x k blocks (user order, each column-major; (a, b) = (l + 1, l) for 'L', (l, l + 1) for 'R'): numpy.linalg.solve for X,
the exact ||K^-1||_1, and LAPACK's estimator xLACN2 restated in numpy on K^-1 (lacn2 below).  The inputs come from
bevec_cases.plain_form / zform and lbevec_cases.schur_form_si / as_right with the seeds fixed in PROBLEMS; every one has
kappa = max_l(||T11_l||_F + ||T22_l||_F) / sigma_min(K) <= 1e6, and the restated estimator is within a factor 3 of the
norm on it (test_reference_inputs checks both on the CPU).

Gates: relation ratios <= evec_cases.GATE; forward errors of X, s and sep <= n eps kappa, the forward bound of triangular
back-substitution (profiles/batch/README.md records what two CPU methods differ by on these seeds).  Bit-for-bit
comparisons are numpy.array_equal on X, s and sep (batch_common.same_bits compares decompositions, which these entries
do not return)."""
import numpy as np
import pytest

import bevec_cases as bc
import evec_cases as vc
import lbevec_cases as lc
import psd_amd
from batch_common import cached

EPS = 2.0 ** -52
GATE = vc.GATE
KAPPA_MAX = 1e6

# (n, p, m, rows of 2 x 2 blocks, schurindex (None: p), ComplexF64, seed): every one runs in 'L' and, as its
# flip-adjoint, in 'R'
PROBLEMS = [
    (2, 1, 1, (), None, False, 5),      # a single scalar system
    (2, 3, 1, (), None, False, 7),
    (5, 1, 2, (3,), None, False, 9),    # p = 1
    (6, 3, 2, (2,), None, False, 5),    # the split directly before a 2 x 2 block: the 1 x 2 block solve
    (6, 3, 2, (2,), 1, False, 7),       # the 2 x 2 blocks in the factor schurindex = 1
    (7, 4, 4, (0, 4), None, False, 9),  # the 2 x 1 and 2 x 2 . 2 x 2 block solves (pp = 4)
    (9, 5, 4, (1, 6), None, False, 17),  # an odd period
    (70, 2, 33, (10, 40), None, False, 23),  # crosses the 64-lane stride (the diagonals of diag70)
    (2, 1, 1, (), None, True, 5),
    (5, 1, 2, (), None, True, 9),
    (8, 2, 3, (), None, True, 9),       # ComplexF64, a full anti-diagonal
    (70, 2, 33, (), None, True, 17),
]
IDS = ["%s_n%d_p%d_m%d%s" % ("z" if pr[5] else "d", pr[0], pr[1], pr[2], "_si1" if pr[4] == 1 else "") for pr in PROBLEMS]


def diag70(p):
    """the diagonals of the Float64 problem of order 70: the products of the rows in three groups — 33 in [1, 1.5], 4 in
    [2.1, 2.4], 33 in [3, 3.5] — so that the split at 33 separates two groups in 'L' and in the flip-adjoint 'R' form
    (linspace(1, 2, 70) throughout, the default of plain_form, has kappa = 4e12 at this order)"""
    d = np.concatenate([np.linspace(1.0, 1.5, 33), np.linspace(2.1, 2.4, 4), np.linspace(3.0, 3.5, 33)])
    return [d ** (1.0 / p) for _ in range(p)]


def problem(k, lr):
    """(ps, As, m) of PROBLEMS[k] in orientation lr, read-only"""
    def make():
        n, p, m, pairs, si, cplx, seed = PROBLEMS[k]
        if cplx:
            pr = bc.zform(n, p, seed)
        elif si is None:
            pr = bc.plain_form(n, p, seed, pairs, diag=diag70(p) if n == 70 else None)
        else:
            pr = lc.schur_form_si(n, p, seed, pairs, si)
        if lr == "R":
            pr = lc.as_right(pr)
        ps, As = pr
        for a in list(ps.Ts) + list(ps.Z) + list(As):
            a.setflags(write=False)
        assert ps.orientation == lr and ps.Ts[ps.schurindex - 1][m, m - 1] == 0  # the split cuts no block
        return ps, As, m
    return cached(("bsylv", k, lr), make)


def ab(l, p, left):
    return ((l + 1) % p, l) if left else (l, (l + 1) % p)


def parts(ps, m):
    return [t[:m, :m] for t in ps.Ts], [t[:m, m:] for t in ps.Ts], [t[m:, m:] for t in ps.Ts]


def stack(Xs):
    return np.concatenate([np.asarray(x).reshape(-1, order="F") for x in Xs])


def unstack(v, p, m, k):
    return [v[l * m * k:(l + 1) * m * k].reshape((m, k), order="F") for l in range(p)]


def kron_matrix(ps, m):
    """block row l: kron(I_k, T11_l) in block column b(l), -kron(T22_l^T, I_m) in block column a(l)"""
    T11, _, T22 = parts(ps, m)
    p, n = len(ps.Ts), ps.Ts[0].shape[0]
    k, mk = n - m, m * (n - m)
    K = np.zeros((p * mk, p * mk), dtype=ps.Ts[0].dtype)
    for l in range(p):
        a, b = ab(l, p, ps.orientation == "L")
        K[l * mk:(l + 1) * mk, b * mk:(b + 1) * mk] += np.kron(np.eye(k), T11[l])
        K[l * mk:(l + 1) * mk, a * mk:(a + 1) * mk] -= np.kron(T22[l].T, np.eye(m))
    return K


def lacn2(Kinv, cplx):
    """xLACN2 on K^-1 (kase 1: K^-1 x, kase 2: K^-H x): (est, solves, iterations)"""
    N = Kinv.shape[0]
    KinvH = Kinv.conj().T
    absx = np.abs

    def sgn(x):
        if cplx:
            a = absx(x)
            return np.where(a > np.finfo(float).tiny, x / np.where(a > 0, a, 1), 1.0)
        return np.where(x > 0, 1.0, -1.0)

    x = Kinv @ np.full(N, 1.0 / N, dtype=Kinv.dtype)
    solves = 1
    if N == 1:
        return absx(x[0]), solves, 0
    est = absx(x).sum()
    x = sgn(x)
    isgn = x.copy()
    x = KinvH @ x
    solves += 1
    j = int(np.argmax(absx(x)))
    it = 2
    while True:
        x = np.zeros(N, dtype=Kinv.dtype)
        x[j] = 1
        x = Kinv @ x
        solves += 1
        estold, est = est, absx(x).sum()
        if not cplx and np.array_equal(sgn(x), isgn):
            break
        if est <= estold:
            break
        x = sgn(x)
        isgn = x.copy()
        x = KinvH @ x
        solves += 1
        jlast, j = j, int(np.argmax(absx(x)))
        if (absx(x[jlast]) if cplx else x[jlast]) != absx(x[j]) and it < 5:
            it += 1
            continue
        break
    x = np.array([(-1.0) ** i * (1.0 + i / (N - 1)) for i in range(N)], dtype=Kinv.dtype)
    x = Kinv @ x
    solves += 1
    return max(est, 2.0 * (absx(x).sum() / (3 * N))), solves, it


def kron_cached(k, lr):
    return cached(("bsylv-kron", k, lr), lambda: kron_matrix(*problem(k, lr)[::2]))


def reference(k, lr):
    """K, K^-1, kappa, X of C = -T12, s, ||K^-1||_1 and the restated estimator of problem (k, lr): computed once"""
    def make():
        ps, As, m = problem(k, lr)
        p, n = len(ps.Ts), ps.Ts[0].shape[0]
        T11, T12, T22 = parts(ps, m)
        K = kron_cached(k, lr)
        Kinv = np.linalg.inv(K)
        smin = 1.0 / np.linalg.norm(Kinv, 2)
        kappa = max(np.linalg.norm(a) + np.linalg.norm(b) for a, b in zip(T11, T22)) / smin
        X = unstack(np.linalg.solve(K, stack([-c for c in T12])), p, m, n - m)
        s = np.array([1.0 / np.sqrt(1.0 + np.linalg.norm(x) ** 2) for x in X])
        est, solves, it = lacn2(Kinv, np.iscomplexobj(K))
        return dict(K=K, Kinv=Kinv, kappa=kappa, X=X, s=s, norm1=np.linalg.norm(Kinv, 1), est=est, solves=solves, it=it)
    return cached(("bsylv-ref", k, lr), make)


def residual_ratio(ps, m, Xs, Cs, Kop=None):
    """max_l ||S(X)_l - C_l||_F / ((||T11_l||_F + ||T22_l||_F) max(||X_a||_F, ||X_b||_F) + ||C_l||_F); Kop: the matrix
    of another operator on the stacked blocks (K^H), whose block row l meets the blocks a(l), b(l) of the adjoint"""
    T11, _, T22 = parts(ps, m)
    p, n = len(ps.Ts), ps.Ts[0].shape[0]
    left = ps.orientation == "L"
    if Kop is None:
        R = [T11[l] @ Xs[ab(l, p, left)[1]] - Xs[ab(l, p, left)[0]] @ T22[l] for l in range(p)]
        nb = [(ab(l, p, left), l, l) for l in range(p)]
    else:
        R = unstack(Kop @ stack(Xs), p, m, n - m)
        # S^H(Y)_j = T11_l^H Y_l - Y_l' T22_l'^H with b(l) = j, a(l') = j
        nb = []
        for j in range(p):
            l = [x for x in range(p) if ab(x, p, left)[1] == j][0]
            l2 = [x for x in range(p) if ab(x, p, left)[0] == j][0]
            nb.append(((l, l2), l, l2))
    worst = 0.0
    for j in range(p):
        (u, v), f1, f2 = nb[j]
        den = ((np.linalg.norm(T11[f1]) + np.linalg.norm(T22[f2])) * max(np.linalg.norm(Xs[u]), np.linalg.norm(Xs[v]))
               + np.linalg.norm(Cs[j]))
        worst = max(worst, np.linalg.norm(R[j] - Cs[j]) / den)
    return worst


def random_blocks(ps, m, seed):
    p, n = len(ps.Ts), ps.Ts[0].shape[0]
    rs = np.random.RandomState(seed)
    cplx = np.iscomplexobj(ps.Ts[0])
    return [np.asfortranarray(rs.randn(m, n - m) + (1j * rs.randn(m, n - m) if cplx else 0)) for _ in range(p)]


def untouched(ps, keep):
    return all(np.array_equal(a, b) for a, b in zip(list(ps.Ts) + list(ps.Z), keep))


# ------------------------------------------------------------------------------------------------
# 0. the inputs (CPU only): kappa, the estimator's factor 3, and what two CPU methods differ by
def reference_figures(k, lr):
    """(kappa, est / ||K^-1||_1, the error of the dense LU solve against lstsq in units of n eps kappa)"""
    ps, As, m = problem(k, lr)
    ref = reference(k, lr)
    n = ps.Ts[0].shape[0]
    _, T12, _ = parts(ps, m)
    x1 = stack(ref["X"])
    x2 = np.linalg.lstsq(ref["K"], stack([-c for c in T12]), rcond=None)[0]
    return ref["kappa"], ref["est"] / ref["norm1"], np.linalg.norm(x1 - x2) / np.linalg.norm(x1) / (n * EPS * ref["kappa"])


def case_reference_inputs(k, lr):
    ref = reference(k, lr)
    assert ref["kappa"] <= KAPPA_MAX, ref["kappa"]
    assert 1.0 / 3.0 <= ref["est"] / ref["norm1"] <= 1.0 + 1e-12, ref["est"] / ref["norm1"]
    assert ref["solves"] <= 11
    if ref["K"].shape[0] <= 1000:  # (order 70: 0.002 at most, profiles/batch/README.md; lstsq takes seconds there)
        pair = reference_figures(k, lr)[2]
        assert pair <= 0.2, pair  # the reference pair stays a factor 5 below the gate


# ------------------------------------------------------------------------------------------------
# 1. solve residual
def case_residual(eng, k, lr):
    ps, As, m = problem(k, lr)
    p, n = len(ps.Ts), ps.Ts[0].shape[0]
    keep = [a.copy() for a in list(ps.Ts) + list(ps.Z)]
    _, T12, T22 = parts(ps, m)
    X = eng.psylvester_batch([ps], m)[0]
    assert len(X) == p and all(x.shape == (m, n - m) for x in X)
    r = residual_ratio(ps, m, X, [-c for c in T12])
    print("residual default", IDS[k], lr, r)
    assert r <= GATE, r
    # the block-diagonalisation: A_l Y_b = Y_a T22_l with Y_l = Z_l [X_l; I] (S(X) = -T12 is T_l [X_b; I] = [X_a; I] T22_l)
    Y = [ps.Z[l] @ np.vstack([X[l], np.eye(n - m)]) for l in range(p)]
    worst = 0.0
    for l in range(p):
        a, b = ab(l, p, lr == "L")
        worst = max(worst, np.linalg.norm(As[l] @ Y[b] - Y[a] @ T22[l])
                    / (np.linalg.norm(As[l]) * max(np.linalg.norm(Y[a]), np.linalg.norm(Y[b]))))
    print("block diagonalisation", IDS[k], lr, worst)
    assert worst <= GATE, worst
    Cs = random_blocks(ps, m, 100 + k)
    keepC = [c.copy() for c in Cs]
    X = eng.psylvester_batch([ps], m, C=[Cs])[0]
    r = residual_ratio(ps, m, X, Cs)
    print("residual random", IDS[k], lr, r)
    assert r <= GATE, r
    assert untouched(ps, keep) and all(np.array_equal(a, b) for a, b in zip(Cs, keepC))


# ------------------------------------------------------------------------------------------------
# 2. transposed solve
def case_transposed(eng, k, lr):
    ps, As, m = problem(k, lr)
    p, n = len(ps.Ts), ps.Ts[0].shape[0]
    K = kron_cached(k, lr)
    KH = K.conj().T
    Cs = random_blocks(ps, m, 200 + k)
    Y = eng.psylvester_batch([ps], m, C=[Cs], trans=True)[0]
    r = residual_ratio(ps, m, Y, Cs, Kop=KH)
    print("residual transposed", IDS[k], lr, r)
    assert r <= GATE, r
    # <Y, S X> = <S^H Y, X>: S X from numpy, Y recovered by the device from S^H Y
    X0, Y0 = random_blocks(ps, m, 300 + k), random_blocks(ps, m, 400 + k)
    SX = K @ stack(X0)
    SHY = unstack(KH @ stack(Y0), p, m, n - m)
    Y1 = eng.psylvester_batch([ps], m, C=[SHY], trans=True)[0]
    lhs, rhs = np.vdot(stack(Y1), SX), np.vdot(stack(SHY), stack(X0))
    gap = abs(lhs - rhs) / (np.linalg.norm(stack(X0)) * np.linalg.norm(stack(Y1)) * np.linalg.norm(K))
    print("adjoint identity", IDS[k], lr, gap)
    assert gap <= GATE, gap


# ------------------------------------------------------------------------------------------------
# 3, 4. s, X and sep against the reference
def case_reference(eng, k, lr):
    ps, As, m = problem(k, lr)
    n = ps.Ts[0].shape[0]
    ref = reference(k, lr)
    bound = n * EPS * ref["kappa"]
    s, sep, X = eng.subspacecond_batch([ps], m, want_x=True)
    st = eng.subspacecond_batch_stats
    es = np.abs(s[0] - ref["s"]) / ref["s"]
    ex = np.linalg.norm(stack(X[0]) - stack(ref["X"])) / np.linalg.norm(stack(ref["X"]))
    print("forward errors", IDS[k], lr, "kappa %.3e s %.3e X %.3e bound %.3e" % (ref["kappa"], es.max(), ex, bound))
    assert np.all(es <= bound), (es.max(), bound)
    assert ex <= bound, (ex, bound)
    est = 1.0 / sep[0]
    print("sep", IDS[k], lr, "est / norm %.4f solves %d (numpy %d) iterations %d (numpy %d)"
          % (est / ref["norm1"], st.nsolve - 1, ref["solves"], st.nest_iter, ref["it"]))
    assert est <= ref["norm1"] * (1.0 + bound), (est, ref["norm1"])
    assert est >= ref["norm1"] / 3.0, (est, ref["norm1"])
    if st.nsolve - 1 == ref["solves"] and st.nest_iter == ref["it"]:  # the same path
        assert abs(est - ref["est"]) <= bound * ref["est"], (est, ref["est"])


# ------------------------------------------------------------------------------------------------
# 5. p = 1 against LAPACK
def case_trsen(eng, k, lr):
    import scipy.linalg.lapack as la

    ps, As, m = problem(k, lr)
    n = ps.Ts[0].shape[0]
    assert len(ps.Ts) == 1
    cplx = np.iscomplexobj(ps.Ts[0])
    sel = np.zeros(n, dtype=np.int32)
    sel[:m] = 1
    mk = max(1, m * (n - m))
    work = dict(lwork=2 * mk) if cplx else dict(lwork=2 * mk, liwork=mk)
    out = (la.ztrsen if cplx else la.dtrsen)(sel, np.array(ps.Ts[0], order="F"), np.eye(n, dtype=ps.Ts[0].dtype, order="F"),
                                             job="B", wantq=0, **work)
    S0, SEP0, info = out[-3], out[-2], out[-1]
    assert info == 0 and out[-4] == m
    s, sep = eng.subspacecond_batch([ps], m)
    bound = n * EPS * reference(k, lr)["kappa"]
    print("trsen", IDS[k], lr, s[0, 0], S0, sep[0], SEP0)
    assert abs(s[0, 0] - S0) <= bound * S0 and abs(sep[0] - SEP0) <= bound * SEP0


# ------------------------------------------------------------------------------------------------
# 6. mixed batch: per-problem m, the trivial splits among them
def mixed_batch(cplx):
    """order 7, period 3: five problems, m = 0 and m = n among them (they take part in no launch)"""
    if cplx:
        probs = bc.mixed_problems(bc.Z)
        return [ps for ps, _ in probs], [3, 0, 7, 4, 1]
    probs = bc.mixed_problems()  # (2 x 2 blocks at rows bc.D.mixed_pairs[q])
    pss = [ps for ps, _ in probs]
    ms = [3, 0, 7, 4, 1]
    for ps, m in zip(pss, ms):
        assert m in (0, 7) or ps.Ts[ps.schurindex - 1][m, m - 1] == 0
    return pss, ms


def case_mixed(eng, cplx):
    pss, ms = mixed_batch(cplx)
    n, p = 7, 3
    s, sep, X = eng.subspacecond_batch(pss, ms, want_x=True)
    st = eng.subspacecond_batch_stats
    assert s.shape == (5, p) and sep.shape == (5,) and st.nb == 5 and st.ngroups == 1 and st.nsingular == 0
    Xs = eng.psylvester_batch(pss, ms)
    for q, (ps, m) in enumerate(zip(pss, ms)):
        assert all(x.shape == (m, n - m) for x in X[q]) and len(X[q]) == p
        if m in (0, n):
            assert np.all(s[q] == 1.0) and sep[q] == np.inf
        else:
            assert np.all((s[q] > 0) & (s[q] < 1)) and 0 < sep[q] < np.inf
        s1, sep1, X1 = eng.subspacecond_batch([ps], m, want_x=True)  # alone
        assert np.array_equal(s1[0], s[q]) and sep1[0] == sep[q]
        assert all(np.array_equal(a, b) for a, b in zip(X1[0], X[q]))
        assert all(np.array_equal(a, b) for a, b in zip(Xs[q], X[q]))
    # the trivial splits alone: no launch at all
    s, sep = eng.subspacecond_batch([pss[1], pss[2]], [0, n])
    st = eng.subspacecond_batch_stats
    assert np.all(s == 1.0) and np.all(sep == np.inf) and st.nsolve == 0 and st.nnorms == 0 and st.nest_steps == 0
    # one common m as an int
    s2, sep2 = eng.subspacecond_batch([pss[0], pss[0]], 3)
    s1, sep1 = eng.subspacecond_batch([pss[0]], [3])
    assert np.array_equal(s2[0], s1[0]) and np.array_equal(s2[1], s1[0]) and sep2[0] == sep2[1] == sep1[0]


# ------------------------------------------------------------------------------------------------
# 7. batch independence, bit for bit
def case_independence(eng, eng_groups, cplx):
    pss, ms = mixed_batch(cplx)
    big = [pss[q % 5] for q in range(11)]
    bm = [ms[q % 5] for q in range(11)]
    s, sep, X = eng.subspacecond_batch(big, bm, want_x=True)
    assert eng.subspacecond_batch_stats.ngroups == 1

    def same(a, b, qa, qb):
        assert np.array_equal(a[0][qa], b[0][qb]) and a[1][qa] == b[1][qb], (qa, qb)
        assert all(np.array_equal(x, y) for x, y in zip(a[2][qa], b[2][qb])), (qa, qb)

    for q in range(5, 11):  # the same problem at another place
        same((s, sep, X), (s, sep, X), q, q % 5)
    parts_ = eng_groups.subspacecond_batch(big, bm, want_x=True)
    assert eng_groups.subspacecond_batch_stats.ngroups == 4
    perm = [7, 2, 9, 0, 4, 10, 1, 6, 3, 8, 5]
    turned = eng.subspacecond_batch([big[q] for q in perm], [bm[q] for q in perm], want_x=True)
    for q in range(11):
        same(parts_, (s, sep, X), q, q)
        same(turned, (s, sep, X), q, perm[q])
    Xa = eng.psylvester_batch(big, bm, trans=True)
    Xb = eng_groups.psylvester_batch(big, bm, trans=True)
    assert eng_groups.psylvester_batch_stats.ngroups == 4
    Xc = eng.psylvester_batch([big[q] for q in perm], [bm[q] for q in perm], trans=True)
    for q in range(11):
        assert all(np.array_equal(x, y) for x, y in zip(Xa[q], Xb[q]))
        assert all(np.array_equal(x, y) for x, y in zip(Xa[perm[q]], Xc[q]))


# ------------------------------------------------------------------------------------------------
# 8. a singular problem
def singular_batch(cplx):
    """problem 1 of three: the diagonal entry at row 1 (in T11, m = 3) repeated exactly at row 4 (in T22), factor by
    factor"""
    def make():
        probs = bc.mixed_problems(bc.Z) if cplx else [bc.plain_form(7, 3, s) for s in bc.D.seeds[:3]]
        pss = [probs[q][0] for q in range(3)]
        Ts = [t.copy(order="F") for t in pss[1].Ts]
        for t in Ts:
            t[4, 4] = t[1, 1]
        pss[1] = psd_amd.PeriodicSchur(Ts, pss[1].Z, np.array(pss[1].values), pss[1].orientation, pss[1].schurindex)
        return pss
    return cached(("bsylv-singular", cplx), make)


def case_singular(eng, cplx):
    pss = singular_batch(cplx)
    m, n, p = 3, 7, 3
    infos = [7, 7, 7]
    s, sep, X = eng.subspacecond_batch(pss, m, want_x=True, infos_out=infos)
    assert infos == [0, 3000, 0]  # PSD_INFO_SINGULAR
    assert eng.subspacecond_batch_stats.nsingular == 1
    assert np.all(s[1] == 0.0) and sep[1] == 0.0 and all(np.isnan(x).all() for x in X[1])
    for q in (0, 2):
        s1, sep1, X1 = eng.subspacecond_batch([pss[q]], m, want_x=True)
        assert np.array_equal(s1[0], s[q]) and sep1[0] == sep[q] and np.all(s[q] > 0) and sep[q] > 0
        assert all(np.array_equal(a, b) for a, b in zip(X1[0], X[q]))
    with pytest.raises(psd_amd.SingularException):
        eng.subspacecond_batch(pss, m)
    infos = [7, 7, 7]
    Xs = eng.psylvester_batch(pss, m, infos_out=infos)
    assert infos[0] == 0 and infos[1] == 3000 and infos[2] == 0
    assert all(np.isnan(x).all() for x in Xs[1])
    assert all(np.array_equal(a, b) for q in (0, 2) for a, b in zip(Xs[q], X[q]))
    with pytest.raises(psd_amd.SingularException):
        eng.psylvester_batch(pss, m)


# ------------------------------------------------------------------------------------------------
# 9. argument errors and the cap
def case_errors(eng, make_engine):
    probs = bc.mixed_problems()
    pss = [ps for ps, _ in probs]
    zss = [ps for ps, _ in bc.mixed_problems(bc.Z)]
    n, p = 7, 3
    pair = bc.D.mixed_pairs[2][0]  # a 2 x 2 block of problem 2 at rows pair, pair + 1
    assert pss[2].Ts[p - 1][pair + 1, pair] != 0
    for call in (eng.subspacecond_batch, eng.psylvester_batch):
        with pytest.raises(ValueError, match="argument 8"):  # a split inside a 2 x 2 block
            call([pss[0], pss[2]], [3, pair + 1])
        for bad in (-1, n + 1):
            with pytest.raises(ValueError, match="argument 8"):
                call(pss, bad)
        with pytest.raises(psd_amd.DimensionMismatch):
            call(pss, [3, 3])  # not [nb]
        with pytest.raises(psd_amd.DimensionMismatch):
            call(pss, 2.5)
        with pytest.raises(TypeError):  # mixed dtypes
            call([pss[0], zss[0]], 3)
        with pytest.raises(TypeError):
            call([zss[0], pss[0]], 3)
        g = psd_amd.GeneralizedPeriodicSchur([True, False, True], pss[0].Ts, pss[0].Z, np.array(pss[0].values), np.ones(n),
                                             np.zeros(n, dtype=np.int32), "L", p)
        with pytest.raises(psd_amd.NotImplementedPSD):
            call([pss[0], g], 3)
        with pytest.raises(psd_amd.DimensionMismatch):  # another order in the batch
            call([pss[0], bc.plain_form(6, 3, 5)[0]], 3)
    with pytest.raises(psd_amd.DimensionMismatch):  # right-hand sides of the wrong shape
        eng.psylvester_batch([pss[0]], 3, C=[[np.zeros((3, 3))] * p])
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.psylvester_batch([pss[0]], 3, C=[[np.zeros((3, 4))] * (p - 1)])
    # an empty batch
    assert eng.psylvester_batch([], 3) == []
    s, sep = eng.subspacecond_batch([], 3)
    assert s.shape[0] == 0 and sep.shape == (0,)
    # the cap: there is no path above it
    low = make_engine({"PSD_BSYL_NMAX": "6"})
    with pytest.raises(psd_amd.NotImplementedPSD):
        low.subspacecond_batch(pss, 3)
    with pytest.raises(psd_amd.NotImplementedPSD):
        low.psylvester_batch(zss, 3)
    s6, _ = low.subspacecond_batch([bc.plain_form(6, 3, 5)[0]], 3)
    assert np.all(s6 > 0)
    sharded = make_engine({})
    sharded.set_shard(0, 2)
    with pytest.raises(psd_amd.NotImplementedPSD):
        sharded.subspacecond_batch(pss, 3)


# ------------------------------------------------------------------------------------------------
# 10. launch count
def case_launch_count(eng, cplx):
    pss, ms = mixed_batch(cplx)
    counts = []
    for batch, m in (([pss[0]], 3), ([pss[0]] * 9, 3), (pss + pss, ms + ms)):
        eng.subspacecond_batch(batch, m)
        st = eng.subspacecond_batch_stats
        assert st.ngroups == 1 and st.nnorms == 1 and 2 <= st.nsolve <= 1 + 12 and st.nest_iter <= 5
        assert st.nest_steps == st.nsolve  # (a step behind every solve of the estimator, and the one that starts it)
        counts.append((st.nsolve, st.nnorms, st.nest_steps, st.nest_iter))
    assert counts[0] == counts[1]  # independent of nb
    eng.psylvester_batch(pss, ms)
    st = eng.psylvester_batch_stats
    assert (st.nsolve, st.nnorms, st.nest_steps, st.ngroups) == (1, 0, 0, 1)


# ------------------------------------------------------------------------------------------------
# 11. the device entry behind pschur_batch_ and ordschur_batch_ (GPU tier)
def case_device(eng, lr, cplx):
    import torch

    import psdtest as pt

    n, p, nb, m = 12, 3, 4, 5
    rs = np.random.RandomState(77)
    facs = [pt.bench_factors(n, p, seed=91 + q) for q in range(nb)]
    if cplx:
        facs = [[np.asfortranarray(a + 1j * rs.randn(n, n) / np.sqrt(n)) for a in A] for A in facs]
    dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in facs])).cuda()
    T, Z, values, _ = (eng.zpschur_batch_ if cplx else eng.pschur_batch_)(dA, lr)
    si = p if lr == "L" else 1
    # the m eigenvalues of largest modulus to the top, conjugate pairs kept whole
    select = np.zeros((nb, n), dtype=bool)
    for q in range(nb):
        order = np.argsort(-np.abs(values[q]), kind="stable")
        select[q, order[:m]] = True
        if not cplx and abs(abs(values[q][order[m - 1]]) - abs(values[q][order[m]])) < 1e-12 * abs(values[q][order[m]]):
            select[q, order[m]] = True  # (the partner of a pair)
    ms = select.sum(axis=1).astype(np.int32)
    T, Z, values, _ = (eng.zordschur_batch_ if cplx else eng.ordschur_batch_)(T, Z, select, lr=lr, schurindex=si)
    keep = T.clone()
    s, sep, X = eng.subspacecond_batch(T, ms, want_x=True, lr=lr, schurindex=si)
    assert torch.equal(T, keep) and X.is_cuda
    Th, Zh = T.cpu().numpy(), Z.cpu().numpy()
    pss = [psd_amd.PeriodicSchur([np.asfortranarray(Th[q, l]) for l in range(p)],
                                 [np.asfortranarray(Zh[q, l]) for l in range(p)], values[q], lr, si) for q in range(nb)]
    s0, sep0, X0 = eng.subspacecond_batch(pss, ms, want_x=True)
    assert np.array_equal(s, s0) and np.array_equal(sep, sep0) and np.all(s > 0) and np.all(sep > 0)
    Xh = X.cpu().numpy()
    for q in range(nb):
        mq, kq = int(ms[q]), n - int(ms[q])
        got = Xh[q] if Xh.ndim == 4 else [Xh[q, l, :mq * kq].reshape((mq, kq), order="F") for l in range(p)]
        assert all(np.array_equal(got[l], X0[q][l]) for l in range(p))
        # the complementary subspace of the ORIGINAL factors
        Y = [pss[q].Z[l] @ np.vstack([X0[q][l], np.eye(kq)]) for l in range(p)]
        for l in range(p):
            a, b = ab(l, p, lr == "L")
            r = (np.linalg.norm(facs[q][l] @ Y[b] - Y[a] @ pss[q].Ts[l][mq:, mq:])
                 / (np.linalg.norm(facs[q][l]) * max(np.linalg.norm(Y[a]), np.linalg.norm(Y[b]))))
            assert r <= GATE, (q, l, r)
    Xd = eng.psylvester_batch(T, ms, lr=lr, schurindex=si)
    assert torch.equal(Xd, X) and torch.equal(T, keep)
    Cs = [random_blocks(pss[q], int(ms[q]), 500 + q) for q in range(nb)]
    xb = int(max(int(mq) * (n - int(mq)) for mq in ms))
    flat = np.zeros((nb, p, xb), dtype=Cs[0][0].dtype)  # the flat column-major blocks of the device form
    for q in range(nb):
        for l in range(p):
            flat[q, l, :Cs[q][l].size] = stack([Cs[q][l]])
    Cd = torch.from_numpy(flat).cuda()
    Yd = eng.psylvester_batch(T, ms, C=Cd, trans=True, lr=lr, schurindex=si)
    Y0 = eng.psylvester_batch(pss, ms, C=Cs, trans=True)
    Yh = Yd.cpu().numpy()
    for q in range(nb):
        mq, kq = int(ms[q]), n - int(ms[q])
        got = Yh[q] if Yh.ndim == 4 else [Yh[q, l, :mq * kq].reshape((mq, kq), order="F") for l in range(p)]
        assert all(np.array_equal(got[l], Y0[q][l]) for l in range(p))


def case_empty_device(eng):
    import torch

    T = torch.zeros((0, 2, 3, 3), dtype=torch.float64, device="cuda")
    s, sep = eng.subspacecond_batch(T, 1)
    assert s.shape == (0, 2) and sep.shape == (0,)
    X = eng.psylvester_batch(T, 1)
    assert X.shape[0] == 0 and X.is_cuda
    with pytest.raises(psd_amd.DimensionMismatch):  # wrong tensor shapes
        eng.subspacecond_batch(torch.zeros((2, 3, 3), dtype=torch.float64, device="cuda"), 1)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.psylvester_batch(torch.zeros((1, 2, 3, 4), dtype=torch.float64, device="cuda"), 1)
    with pytest.raises(TypeError):
        eng.subspacecond_batch(torch.zeros((1, 2, 3, 3), dtype=torch.float32, device="cuda"), 1)
