"""geigvecs(P, select; shifted) — eigenvectors of signed and singular periodic products (psd_?_geigvecs): the cases
shared by the simulated tier (test_hostsim_geigvecs.py) and the device tier (test_gpu_geigvecs.py), and an independent
numpy prototype (the cyclic block system of each column, solved densely) as their host reference."""
import numpy as np
import pytest

import evec_cases as vc
import psd_amd

GATE = vc.GATE


def signed_form(n, p, S, lr="L", diag=None, seed=0, cplx=False, pairs=(), si=None):
    """a signed periodic Schur form built directly: T_l upper triangular with diagonals diag[l] (default: moderate
    random), T_si with 2x2 blocks at the rows in `pairs`, random unitary Z_l; A_l = Z_{l+1} T_l Z_l^H if S[l] else
    Z_l T_l Z_{l+1}^H for 'L', the mirror for 'R'.  Returns (GeneralizedPeriodicSchur, As)."""
    rs = np.random.RandomState(seed)
    dt = np.complex128 if cplx else np.float64
    si = p if si is None else si
    if diag is None:
        diag = [(0.6 + rs.rand(n)) * np.where(rs.rand(n) < 0.3, -1, 1) for _ in range(p)]
    Ts = []
    for l in range(p):
        t = 0.2 * np.triu(rs.randn(n, n) + (1j * rs.randn(n, n) if cplx else 0), 1).astype(dt)
        t[np.arange(n), np.arange(n)] = diag[l]
        Ts.append(t)
    for i in pairs:  # (the other factors' blocks there: positive multiples of I, so the product keeps the pair)
        T = Ts[si - 1]
        T[i, i + 1], T[i + 1, i], T[i + 1, i + 1] = 0.8, -0.6, T[i, i]
        for l in range(p):
            if l != si - 1:
                Ts[l][i, i] = Ts[l][i + 1, i + 1] = abs(Ts[l][i, i]) + 0.5
                Ts[l][i, i + 1] = 0.0
    Ts = [np.asfortranarray(t) for t in Ts]
    Zs = [np.asfortranarray(np.linalg.qr(rs.randn(n, n) + (1j * rs.randn(n, n) if cplx else 0))[0]) for _ in range(p)]
    left = lr == "L"
    As = []
    for l in range(p):
        ln = (l + 1) % p
        fwd = bool(S[l]) == left
        As.append(Zs[ln] @ Ts[l] @ Zs[l].conj().T if fwd else Zs[l] @ Ts[l] @ Zs[ln].conj().T)
    with np.errstate(divide="ignore", invalid="ignore"):
        vals = np.ones(n, dtype=complex)
        for l in range(p):
            d = np.diag(Ts[l]).astype(complex)
            vals = vals * (d if S[l] else 1.0 / d)
    for i in pairs:  # the signed product of the 2x2 blocks, in the orientation's order
        M = np.eye(2)
        for l in range(p):
            B = Ts[l][i:i + 2, i:i + 2]
            F = B if S[l] else np.linalg.inv(B)
            M = F @ M if left else M @ F
        ev = np.linalg.eigvals(M)
        vals[i], vals[i + 1] = ev[np.argmax(ev.imag)], ev[np.argmin(ev.imag)]
    alpha = np.where(np.isfinite(vals), vals, 1.0).astype(np.complex128)
    beta = np.where(np.isfinite(vals), 1.0, 0.0)
    P = psd_amd.GeneralizedPeriodicSchur(list(S), Ts, Zs, alpha, beta, np.zeros(n, dtype=np.int32), lr, si)
    return P, As


def _sgn(P):
    return list(P.S) if isinstance(P, psd_amd.GeneralizedPeriodicSchur) else [True] * len(P.Ts)


def _pairs_of(P):
    n = P.Ts[0].shape[0]
    T = P.Ts[P.schurindex - 1]
    bsz = [1] * n
    if not np.iscomplexobj(T):
        for i in range(n - 1):
            if bsz[i] == 1 and T[i + 1, i] != 0:
                bsz[i], bsz[i + 1] = 2, 0
    return bsz


def _columns(P, select):
    bsz = _pairs_of(P)
    cols, i = [], 0
    while i < len(bsz):
        b = bsz[i]
        if select[i] or (b == 2 and select[i + 1]):
            cols.append((i, b))
        i += b
    return cols


def pair_scalars(P, k):
    """the scalars of the first column of the pair at rows k, k+1"""
    p, si, S = len(P.Ts), P.schurindex - 1, _sgn(P)
    lam = P.values[k]
    a = np.array([np.sqrt(abs(np.linalg.det(P.Ts[l][k:k + 2, k:k + 2]))) for l in range(p)], dtype=complex)
    a[si] *= np.exp(1j * np.angle(lam) * (1 if S[si] else -1))  # (an inverted quasi-triangular factor: the conjugate)
    return a


def forward(P, l):
    """True: factor l's relation in Schur coordinates is T_l x_l = a_l x_{l+1}; False: T_l x_{l+1} = a_l x_l"""
    return bool(_sgn(P)[l]) == (P.orientation == "L")


def prototype(P, select):
    """independent numpy reference: per column, the homogeneous cyclic block system of the relations in Schur
    coordinates on rows 0 .. k+m-1 (unknowns x_1 .. x_p there), its null vector by SVD, V_l = Z_l x_l, normalised by
    the eigvecs rule.  Returns (Vs, a)."""
    Ts, Zs, p, n = P.Ts, P.Z, len(P.Ts), P.Ts[0].shape[0]
    out, scal = [], []
    for k, m in _columns(P, select):
        a = pair_scalars(P, k) if m == 2 else np.array([Ts[l][k, k] for l in range(p)], dtype=complex)
        r = k + m
        M = np.zeros((p * r, p * r), dtype=complex)
        for l in range(p):
            ln = (l + 1) % p
            T = np.array(Ts[l][:r, :r], dtype=complex)
            if forward(P, l):  # T x_l = a x_{l+1}
                M[l * r:(l + 1) * r, l * r:(l + 1) * r] += T
                M[l * r:(l + 1) * r, ln * r:(ln + 1) * r] -= a[l] * np.eye(r)
            else:  # T x_{l+1} = a x_l
                M[l * r:(l + 1) * r, ln * r:(ln + 1) * r] += T
                M[l * r:(l + 1) * r, l * r:(l + 1) * r] -= a[l] * np.eye(r)
        x = np.linalg.svd(M)[2][-1].conj()
        V = [Zs[l][:, :r] @ x[l * r:(l + 1) * r] for l in range(p)]
        am = np.argmax(np.abs(V[0]))
        s = np.conj(V[0][am]) / abs(V[0][am]) / np.linalg.norm(V[0])
        out.append([s * v for v in V])
        scal.append(a)
        if m == 2:
            out.append([np.conj(s * v) for v in V])
            scal.append(np.conj(a))
    return [np.stack([c[l] for c in out], axis=1) for l in range(p)], np.stack(scal, axis=1)


def relation_ratio(As, S, lr, Vs, a):
    """max over l and columns of ||lhs - rhs|| / (||A_l||_F ||v|| + |a_l| ||v'||) for the relations of the table"""
    p = len(As)
    worst = 0.0
    for j in range(Vs[0].shape[1]):
        for l in range(p):
            x, y = Vs[l][:, j], Vs[(l + 1) % p][:, j]
            if bool(S[l]) != (lr == "L"):
                x, y = y, x  # A_l v_{l+1} = a_l v_l
            den = np.linalg.norm(As[l]) * np.linalg.norm(x) + abs(a[l, j]) * np.linalg.norm(y)
            worst = max(worst, np.linalg.norm(As[l] @ x - a[l, j] * y) / den)
    return worst


def check(eng, P, As, select, proto=True, dense=True):
    """geigvecs against the contract: relations, scalars, normalisation, shifted=False, the prototype, and (n <= 12)
    V_1 an eigenvector of the dense signed product.  Returns (Vs, a)."""
    S, p, n = _sgn(P), len(P.Ts), P.Ts[0].shape[0]
    keep = [t.copy() for t in P.Ts]
    Vs, a = eng.geigvecs(P, select)
    assert all(np.array_equal(x, y) for x, y in zip(keep, P.Ts))
    lams = vc.order_values(P, select)
    assert len(Vs) == p and Vs[0].shape == (n, len(lams)) and a.shape == (p, len(lams))
    assert all(np.isfinite(V).all() for V in Vs)
    r = relation_ratio(As, S, P.orientation, Vs, a)
    assert r <= GATE, r
    with np.errstate(divide="ignore", invalid="ignore"):
        prod = np.prod([a[l] if S[l] else 1.0 / a[l] for l in range(p)], axis=0)
    for j, lam in enumerate(lams):
        if np.isfinite(lam) and lam != 0:
            assert abs(prod[j] - lam) <= 1e-12 * abs(lam) * p, (j, prod[j], lam)
    V1 = Vs[0]
    assert np.allclose(np.linalg.norm(V1, axis=0), 1.0, atol=1e-13)
    for c in range(V1.shape[1]):
        am = np.argmax(np.abs(V1[:, c]))
        assert V1[am, c].imag == 0 and V1[am, c].real > 0
    W, a1 = eng.geigvecs(P, select, shifted=False)
    assert len(W) == 1 and np.array_equal(W[0], V1) and np.array_equal(a1, a)
    if proto:
        ref, aref = prototype(P, select)
        assert np.allclose(a, aref, rtol=1e-13, atol=0)
        for l in range(p):
            assert np.allclose(Vs[l], ref[l], rtol=0, atol=1e-9), (l, np.abs(Vs[l] - ref[l]).max())
    if dense and n <= 12 and all(np.isfinite(lams)) and all(lams != 0):
        Pm = np.eye(n)
        for l in range(p):
            F = As[l] if S[l] else np.linalg.inv(As[l])
            Pm = F @ Pm if P.orientation == "L" else Pm @ F
        for j, lam in enumerate(lams):
            v = V1[:, j]
            assert np.linalg.norm(Pm @ v - lam * v) <= 1e-9 * np.linalg.norm(Pm, 2), (j, lam)
    return Vs, a


S_ALT = lambda p: [l % 2 == 0 for l in range(p)]  # noqa: E731
S_TFFT = lambda p: [l % 4 in (0, 3) for l in range(p)]  # noqa: E731


def case_signed(eng, cplx, lr, spat):
    """signed Schur forms, schurindex not 1, two signature patterns, all and partial selections"""
    n, p = 9, 5
    S = (S_ALT if spat == "alt" else S_TFFT)(p)
    P, As = signed_form(n, p, S, lr, seed=31 + cplx + 2 * (lr == "R") + 4 * (spat == "alt"), cplx=cplx,
                        pairs=() if cplx else (2, 6), si=3)
    check(eng, P, As, np.ones(n, dtype=bool))
    sel = np.zeros(n, dtype=bool)
    sel[[0, 3, 6, 8]] = True  # (row 6 starts a pair in the real case: completed)
    check(eng, P, As, sel)


def case_end_to_end(eng, cplx):
    """pschur(A, S=...) (Float64: psd_d_gpschur) and gpschur(As, Bs) (ComplexF64), then geigvecs; the default eigvecs
    refuses the signed decomposition instead of returning wrong vectors"""
    rs = np.random.RandomState(41 + cplx)
    n = 6
    if not cplx:
        S = [True, False, True]
        As = [rs.randn(n, n) for _ in S]
        P = eng.pschur(As, "L", S=S)
    else:
        A = [rs.randn(n, n) + 1j * rs.randn(n, n) for _ in range(2)]
        B = [rs.randn(n, n) + 1j * rs.randn(n, n) for _ in range(2)]
        P = eng.gpschur(A, B)
        S = P.S
        As = []  # the factors the decomposition represents
        for l in range(len(S)):
            ln = (l + 1) % len(S)
            fwd = bool(S[l]) == (P.orientation == "L")
            As.append(P.Z[ln] @ P.Ts[l] @ P.Z[l].conj().T if fwd else P.Z[l] @ P.Ts[l] @ P.Z[ln].conj().T)
    assert not all(P.S)
    check(eng, P, As, np.ones(n, dtype=bool))
    with pytest.raises(psd_amd.NotImplementedPSD, match="geigvecs"):
        eng.eigvecs(P, [True] * n)


def case_zero_infinite(eng, cplx, lr):
    """an exact zero on the diagonal of a forward factor (zero eigenvalue) and of an inverted one (infinite)"""
    n, p = 7, 4
    S = [True, False, True, False]
    rs = np.random.RandomState(53 + cplx)
    diag = [1.0 + rs.rand(n) for _ in range(p)]
    diag[0][2] = 0.0  # zero eigenvalue at row 2
    diag[1][4] = 0.0  # infinite eigenvalue at row 4
    P, As = signed_form(n, p, S, lr, diag=diag, seed=57 + cplx, cplx=cplx)
    Vs, a = check(eng, P, As, np.ones(n, dtype=bool), proto=False)
    assert eng.eigvecs_stats.nzero == 2
    left = lr == "L"
    v_zero = Vs[0][:, 2] if left else Vs[1][:, 2]  # A_1 v_1 = 0 ('L'), A_1 v_2 = 0 ('R')
    assert np.linalg.norm(As[0] @ v_zero) <= GATE * np.linalg.norm(As[0]) * np.linalg.norm(v_zero)
    v_inf = Vs[2][:, 4] if left else Vs[1][:, 4]  # A_2 v_3 = 0 ('L'), A_2 v_2 = 0 ('R')
    assert np.linalg.norm(As[1] @ v_inf) <= GATE * np.linalg.norm(As[1]) * np.linalg.norm(v_inf)
    assert a[0, 2] == 0 and a[1, 4] == 0


def case_plain_zero(eng, cplx):
    """a PeriodicSchur with a zero eigenvalue: eigvecs gives NaN, geigvecs a valid vector"""
    n, p = 6, 3
    diag = [np.linspace(1.0, 2.0, n) for _ in range(p)]
    diag[0][3] = 0.0
    ps, As = vc.schur_form(n, p, diag, seed=9, cplx=cplx)
    assert np.isnan(eng.eigvecs(ps, np.ones(n, dtype=bool), method="backsub")[0][:, 3]).all()
    Vs, a = check(eng, ps, As, np.ones(n, dtype=bool), proto=False)
    assert eng.eigvecs_stats.nzero == 1
    assert np.linalg.norm(As[0] @ Vs[0][:, 3]) <= GATE * np.linalg.norm(As[0])


def case_pairs(eng, lr, n=12, pairs=(1, 5, 9)):
    """conjugate pairs of a signed real decomposition, one member selected: the partner is the conjugate"""
    p = 4
    S = S_ALT(p)
    P, As = signed_form(n, p, S, lr, seed=61 + n + (lr == "R"), pairs=pairs, si=2)
    sel = np.zeros(n, dtype=bool)
    sel[pairs[0] + 1] = True
    Vs, a = check(eng, P, As, sel)
    assert Vs[0].shape[1] == 2
    for V in Vs:
        assert np.array_equal(V[:, 1], np.conj(V[:, 0]))
    assert np.array_equal(a[:, 1], np.conj(a[:, 0]))
    check(eng, P, As, np.ones(n, dtype=bool), proto=n <= 12)


def case_chunk_pair(eng, cplx):
    """n = 40: several chunks; a pair at rows 23-24 straddles the chunk boundary at n - 16 (real case)"""
    n, p = 40, 3
    S = [True, False, True]
    rs = np.random.RandomState(13)
    diag = [np.linspace(0.6, 1.9, n) * (1 + 0.2 * rs.rand(n)) for _ in range(p)]
    P, As = signed_form(n, p, S, "L", diag=diag, seed=17, cplx=cplx, pairs=() if cplx else (5, 23, 37))
    for sel in (np.ones(n, dtype=bool), np.arange(n) % 3 == 0):
        check(eng, P, As, sel, proto=False)
    ref, aref = prototype(P, np.arange(n) % 3 == 0)
    Vs, _ = eng.geigvecs(P, np.arange(n) % 3 == 0)
    for l in range(p):
        assert np.allclose(Vs[l], ref[l], rtol=0, atol=1e-9)


def case_repeated(eng, cplx):
    """an exactly repeated finite eigenvalue: finite vectors, perturbed pivots counted"""
    n, p = 6, 4
    S = S_ALT(p)
    P, As = signed_form(n, p, S, "L", diag=[np.full(n, 1.5) for _ in range(p)], seed=7, cplx=cplx)
    Vs, a = eng.geigvecs(P, np.ones(n, dtype=bool))
    assert all(np.isfinite(V).all() for V in Vs)
    assert eng.eigvecs_stats.nperturbed > 0 and Vs[0].shape[1] == n


def case_rescale(eng):
    """graded factors (2^+-175 inside the period, each row's signed product moderate): columns rescaled, still valid"""
    n, p = 8, 6
    S = S_ALT(p)
    diag = []
    for l in range(p):
        g = np.where(np.arange(n) % 2 == 1, 2.0 ** (175 if l < 3 else -175), 1.0)
        d = np.linspace(1.0, 1.7, n) ** (1.0 / p) * g
        diag.append(d if S[l] else 1.0 / d)
    P, As = signed_form(n, p, S, "L", diag=diag, seed=23)
    Vs, a = eng.geigvecs(P, np.ones(n, dtype=bool))
    assert all(np.isfinite(V).all() for V in Vs)
    assert eng.eigvecs_stats.nrescaled > 0
    assert relation_ratio(As, S, "L", Vs, a) <= GATE


def case_vs_eigvecs(eng, cplx, lr):
    """all-true S: geigvecs against eigvecs(method="backsub") on distinct non-zero eigenvalues"""
    import engine_cases as ec

    n, p = 9, 5
    A = ec._distinct_real_factors(n, p, cplx, seed=77 + cplx)
    ps = eng.pschur(A, lr)
    sel = np.ones(n, dtype=bool)
    Vb = eng.eigvecs(ps, sel, method="backsub")
    Vg, a = check(eng, ps, A, sel)
    assert np.allclose(Vg[0], Vb[0], rtol=0, atol=1e-10), np.abs(Vg[0] - Vb[0]).max()
    for l in range(p):
        vc._parallel(Vg[l], Vb[l])
    g = psd_amd.GeneralizedPeriodicSchur([True] * p, ps.Ts, ps.Z, np.array(ps.values), np.ones(n),
                                         np.zeros(n, dtype=np.int32), ps.orientation, ps.schurindex)
    Vh, ah = eng.geigvecs(g, sel)
    assert all(np.array_equal(x, y) for x, y in zip(Vh, Vg)) and np.array_equal(ah, a)


def case_errors(eng):
    n, p = 6, 3
    P, As = signed_form(n, p, [True, False, True], "L", seed=3)
    with pytest.raises(ValueError):
        eng.geigvecs(P, [True] * (n - 1))  # select length
    bad = psd_amd.GeneralizedPeriodicSchur([True, False], P.Ts, P.Z, P.alpha, P.beta, P.alphascale, "L", p)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.geigvecs(bad, [True] * n)  # S length
    bad = psd_amd.GeneralizedPeriodicSchur(P.S, P.Ts, P.Z, P.alpha, P.beta, P.alphascale, "L", p + 1)
    with pytest.raises(ValueError, match="argument 8"):
        eng.geigvecs(bad, [True] * n)  # schurindex
    bad = psd_amd.GeneralizedPeriodicSchur(P.S, P.Ts, [], P.alpha, P.beta, P.alphascale, "L", p)
    with pytest.raises(ValueError):
        eng.geigvecs(bad, [True] * n)  # no Schur vectors
    bad = psd_amd.GeneralizedPeriodicSchur(P.S, P.Ts, [z.astype(np.complex128) for z in P.Z], P.alpha, P.beta,
                                           P.alphascale, "L", p)
    with pytest.raises(TypeError):
        eng.geigvecs(bad, [True] * n)  # real T with complex Z
    with pytest.raises(psd_amd.NotImplementedPSD, match="geigvecs"):
        eng.eigvecs(P, [True] * n)  # the signed default eigvecs
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.eigvecs(P, [True] * n, method="backsub")
