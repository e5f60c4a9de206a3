"""eigvecs(ps, select; shifted) by periodic back-substitution (method="backsub", psd_?_eigvecs) — the cases shared by the
simulated tier (test_hostsim_eigvecs.py) and the device tier (test_gpu_eigvecs.py), and a numpy prototype of the
algorithm as their host reference."""
import numpy as np
import pytest

import engine_cases as ec
import psdtest as pt
import psd_amd

GATE = 1e-11


def backsub_ref(ps, select):
    """numpy prototype: periodic back-substitution in the left working form W_j y_j = mu y_{j+1}, then V_l = Z_l x_l,
    ||V_1(:, c)|| = 1 with its largest entry real positive; the partner of a real pair is the conjugate."""
    Ts, p, n = ps.Ts, len(ps.Ts), ps.Ts[0].shape[0]
    left, si = ps.orientation == "L", ps.schurindex
    W = [Ts[j] if left else Ts[p - 1 - j] for j in range(p)]
    six = si - 1 if left else p - si
    vmap = [l if left else (p - l) % p for l in range(p)]
    lam = np.asarray(ps.values, dtype=complex)
    real = not np.iscomplexobj(Ts[0])
    bsz = [1] * n
    for i in range(n - 1):
        if real and bsz[i] == 1 and Ts[si - 1][i + 1, i] != 0:
            bsz[i], bsz[i + 1] = 2, 0

    def D(j, i, b):
        d = np.array(W[j][i:i + b, i:i + b], dtype=complex)
        if b == 2 and j != six:
            d[1, 0] = 0
        return d

    cols = []
    i = 0
    while i < n:
        b = bsz[i]
        if select[i] or (b == 2 and select[i + 1]):
            cols.append((i, b))
        i += b
    out = []
    for k, m in cols:
        mu = complex(lam[k] + 0j) ** (1.0 / p)
        Y = np.zeros((p, n), dtype=complex)
        y = np.array([1.0, 0.0][:m], dtype=complex)
        if m == 2:
            G = np.eye(2, dtype=complex)
            for j in range(p):
                G = D(j, k, 2) @ G / mu
            N = G - np.eye(2)
            v1, v2 = np.array([N[0, 1], -N[0, 0]]), np.array([N[1, 1], -N[1, 0]])
            y = v1 if np.linalg.norm(v1) >= np.linalg.norm(v2) else v2
        for j in range(p):
            Y[j, k:k + m] = y
            y = D(j, k, m) @ y / mu
        i1 = k
        while i1 > 0:
            b = 2 if bsz[i1 - 1] == 0 else 1
            i = i1 - b
            r = [W[j][i:i1, i1:k + m] @ Y[j, i1:k + m] for j in range(p)]
            c, G = np.zeros(b, dtype=complex), np.eye(b, dtype=complex)
            for j in range(p):
                c = (D(j, i, b) @ c + r[j]) / mu
                G = D(j, i, b) @ G / mu
            y = np.linalg.solve(np.eye(b) - G, c)
            for j in range(p):
                Y[j, i:i1] = y
                y = (D(j, i, b) @ y + r[j]) / mu
            big = np.abs(Y).max()
            if big > 2.0 ** 500:  # the power-of-two column scaling (exact)
                Y *= 2.0 ** -(int(np.log2(big)) - 200)
            i1 = i
        V = [ps.Z[l] @ Y[vmap[l]] for l in range(p)]
        am = np.argmax(np.abs(V[0]))
        s = np.conj(V[0][am]) / abs(V[0][am]) / np.linalg.norm(V[0])
        out.append([s * v for v in V])
        if m == 2:
            out.append([np.conj(s * v) for v in V])
    return [np.stack([c[l] for c in out], axis=1) for l in range(p)]


def relation_ratio(As, Vs, lams, left=True):
    """max over l and columns of ||A_l v_l - mu v_{l+1}|| / (||A_l||_F ||v_l||) (right: A_l v_{l+1} - mu v_l)."""
    p = len(As)
    worst = 0.0
    for k in range(Vs[0].shape[1]):
        mu = complex(lams[k] + 0j) ** (1.0 / p)
        for l in range(p):
            x, y = (Vs[l][:, k], Vs[(l + 1) % p][:, k]) if left else (Vs[(l + 1) % p][:, k], Vs[l][:, k])
            worst = max(worst, np.linalg.norm(As[l] @ x - mu * y) / (np.linalg.norm(As[l]) * np.linalg.norm(x)))
    return worst


def order_values(ps, select):
    """the eigenvalues in the order of the returned columns (top to bottom, pairs completed)"""
    lam = np.asarray(ps.values)
    sel = np.array(select, dtype=bool)
    real = not np.iscomplexobj(ps.Ts[0])
    for j in range(len(lam) - 1):
        if real and lam[j].imag != 0 and lam[j + 1] == np.conj(lam[j]) and (sel[j] or sel[j + 1]):
            sel[j] = sel[j + 1] = True
    return lam[sel]


def check_columns(ps, Vs, select, As):
    lams = order_values(ps, select)
    assert Vs[0].shape[1] == len(lams)
    ec.ev_check(As, Vs, lams, left=(ps.orientation == "L"))
    r = relation_ratio(As, Vs, lams, left=(ps.orientation == "L"))
    assert r <= GATE, r
    ref = backsub_ref(ps, select)
    for l in range(len(Vs)):
        assert np.allclose(Vs[l], ref[l], rtol=0, atol=1e-9), (l, np.abs(Vs[l] - ref[l]).max())
    V1 = Vs[0]
    assert np.allclose(np.linalg.norm(V1, axis=0), 1.0, atol=1e-13)
    for c in range(V1.shape[1]):
        am = np.argmax(np.abs(V1[:, c]))
        assert V1[am, c].imag == 0 and V1[am, c].real > 0
    return lams


def _clone(ps):
    return type(ps)([t.copy(order="F") for t in ps.Ts], [z.copy(order="F") for z in ps.Z], np.array(ps.values),
                    ps.orientation, ps.schurindex)


def case_vectors_jl(eng, cplx, p):
    """test/vectors.jl: smallest and largest two eigenvalues of the distinct-real problems."""
    n = 7
    A = ec._distinct_real_factors(n, p, cplx, seed=60 + p + 10 * cplx)
    ps0 = eng.pschur(A, "L")
    keepT, keepZ = [t.copy() for t in ps0.Ts], [z.copy() for z in ps0.Z]
    lam0 = np.array(ps0.values)
    for rev in (False, True):
        idx = np.argsort(-np.abs(lam0) if rev else np.abs(lam0), kind="stable")
        select = np.zeros(n, dtype=bool)
        select[idx[:2]] = True
        Vs = eng.eigvecs(ps0, select, method="backsub")
        assert len(Vs) == p and Vs[0].shape == (n, 2)
        check_columns(ps0, Vs, select, A)
        V1 = eng.eigvecs(ps0, select, shifted=False, method="backsub")
        assert len(V1) == 1 and np.array_equal(V1[0], Vs[0])  # bit-identical
    assert all(np.array_equal(a, b) for a, b in zip(keepT, ps0.Ts))  # ps is not modified
    assert all(np.array_equal(a, b) for a, b in zip(keepZ, ps0.Z))


def _parallel(Va, Vb):
    assert Va.shape == Vb.shape
    for c in range(Va.shape[1]):
        a = Va[:, c] / np.linalg.norm(Va[:, c])
        b = Vb[:, c] / np.linalg.norm(Vb[:, c])
        assert 1 - abs(np.vdot(a, b)) <= 1e-8, (c, 1 - abs(np.vdot(a, b)))


def case_vs_ordschur(eng, cplx):
    n, p = 9, 5
    A = ec._distinct_real_factors(n, p, cplx, seed=77 + cplx)
    ps0 = eng.pschur(A, "L")
    select = np.ones(n, dtype=bool)
    select[[1, 4]] = False
    Vb = eng.eigvecs(ps0, select, method="backsub")
    Vo = eng.eigvecs(ps0, select)
    for l in range(p):
        _parallel(Vb[l], Vo[l])


def case_pairs(eng, lr):
    """conjugate pairs (the 2x2 own block) in a real decomposition, one member selected, both orientations; the left
    orientation has schurindex = p"""
    n, p = 12, 3
    A = pt.bench_factors(n, p, seed=91)
    ps0 = eng.pschur(A, lr)
    assert ps0.schurindex == (p if lr == "L" else 1)
    lam0 = np.array(ps0.values)
    cidx = [j for j in range(n) if lam0[j].imag > 0]
    assert cidx
    select = np.zeros(n, dtype=bool)
    select[cidx[0]] = True
    Vs = eng.eigvecs(ps0, select, method="backsub")
    assert Vs[0].shape[1] == 2
    for V in Vs:
        assert np.array_equal(V[:, 1], np.conj(V[:, 0]))
    check_columns(ps0, Vs, select, A)
    allsel = np.ones(n, dtype=bool)
    Vs = eng.eigvecs(ps0, allsel, method="backsub")
    check_columns(ps0, Vs, allsel, A)
    for l in range(p):
        _parallel(Vs[l], eng.eigvecs(ps0, allsel)[l])


def schur_form(n, p, diag, seed, cplx=False, pairs=()):
    """a periodic Schur form built directly (left orientation, schurindex p): T_l upper triangular with the given
    diagonals (diag[l][i]), random orthogonal Z_l; A_l = Z_{l+1} T_l Z_l'.  `pairs`: rows i where T_p gets a 2x2 block
    with complex eigenvalues."""
    rs = np.random.RandomState(seed)
    dt = np.complex128 if cplx else np.float64
    Ts = []
    for l in range(p):
        t = 0.1 * np.triu(rs.rand(n, n) + (1j * rs.rand(n, n) if cplx else 0), 1).astype(dt)
        t[np.arange(n), np.arange(n)] = diag[l]
        Ts.append(np.asfortranarray(t))
    for i in pairs:
        Ts[-1][i, i + 1], Ts[-1][i + 1, i], Ts[-1][i + 1, i + 1] = 0.7, -0.5, Ts[-1][i, i]
    Zs = []
    for l in range(p):
        g = rs.randn(n, n) + (1j * rs.randn(n, n) if cplx else 0)
        Zs.append(np.asfortranarray(np.linalg.qr(g)[0]))
    vals = np.prod(np.array([np.diag(t) for t in Ts]), axis=0).astype(complex)
    for i in pairs:
        P = np.eye(2)
        for t in Ts:
            P = t[i:i + 2, i:i + 2] @ P
        ev = np.linalg.eigvals(P)
        vals[i], vals[i + 1] = ev[np.argmax(ev.imag)], ev[np.argmin(ev.imag)]
    As = [Zs[(l + 1) % p] @ Ts[l] @ Zs[l].conj().T for l in range(p)]
    return psd_amd.PeriodicSchur(Ts, Zs, vals, "L", p), As


def case_negative_even_p(eng):
    """a negative real eigenvalue with even p: mu is complex, so are the vectors of a real decomposition"""
    n, p = 6, 4
    diag = [np.linspace(1.0, 2.0, n) for _ in range(p)]
    diag[1] = diag[1].copy()
    diag[1][2] = -1.3
    ps, As = schur_form(n, p, diag, seed=5, pairs=(4,))
    select = np.ones(n, dtype=bool)
    Vs = eng.eigvecs(ps, select, method="backsub")
    assert np.abs(Vs[0][:, 2].imag).max() < 1e-12  # (an eigenvector of the real product: real in V_1 ...)
    assert np.abs(Vs[1][:, 2].imag).max() > 1e-3   # (... but v_2 = A_1 v_1 / mu with mu complex)
    check_columns(ps, Vs, select, As)


def case_repeated(eng, cplx):
    """an exactly repeated diagonal: finite vectors, perturbed pivots counted, no exception"""
    n, p = 6, 3
    ps, As = schur_form(n, p, [np.full(n, 1.5) for _ in range(p)], seed=7, cplx=cplx)
    Vs = eng.eigvecs(ps, np.ones(n, dtype=bool), method="backsub")
    assert all(np.isfinite(V).all() for V in Vs)
    assert eng.eigvecs_stats.nperturbed > 0
    assert Vs[0].shape[1] == n


def case_zero(eng, cplx):
    """an eigenvalue zero: its column is NaN and counted; the others are unaffected"""
    n, p = 6, 3
    diag = [np.linspace(1.0, 2.0, n) for _ in range(p)]
    diag[0] = diag[0].copy()
    diag[0][3] = 0.0
    ps, As = schur_form(n, p, diag, seed=9, cplx=cplx)
    Vs = eng.eigvecs(ps, np.ones(n, dtype=bool), method="backsub")
    assert eng.eigvecs_stats.nzero == 1
    assert all(np.isnan(V[:, 3]).all() for V in Vs)
    keep = [0, 1, 2, 4, 5]
    Vk = [V[:, keep] for V in Vs]
    assert relation_ratio(As, Vk, np.asarray(ps.values)[keep]) <= GATE


def case_errors(eng):
    n, p = 7, 3
    A = ec._distinct_real_factors(n, p, False, seed=3)
    ps0 = eng.pschur(A, "L")
    with pytest.raises(ValueError):
        eng.eigvecs(ps0, [True] * (n - 1), method="backsub")  # select length (vectors.jl:34-36)
    bad = _clone(ps0)
    bad.Z = []
    with pytest.raises(ValueError):
        eng.eigvecs(bad, [True] * n, method="backsub")  # no Schur vectors (vectors.jl:30-32)
    bad = _clone(ps0)
    bad.schurindex = p + 1
    with pytest.raises(ValueError, match="argument 8"):
        eng.eigvecs(bad, [True] * n, method="backsub")
    with pytest.raises(ValueError):
        eng.eigvecs(ps0, [True] * n, method="nonsense")
    bad = _clone(ps0)
    bad.Z = [z.astype(np.complex128) for z in bad.Z]
    with pytest.raises(TypeError):  # real T with complex Z: rejected, not run as a complex problem
        eng.eigvecs(bad, [True] * n, method="backsub")
    g = psd_amd.GeneralizedPeriodicSchur([True, False, True], ps0.Ts, ps0.Z, np.array(ps0.values), np.ones(n),
                                         np.zeros(n, dtype=np.int32), "L", p)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.eigvecs(g, [True] * n, method="backsub")
    # an all-true signature is the plain decomposition
    g.S = [True] * p
    sel = [True, False, True, False, False, True, True]
    assert np.array_equal(eng.eigvecs(g, sel, method="backsub")[2], eng.eigvecs(ps0, sel, method="backsub")[2])


def case_partial(eng, cplx):
    import krylov_cases as kc

    As = kc.mkmats1(30, 3, cplx=cplx, seed=11 + cplx)
    P, _ = eng.partial_pschur(As, 4, "LM", mindim=6, maxdim=12, tol=1e-10, restarts=60)
    k = P.Z[0].shape[1]
    sel = [i < k - 1 for i in range(k)]
    Vb = eng.eigvecs(P, sel, method="backsub")
    Vo = eng.eigvecs(P, sel)
    Vb = [np.asarray(v.cpu()) if hasattr(v, "cpu") else np.asarray(v) for v in Vb]
    Vo = [np.asarray(v.cpu()) if hasattr(v, "cpu") else np.asarray(v) for v in Vo]
    for l in range(len(As)):
        _parallel(Vb[l], Vo[l])


def case_chunks(eng, cplx):
    """n = 40: several chunks of the back-substitution, so the update products of the rows below run; a 2x2 block at
    rows 23-24 straddles the chunk boundary at row n - 16 and must stay whole (real case)."""
    n, p = 40, 3
    rs = np.random.RandomState(13)
    diag = [np.linspace(0.6, 1.9, n) * (1 + 0.2 * rs.rand(n)) for _ in range(p)]
    ps, As = schur_form(n, p, diag, seed=17, cplx=cplx, pairs=() if cplx else (5, 23, 37))
    for select in (np.ones(n, dtype=bool), np.arange(n) % 3 == 0):
        Vs = eng.eigvecs(ps, select, method="backsub")
        check_columns(ps, Vs, select, As)


def case_rescale(eng):
    """diagonals graded over 2^+-175 inside the period (each row's product stays moderate): the vectors of the middle
    factors are about 2^525 apart in their rows, past the 2^500 bound, so columns are rescaled by powers of two; finite,
    the relation holds, and they match the unscaled prototype (which still fits the exponent range here)"""
    n, p = 8, 6
    diag = []
    for l in range(p):
        g = np.where(np.arange(n) % 2 == 1, 2.0 ** (175 if l < 3 else -175), 1.0)
        diag.append(np.linspace(1.0, 1.7, n) ** (1.0 / p) * g)
    ps, As = schur_form(n, p, diag, seed=23)
    select = np.ones(n, dtype=bool)
    Vs = eng.eigvecs(ps, select, method="backsub")
    assert all(np.isfinite(V).all() for V in Vs)
    assert eng.eigvecs_stats.nrescaled > 0
    assert relation_ratio(As, Vs, np.asarray(ps.values)) <= GATE
    ref = backsub_ref(ps, select)
    for l in range(p):
        for c in range(n):
            err = np.linalg.norm(Vs[l][:, c] - ref[l][:, c])
            assert err <= 1e-9 * np.linalg.norm(ref[l][:, c]), (l, c, err)
