"""Cases of partial_pschur (src/krylov.jl:446-798), shared by the CPU tier (serial simulation of the device code) and the
GPU tier.  The problems and the acceptance rules restate test/krylov.jl of the reference."""
import numpy as np

import psdtest as pt

EPS = np.finfo(np.float64).eps

# ordering of the full spectrum per target (test/krylov.jl:36-38): key, descending
BYES = {"LM": (np.abs, True), "LR": (np.real, True), "SR": (np.real, False), "LI": (np.imag, True),
        "SI": (np.imag, False)}


def mkmats1(n=30, p=3, xpnd=1.25, cplx=False, seed=0, unit=False):
    """test/krylov.jl:40-56: triangular factors whose diagonal products are spread by xpnd^(j-1) in order of magnitude,
    then hidden by orthogonal / unitary similarities between neighbours.  unit: every factor scaled so that the dominant
    eigenvalue of the product has modulus 1 (for the larger cases: the reference's convergence test compares a footer
    entry of one factor with tol |lambda| of the product, which says little when |lambda| is 1e28)."""
    rng = np.random.default_rng(seed)

    def randn(*shape):
        if cplx:
            return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)
        return rng.standard_normal(shape)

    As = [np.triu(randn(n, n)) for _ in range(p)]
    lam = np.prod([np.diag(a) for a in As], axis=0)
    idx = np.argsort(np.abs(lam), kind="stable")
    for j in range(n):
        fac = float(xpnd) ** j
        for a in As:
            a[idx[j], idx[j]] *= fac
    if unit:
        top = np.max(np.abs(np.prod([np.diag(a) for a in As], axis=0)))
        for a in As:
            a /= top ** (1.0 / p)
    for l in range(p):
        q, _ = np.linalg.qr(randn(n, n))
        l1 = (l + 1) % p
        As[l] = As[l] @ q
        As[l1] = q.conj().T @ As[l1]
    return [np.asfortranarray(a) for a in As]


def dominant(n, p, cplx=False, seed=0):
    """Dense factors diag(d) + 0.3 G / sqrt(n) with 16 leading entries of d between 2 and 1.3, the rest 1: the dominant
    eigenvalues of the product are well separated and well conditioned at any order (the triangular construction of
    mkmats1 is not, beyond a few hundred: its eigenvalues are exact but hugely sensitive)."""
    rng = np.random.default_rng(seed)
    d = np.ones(n)
    d[:16] = np.linspace(2.0, 1.3, 16)
    As = []
    for _ in range(p):
        g = rng.standard_normal((n, n))
        if cplx:
            g = (g + 1j * rng.standard_normal((n, n))) / np.sqrt(2)
        a = 0.3 / np.sqrt(n) * g
        a[np.diag_indices(n)] += d
        As.append(np.asfortranarray(a))
    return As


def full_values(As):
    if np.iscomplexobj(As[0]):
        return np.asarray(pt.oracle_zpschur([a.copy() for a in As], "L").values)
    return np.asarray(pt.oracle_pschur([a.copy() for a in As], "L").values)


def check(P, As, tol=1e-10):
    """test/krylov.jl:6-26 for every relation A_l Z_l = Z_{l+1} T_l (the last one up to the Krylov residual, which the
    convergence test bounds by tol |lambda|), plus orthonormality of every Z_l.  Returns the worst normalised numbers."""
    p = len(As)
    n = As[0].shape[0]
    Z = [np.asarray(z) for z in P.Z]
    k = Z[0].shape[1]
    worst_rel, worst_orth = 0.0, 0.0
    for l in range(p):
        a = As[l]
        res = a @ Z[l] - Z[(l + 1) % p] @ P.Ts[l]
        cn = np.linalg.norm(res, axis=0)
        an = np.linalg.norm(a, 2)
        if l < p - 1:
            bound = np.full(k, 1e3 * n * EPS * an)
        else:  # the Krylov residual: the convergence test bounds each locked footer entry by tol |lambda|
            lmax = float(np.max(np.abs(P.values[:k]))) if k else 0.0
            bound = np.full(k, 100 * tol * lmax + 1e3 * n * EPS * an)
        assert np.all(cn <= bound), (l, cn / an, bound / an)
        worst_rel = max(worst_rel, float(np.max(cn / an)) if k else 0.0)
        o = np.linalg.norm(Z[l].conj().T @ Z[l] - np.eye(k))
        assert o < 100 * n * EPS, (l, o)
        worst_orth = max(worst_orth, o)
    for l in range(p - 1):  # T_1..T_{p-1} upper triangular
        assert np.all(np.tril(P.Ts[l], -1) == 0)
    return worst_rel, worst_orth


def check_values(P, vfull, which, nev, rtol=1e-5, among=None, found=0):
    """Every returned value is one of the `among` leading values of the full spectrum in the order of the target
    (default 2 nev; a wide subspace locks many more than nev values, then len(P.values) + nev is the count to pass), and
    the `found` leading values of the full spectrum are each returned to 1e-6 |lambda|."""
    key, desc = BYES[which]
    order = np.argsort(key(vfull), kind="stable")
    if desc:
        order = order[::-1]
    best = vfull[order[: 2 * nev if among is None else among]]
    if not np.iscomplexobj(P.Ts[0]):  # (a real spectrum: the cut may separate a conjugate pair)
        best = np.concatenate([best, np.conj(best)])
    for lam in P.values:
        assert np.any(np.abs(best - lam) <= rtol * np.abs(best)), (lam, best)
    for lam in vfull[order[:found]]:
        assert np.min(np.abs(P.values - lam)) <= 1e-6 * abs(lam), (lam, P.values)


def ev_check(eng, P, As):
    """test/krylov.jl:103-115: eigenvectors of the partial result, A_l v_l = mu v_{l+1} to 20 sqrt(eps)."""
    k = P.Z[0].shape[1] if hasattr(P.Z[0], "shape") else 0
    sel = [False] * k
    for i in range(k >> 1):
        sel[i] = True
    if not any(sel):
        return
    Vs = eng.eigvecs(P, sel)
    Vs = [np.asarray(v.cpu()) if hasattr(v, "cpu") else np.asarray(v) for v in Vs]
    p = len(As)
    nv = Vs[0].shape[1]
    for c in range(nv):
        mu = None
        for l in range(p):
            x, y = Vs[l][:, c], Vs[(l + 1) % p][:, c]
            ax = As[l] @ x
            m = np.vdot(y, ax) / np.vdot(y, y)
            r = np.linalg.norm(ax - m * y) / (np.linalg.norm(As[l], 2) * np.linalg.norm(x))
            assert r < 20 * np.sqrt(EPS), (l, c, r)
            mu = m
        assert mu is not None


def pkstest(eng, As, which, vfull=None, nev=4, k0=6, tol=1e-10, restarts=60, **kw):
    """test/krylov.jl:58-117 (pkstest1): the reference's parameters and acceptance rule."""
    P, hist = eng.partial_pschur(As, nev, which, mindim=k0, maxdim=2 * k0, tol=tol, restarts=restarts, **kw)
    nconv = P.Z[0].shape[1]
    assert nconv >= (nev >> 1), (nconv, hist)
    assert hist.nconverged == nconv and hist.nev == nev
    assert hist.converged == (nconv >= nev)
    assert hist.mvproducts % len(As) == 0 and hist.mvproducts > 0
    assert len(P.values) == nconv and P.schurindex == len(As) and P.orientation == "L"
    check(P, As, tol)
    if vfull is not None:
        check_values(P, vfull, which, nev)
    ev_check(eng, P, As)
    return P, hist


# A subspace wider than a workgroup of the row kernels (ncols > 256: the strided loops of psd_kr_axpy / psd_kr_store take
# a second trip, psd_kr_basis tiles fewer than 64 rows): dominant(600, 2) with these keywords
WIDE_N, WIDE_P, WIDE_NEV = 600, 2, 6
WIDE_KW = dict(mindim=150, maxdim=300, tol=1e-10, restarts=100, seed=1)


def wide_subspace(eng, cplx):
    """dominant(600, 2), nev = 6, mindim = 150, maxdim = 300, tol = 1e-10: converges in the first restart iteration
    (restarts = 1 observed on the serial simulation, real and complex, with well over nev values locked), so the values
    are matched against len(P.values) + nev leading values of the full spectrum, and the nev / 2 dominant ones must be
    found.  The full spectrum comes from numpy's eigvals of the explicit product A_2 A_1: the factors of dominant() are
    well conditioned (it agrees with the oracle's periodic QR to 2e-13 |lambda| on the 40 leading values, in a second
    where the complex oracle takes half a minute at this order)."""
    As = dominant(WIDE_N, WIDE_P, cplx=cplx, seed=51 + int(cplx))
    P, hist = eng.partial_pschur(As, WIDE_NEV, "LM", **WIDE_KW)
    assert hist.nconverged >= WIDE_NEV and hist.converged, hist.__dict__
    assert hist.nconverged == P.Z[0].shape[1] == len(P.values)
    check(P, As, WIDE_KW["tol"])
    check_values(P, np.linalg.eigvals(As[1] @ As[0]), "LM", WIDE_NEV, among=len(P.values) + WIDE_NEV, found=WIDE_NEV // 2)
    return P, hist


def rank_deficient(n=30, p=3, r=3, seed=5):
    """Factor 2 of rank r < the subspace order: its products fall into the span of the basis after r steps, so the
    in-span / re-initialisation / deflation paths of the Arnoldi process run (krylov.jl:300-311, :375-407)."""
    As = mkmats1(n, p, seed=seed)
    rng = np.random.default_rng(seed + 1)
    As[1] = np.asfortranarray(rng.standard_normal((n, r)) @ rng.standard_normal((r, n)))
    return As


def same_bits(P1, h1, P2, h2):
    assert h1.mvproducts == h2.mvproducts and h1.nconverged == h2.nconverged
    assert np.array_equal(P1.values, P2.values)
    for a, b in zip(P1.Ts, P2.Ts):
        assert np.array_equal(a, b)
    for a, b in zip(P1.Z, P2.Z):
        a = a.cpu().numpy() if hasattr(a, "cpu") else a
        b = b.cpu().numpy() if hasattr(b, "cpu") else b
        assert np.array_equal(a, b)
