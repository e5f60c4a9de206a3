"""Kernel-level cases of the dense Krylov driver (csrc/psd_krylov.h), shared by the CPU tier (serial simulation) and the
GPU tier: the matvec (psd_kr_mv + the chunk sum of psd_kr_dots), one orthogonalisation stage (psd_kr_dots / psd_kr_axpy /
psd_kr_store) and the basis update (psd_kr_basis), each run once through the diagnostic entries of include/psd_mi355x.h
and compared with a plain numpy reference in extended precision (np.longdouble / np.clongdouble) written here.

Every check returns the worst err / bound ratio it saw, so a reader can see how much room a bound leaves."""
import numpy as np

EPS = np.finfo(np.float64).eps
TINY = np.finfo(np.float64).tiny
NT = 256            # PSD_KR_NT: rows per workgroup (twice as many in the two-row matvec)
BASIS_LDS = 65536   # PSD_KR_BASIS_LDS
ETA = 1.0 / np.sqrt(2.0)


def ld(a):
    """An array in extended precision."""
    return np.asarray(a, dtype=np.clongdouble if np.iscomplexobj(a) else np.longdouble)


def randn(rng, shape, cplx):
    if cplx:
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return rng.standard_normal(shape)


def norm(x):
    """2-norm of a vector in the precision of x (np.linalg.norm would go through Float64 LAPACK for some shapes)."""
    x = np.asarray(x).reshape(-1)
    return np.sqrt(np.sum(x.real * x.real + x.imag * x.imag))


# ---- matvec ----------------------------------------------------------------------------------------------------------
# 1, 2, 3, 31; one row either side of the one-row tile (256) and of the two-row tile (512), odd and even; 1023 and 1026
# in the region where nchunk meets its (n + 31) / 32 cap; 993: the smallest order whose last chunk is ONE column wide
# (asserted in matvec_coverage; no even order below 3000 has one in the two-row body)
MATVEC_ORDERS = (1, 2, 3, 31, 255, 256, 257, 510, 511, 512, 513, 514, 993, 1023, 1026)


def matvec_problem(n, cplx):
    rng = np.random.default_rng(7000 + 2 * n + int(cplx))
    return np.asfortranarray(randn(rng, (n, n), cplx)), randn(rng, n, cplx)


def matvec_bound(A, x):
    """(reference, bound): row i within 8 (n + 2) eps (|A| |x|)_i of the extended-precision product, the bound of
    csr_cases.check_matvec with nnz_i = n (any summation order, fused or not; complex products add 2 sqrt(2) < 4)."""
    n = A.shape[0]
    ref = ld(A) @ ld(x)
    bound = 8 * (n + 2) * EPS * (np.abs(A) @ np.abs(x))
    return ref, bound


def check_matvec_result(y, geom, n, cplx, ref, bound, rp):
    """y against the reference, and the geometry against the header's formulas for the body `rp` that must have run."""
    assert y.shape == (n,) and np.iscomplexobj(y) == cplx
    assert geom["rp"] == rp, geom
    tiles = -(-n // (NT * rp))
    nchunk0 = max(1, min(-(-1024 // tiles), (n + 31) // 32))
    ccols = -(-n // nchunk0)
    assert (geom["tiles"], geom["ccols"], geom["nchunk"]) == (tiles, ccols, -(-n // ccols)), geom
    assert geom["nblk"] == -(-n // NT)
    err = np.abs(ld(y) - ref)
    assert np.all(err <= bound), (n, cplx, geom, int(np.argmax(err - bound)), float(np.max(err / np.maximum(bound, TINY))))
    return float(np.max(err / np.maximum(bound, TINY)))


def check_matvec(eng, n, cplx):
    """One order: even real orders must take the two-row body, odd or complex ones the one-row body."""
    A, x = matvec_problem(n, cplx)
    ref, bound = matvec_bound(A, x)
    y, geom = eng.dense_matvec(A, x)
    return check_matvec_result(y, geom, n, cplx, ref, bound, 2 if (not cplx and n % 2 == 0) else 1), geom


def matvec_coverage(geoms, bodies=(1, 2)):
    """From the geometry the entry reported for every (n, geom) of the sweep: the set holds a last chunk narrower than
    the others, an odd chunk width and a single chunk, in the one-row and in the two-row body alike, and a last chunk of
    one column in the one-row body, so a change of the chunk formula cannot silently empty a case."""
    for rp in bodies:
        gs = [(n, g) for n, g in geoms if g["rp"] == rp]
        last = [n - (g["nchunk"] - 1) * g["ccols"] for n, g in gs]
        assert any(g["nchunk"] > 1 and w < g["ccols"] for (n, g), w in zip(gs, last)), (rp, gs)
        assert rp == 2 or any(g["nchunk"] > 1 and w == 1 for (n, g), w in zip(gs, last)), (rp, gs)
        assert any(g["nchunk"] > 1 and g["ccols"] % 2 == 1 for n, g in gs), (rp, gs)
        assert any(g["nchunk"] == 1 for n, g in gs), (rp, gs)


# ---- orthogonalisation -----------------------------------------------------------------------------------------------
# (257, 0 / 1 / 20): a tail workgroup of one row; (513, 255 .. 300): the strided loops of psd_kr_axpy / psd_kr_store take
# a second trip and nblk = 3; (256, 40): all workgroups full; (31, 30): one short of the whole space
ORTH_SHAPES = ((257, 0), (257, 1), (257, 20), (513, 255), (513, 256), (513, 257), (513, 300), (256, 40), (31, 30))
ORTH_KINDS = ("random", "onepass", "twopass", "inspan")
SENTINEL = 12345.678  # what column ncols of the basis holds before a stage


def orth_problem(n, ncols, cplx, kind):
    """U: ncols orthonormal columns from a QR of a random matrix.  v by kind:
    random   a standard-normal vector; whether one Gram-Schmidt pass suffices follows from the rule ||w|| < eta ||v||
             and is taken from the reference (a random vector loses about ncols / n of its squared norm, so at ncols
             near or above n / 2 the second pass must run);
    onepass  the same vector with its component in span(U) scaled to half the norm of the rest: ||w|| / ||v|| = 0.894,
             one pass suffices at every shape;
    twopass  U c + 1e-6 w: the first pass removes nearly all of the norm, the second must run;
    inspan   U c."""
    rng = np.random.default_rng(9000 + 7 * n + 3 * ncols + int(cplx))
    U = np.asfortranarray(np.linalg.qr(randn(rng, (n, max(ncols, 1)), cplx))[0][:, :ncols])
    w = randn(rng, n, cplx)
    c = randn(rng, ncols, cplx)
    if kind == "random":
        v = w
    elif kind == "onepass":
        par = U @ (U.conj().T @ w)
        perp = w - par
        v = perp + (0.5 * np.linalg.norm(perp) / np.linalg.norm(par)) * par if ncols else w
    elif kind == "twopass":
        v = U @ c + 1e-6 * w
    else:
        v = U @ c
    return U, np.ascontiguousarray(v)


def orth_reference(U, v):
    """Two-pass classical Gram-Schmidt in extended precision: (h, hjj, ||w1|| / ||v||), w1 the vector after pass one."""
    Ul, vl = ld(U), ld(v)
    h1 = Ul.conj().T @ vl
    w = vl - Ul @ h1
    ratio = norm(w) / norm(vl) if norm(vl) > 0 else np.longdouble(0)
    h2 = Ul.conj().T @ w
    w = w - Ul @ h2
    return h1 + h2, norm(w), float(ratio)


def check_orth(eng, n, ncols, cplx, kind):
    """One stage against the reference; returns the worst err / bound ratio of the numeric bounds (0.0 for a stop)."""
    U, v = orth_problem(n, ncols, cplx, kind)
    sent = np.full(n, SENTINEL)
    h, hjj, unew, st, Uafter = eng.kr_orth(U, v, sent)
    h2, hjj2, unew2, st2, _ = eng.kr_orth(U, v, sent)
    # no floating-point atomics anywhere: the same call twice gives the same bits
    assert np.array_equal(h, h2) and hjj == hjj2 and np.array_equal(unew, unew2) and st == st2
    assert np.array_equal(Uafter, U)  # the basis columns are only read
    assert st["nblk"] == -(-n // NT)
    href, hjjref, ratio = orth_reference(U, v)
    vn = float(norm(ld(v)))
    if kind == "inspan" and ncols > 0:
        # v = U c: the stage stops the step with kind 1 and writes no column
        assert st["reorth"] == 1, st
        assert st["stop"] == 1 and st["kind"] == 1, (st, hjj, vn)
        assert hjj == 0.0
        assert np.array_equal(unew, sent.astype(unew.dtype))
        worst = float(np.max(np.abs(ld(h) - href)) / (8 * (n + 2) * EPS * vn))
        assert worst <= 1.0, worst
        return worst
    if kind == "inspan":  # ncols = 0: the span is {0}, U c the null vector: kind 2 (the null test of a first column)
        assert st["stop"] == 1 and st["kind"] == 2 and hjj == 0.0, st
        assert np.array_equal(unew, sent.astype(unew.dtype))
        return 0.0
    assert st["stop"] == 0 and st["kind"] == 0, st
    if ncols == 0:
        assert st["reorth"] == 0, st
    elif kind == "onepass":
        assert st["reorth"] == 0, (st, ratio)
    elif kind == "twopass":
        assert st["reorth"] == 1, (st, ratio)
    elif abs(ratio - ETA) > 1e-6:  # random: the rule itself, unless the norms sit on the threshold to rounding
        assert st["reorth"] == int(ratio < ETA), (st, ratio)
    Ul, ul, hl = ld(U), ld(unew), ld(h)
    ratios = []
    ratios.append(float(norm(Ul.conj().T @ ul)) / (100 * n * EPS) if ncols else 0.0)  # orthogonal to the basis
    ratios.append(abs(float(norm(ul) - 1)) / (10 * EPS))                              # normalised
    unorm = float(np.linalg.norm(U, 2)) if ncols else 0.0
    rec = norm(Ul @ hl + np.longdouble(hjj) * ul - ld(v))                             # v = U h + hjj u_new
    ratios.append(float(rec) / (8 * (ncols + 2) * EPS * (unorm * float(norm(hl)) + hjj) + n * EPS * vn))
    hb = 8 * (n + 2) * EPS * vn                                                       # coefficients and norm
    ratios.append(float(np.max(np.abs(hl - href))) / hb if ncols else 0.0)
    ratios.append(abs(float(np.longdouble(hjj) - hjjref)) / hb)
    assert max(ratios) <= 1.0, (n, ncols, cplx, kind, st, ratios)
    return max(ratios)


# ---- basis update ----------------------------------------------------------------------------------------------------
# (n, m, cplx): R = 64 with a row-tile tail of 1; R = 11; R = 2 with the LDS tile exactly at the budget; a single column
BASIS_SHAPES = ((257, 12, False), (257, 12, True), (130, 700, False), (70, 2048, True), (64, 1, False), (64, 1, True))
BASIS_P, BASIS_A0, BASIS_PAD = 3, 2, 3  # factors; first updated column; columns behind the updated block


def basis_rows(m, cplx):
    """R as the header gives it: the R x m tile fits the LDS budget, at most 64 rows."""
    return max(1, min(64, BASIS_LDS // (m * (16 if cplx else 8))))


def _slices(A, axis, nbits=20, count=3):
    """A (real) as a sum of `count` matrices whose entries are integers of at most nbits bits times a power of two that
    is common to every entry along `axis`, plus a remainder below 2^-60 of the largest entry along that axis."""
    mx = np.max(np.abs(A), axis=axis, keepdims=True)
    e = np.ceil(np.log2(np.where(mx > 0, mx, 1.0)))
    out, rest = [], A.copy()
    for s in range(count):
        sigma = 1.5 * np.exp2(e + 52 - nbits * (s + 1))  # (x + sigma) - sigma: x rounded to a multiple of 2^(e - nbits (s + 1))
        top = (rest + sigma) - sigma
        out.append(top)
        rest = rest - top  # exact
    return out


def product_ld(A, B):
    """A B in extended precision for matrices too large for numpy's own longdouble product (minutes at m = 2048): the
    factors are cut into slices of 20 significant bits (rows of A and columns of B share an exponent), so every Float64
    product of two slices is exact whatever the summation order (20 + 20 + 11 bits <= 53 for an inner dimension up to
    2048), and the exact pieces are added in np.longdouble.  The slice pairs left out are below 2^-58 of (largest entry of
    the row) x (largest entry of the column) x m, some 1e-4 of the bounds used here for standard-normal entries;
    test_product_ld_matches_numpy pins the function against numpy's longdouble product at a small shape."""
    assert A.shape[1] <= 2048
    if np.iscomplexobj(A) or np.iscomplexobj(B):
        A, B = np.asarray(A, dtype=np.complex128), np.asarray(B, dtype=np.complex128)
        ar, ai, br, bi = A.real, A.imag, B.real, B.imag
        return (product_ld(ar, br) - product_ld(ai, bi)) + 1j * (product_ld(ar, bi) + product_ld(ai, br))
    sa, sb = _slices(np.asarray(A, dtype=np.float64), 1), _slices(np.asarray(B, dtype=np.float64), 0)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.longdouble)
    for i in range(3):
        for j in range(3 - i):
            acc += sa[i] @ sb[j]
    return acc


def check_basis(eng, n, m, cplx):
    rng = np.random.default_rng(11000 + n + m + int(cplx))
    cols = BASIS_A0 + m + BASIS_PAD
    V = [np.asfortranarray(randn(rng, (n, cols), cplx)) for _ in range(BASIS_P)]
    Q = [np.asfortranarray(randn(rng, (m, m), cplx)) for _ in range(BASIS_P)]  # (a product check: Q_l any matrix)
    W, R = eng.kr_basis(V, Q, BASIS_A0)
    assert R == basis_rows(m, cplx), (R, m, cplx)
    worst = 0.0
    blk = slice(BASIS_A0, BASIS_A0 + m)
    for l in range(BASIS_P):
        assert W[l].shape == V[l].shape and np.iscomplexobj(W[l]) == cplx
        assert np.array_equal(W[l][:, :BASIS_A0], V[l][:, :BASIS_A0]), l   # columns outside the block: untouched
        assert np.array_equal(W[l][:, BASIS_A0 + m:], V[l][:, BASIS_A0 + m:]), l
        ref = product_ld(V[l][:, blk], Q[l])
        bound = 8 * (m + 2) * EPS * (np.abs(V[l][:, blk]) @ np.abs(Q[l]))
        err = np.abs(ld(W[l][:, blk]) - ref)
        assert np.all(err <= bound), (n, m, cplx, l, float(np.max(err / np.maximum(bound, TINY))))
        worst = max(worst, float(np.max(err / np.maximum(bound, TINY))))
    return worst
