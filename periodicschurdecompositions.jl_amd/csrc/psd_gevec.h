// Eigenvectors of a signed (generalized) periodic Schur decomposition, zero and infinite eigenvalues included: the
// periodic form of LAPACK xTGEVC.  The companion of psd_evec.h (xTREVC form), whose GEMM, column accessors, 2x2 solve,
// lane segments and normalisation it reuses; the host driver is psd_gevec_host.inl.
//
// Working form (left orientation, 0-based, j cyclic): a forward factor (sgn[j] = 1) gives W_j y_j = a_j y_{j+1}, an
// inverted one (sgn[j] = 0) W_j y_{j+1} = a_j y_j.  The scalars a_j are the diagonal entries of the column's own row
// (the host computes them, and the pair scalars), so y_j = 1 on a 1x1 own row for every j and nothing is divided by the
// eigenvalue.  Per row block I and factor j the relation is homogeneous, c y_{j+1}(I) = A y_j(I) + b:
//   forward:              c = a_j,  A = D_j,            b = r_j = W_j(I, below) y_j(below)
//   inverted, 1x1 row:    c = D_j,  A = a_j,            b = -r_j, r_j = W_j(I, below) y_{j+1}(below)
//   inverted, 2x2 row:    c = 1,    A = a_j D_j^-1,     b = -D_j^-1 r_j
// A map [[A, b], [0, c]] composes by the matrix product, so the chain round the period is a scan over the lanes as in
// psd_evec.h.  The scaling of a map is free (the relation is homogeneous): maps are only renormalised by powers of two.
// A zero c (an open chain) needs no special case: y_j comes from the period rotated to start at j,
// (C - A^(j)) y_j = B^(j), the composition of the inclusive prefix before j and the suffix from j; C is the same for
// every j, and for a 1x1 row so is C - A^(j).  Hence a forward and a backward scan.  A pivot below
// smin = max(eps max(|A|, |C|), tiny) is replaced by smin and counted (the count is taken at factor 0).
// The own 2x2 block of a conjugate pair: y_0 the null vector of C - A round the period, then y_j from the prefixes
// (every c is non-zero there: the factors' 2x2 blocks are nonsingular).
//
// The inverted factors' updates read X_{j+1}: the GEMM through its per-factor B map, the solve kernel from memory
// written before the last PSD_SYNC (lane t reads the next lane's rows only after they are complete).  No atomics; the
// summation order is fixed.
#pragma once
#include "psd_evec.h"

struct psd_gev_args {
    psd_ev_args e;     // T, wmap, bsz, k0, m, kend, X, R, cnt, n, p, ns, six, r0, r1, jlo (mu, lam, ev unused)
    const int* sgn;    // per working factor: 1 forward, 0 inverted
    const double* ac;  // [p][ns] (re, im): the scalar a of working factor j for solve column c
};

template <int B>
struct psd_gm {
    psd_z A[B][B];
    psd_z b[B];
    psd_z c;
};

template <int B>
PSD_HD void psd_gm_norm(psd_gm<B>& m) {
    double mx = zabs1(m.c);
    for (int i = 0; i < B; ++i) {
        mx = fmax(mx, zabs1(m.b[i]));
        for (int k = 0; k < B; ++k) mx = fmax(mx, zabs1(m.A[i][k]));
    }
    if (mx > 0.0 && mx < INFINITY && (mx > 0x1p64 || mx < 0x1p-64)) {
        const double f = ldexp(1.0, -ilogb(mx));
        m.c = zscal(f, m.c);
        for (int i = 0; i < B; ++i) {
            m.b[i] = zscal(f, m.b[i]);
            for (int k = 0; k < B; ++k) m.A[i][k] = zscal(f, m.A[i][k]);
        }
    }
}

template <int B>
PSD_HD psd_gm<B> psd_gm_ident() {
    psd_gm<B> m;
    for (int i = 0; i < B; ++i) {
        m.b[i] = zmk(0.0, 0.0);
        for (int k = 0; k < B; ++k) m.A[i][k] = zmk(i == k ? 1.0 : 0.0, 0.0);
    }
    m.c = zmk(1.0, 0.0);
    return m;
}

// m2 after m1: [[A2, b2], [0, c2]] [[A1, b1], [0, c1]]
template <int B>
PSD_HD psd_gm<B> psd_gm_compose(const psd_gm<B>& m2, const psd_gm<B>& m1) {
    psd_gm<B> r;
    for (int i = 0; i < B; ++i) {
        psd_z s = zmul(m1.c, m2.b[i]);
        for (int k = 0; k < B; ++k) {
            psd_z v = zmk(0.0, 0.0);
            for (int q = 0; q < B; ++q) v = zadd(v, zmul(m2.A[i][q], m1.A[q][k]));
            r.A[i][k] = v;
            s = zadd(s, zmul(m2.A[i][k], m1.b[k]));
        }
        r.b[i] = s;
    }
    r.c = zmul(m2.c, m1.c);
    psd_gm_norm(r);
    return r;
}

// What a map takes from its column beside the factors' entries — the scalar a_l, the sense of working factor l and the
// update product r_l(row) — as the single path keeps them: a in the uploaded table, r in the GEMM's R buffer.  (The
// batched paths have source types of their own: psd_zgbevec.h reads a from the factors, psd_gbevec.h from its tables,
// and both keep r in LDS.)
template <bool CPLX>
struct psd_gev_src {
    const psd_gev_args& g;
    const psd_ev_col<CPLX>& col;
    PSD_HD psd_z a(int l) const {
        return zmk(g.ac[2 * ((size_t)l * g.e.ns + col.j)], g.ac[2 * ((size_t)l * g.e.ns + col.j) + 1]);
    }
    PSD_HD bool fwd(int l) const { return g.sgn[l] != 0; }
    PSD_HD psd_z r(int l, int i) const { return col.r(l, i); }
};

// the map of working factor l on the row block (i, B) of column col.j (own: no r, the rows below are zero)
template <bool CPLX, int B, class SRC>
PSD_HD psd_gm<B> psd_gev_map(const SRC& g, const psd_ev_col<CPLX>& col, int l, int i, bool own) {
    psd_z D[2][2];
    col.d(l, i, B, D);
    const psd_z a = g.a(l);
    psd_z r[2] = {zmk(0.0, 0.0), zmk(0.0, 0.0)};
    if (!own)
        for (int q = 0; q < B; ++q) r[q] = g.r(l, i + q);
    psd_gm<B> m;
    if (g.fwd(l)) {
        for (int q = 0; q < B; ++q) {
            m.b[q] = r[q];
            for (int k = 0; k < B; ++k) m.A[q][k] = D[q][k];
        }
        m.c = a;
    } else if (B == 1) {
        m.A[0][0] = a;
        m.b[0] = zneg(r[0]);
        m.c = D[0][0];
    } else {  // D^-1 = adj(D) / det(D)
        const psd_z rdet = zdiv(zmk(1.0, 0.0), zsub(zmul(D[0][0], D[1][1]), zmul(D[0][1], D[1][0])));
        psd_z Di[2][2] = {{zmul(D[1][1], rdet), zneg(zmul(D[0][1], rdet))},
                          {zneg(zmul(D[1][0], rdet)), zmul(D[0][0], rdet)}};
        for (int q = 0; q < B; ++q) {
            psd_z s = zmk(0.0, 0.0);
            for (int k = 0; k < B; ++k) {
                m.A[q][k] = zmul(a, Di[q][k]);
                s = zsub(s, zmul(Di[q][k], r[k]));
            }
            m.b[q] = s;
        }
        m.c = zmk(1.0, 0.0);
    }
    psd_gm_norm(m);
    return m;
}

PSD_HD int psd_gev_ilogb(psd_z z) {
    const double m = zabs1(z);
    return m > 0.0 ? ilogb(m) : 0;
}

// y_l of every factor l of lane t on the row block (i, B): y = mant * 2^e.  store = false: the largest exponent of the
// segment into mx and the perturbed pivots (counted at factor 0) into np; store = true: X rows i.. scaled by 2^-shift.
// inc, suf: the scans of the column's nl lanes (the wavefront, or a sub-group of it in the batched layout).
template <bool CPLX, int B, class SRC>
PSD_D void psd_gev_lane(const SRC& g, const psd_ev_col<CPLX>& col, const psd_gm<B>* inc, const psd_gm<B>* suf, int t,
                        int nl, int i, bool own, const psd_z* y0, bool store, int shift, int& mx, int& np) {
    const int p = col.a.p;
    const double eps = PSD_DBL_EPS, tiny = PSD_DBL_MIN;
    int lo, hi;
    psd_ev_seg(t, p, lo, hi);
    psd_gm<B> pre = t > 0 ? inc[t - 1] : psd_gm_ident<B>();  // factors 0 .. l-1
    mx = -100000;
    np = 0;
    for (int l = lo; l < hi; ++l) {
        psd_z y[2] = {zmk(0.0, 0.0), zmk(0.0, 0.0)};
        int e = 0;
        if (own) {  // (B == 2) y_l = pre(y_0) / c
            for (int q = 0; q < B; ++q)
                for (int k = 0; k < B; ++k) y[q] = zadd(y[q], zmul(pre.A[q][k], y0[k]));
            if (!ziszero(pre.c)) {
                e = -psd_gev_ilogb(pre.c);
                const psd_z rc = zdiv(zmk(1.0, 0.0), zscal(ldexp(1.0, e), pre.c));
                for (int q = 0; q < B; ++q) y[q] = zmul(y[q], rc);
            }
        } else {
            // the period from l: suffix l .. p-1 (this segment's factors, then the lanes after it), then the prefix
            psd_gm<B> s = psd_gm_ident<B>();
            for (int k = l; k < hi; ++k) s = psd_gm_compose(psd_gev_map<CPLX, B>(g, col, k, i, false), s);
            if (t + 1 < nl) s = psd_gm_compose(suf[t + 1], s);
            const psd_gm<B> T = psd_gm_compose(pre, s);
            double ref = zabs(T.c);
            for (int q = 0; q < B; ++q)
                for (int k = 0; k < B; ++k) ref = fmax(ref, zabs(T.A[q][k]));
            int npl = 0;
            if (B == 1) {
                psd_z d = zsub(T.c, T.A[0][0]);
                const double smin = fmax(eps * ref, tiny);
                if (!(zabs(d) >= smin)) {
                    d = zmk(smin, 0.0);
                    ++npl;
                }
                e = -psd_gev_ilogb(d);
                y[0] = zdiv(T.b[0], zscal(ldexp(1.0, e), d));
            } else {  // (C - A) scaled to its largest entry 1
                psd_z M[2][2], cc[2];
                double mm = 0.0;
                for (int q = 0; q < 2; ++q)
                    for (int k = 0; k < 2; ++k) {
                        M[q][k] = zsub(q == k ? T.c : zmk(0.0, 0.0), T.A[q][k]);
                        mm = fmax(mm, zabs(M[q][k]));
                    }
                const int eM = mm > 0.0 ? ilogb(mm) : 0;
                const double f = ldexp(1.0, -eM);
                for (int q = 0; q < 2; ++q) {
                    cc[q] = T.b[q];
                    for (int k = 0; k < 2; ++k) M[q][k] = zscal(f, M[q][k]);
                }
                const double smin = ref > 0.0 ? fmax(eps * ref * f, tiny) : 1.0;
                npl = psd_ev_solve2(M, cc, smin, y);
                e = -eM;
            }
            if (l == 0) np = npl;
        }
        if (store) {
            for (int q = 0; q < B; ++q) col.setx(l, i + q, zscal(ldexp(1.0, e - shift), y[q]));
        } else {
            const double m = B == 2 ? fmax(zabs1(y[0]), zabs1(y[1])) : zabs1(y[0]);
            if (m > 0.0) mx = e + ilogb(m) > mx ? e + ilogb(m) : mx;
        }
        pre = psd_gm_compose(psd_gev_map<CPLX, B>(g, col, l, i, own), pre);
    }
}

// y_0 of the own 2x2 block of a conjugate pair from the total map round the period (the last entry of the column's
// forward scan): the null vector of C - A, (N01, -N00) or (N11, -N10), scaled to a largest entry in [1, 2)
template <int B>
PSD_HD void psd_gev_null(const psd_gm<B>& tot, psd_z y0[2]) {
    psd_z N[2][2];
    for (int q = 0; q < 2; ++q)
        for (int k = 0; k < 2; ++k) N[q][k] = zsub(tot.A[q % B][k % B], q == k ? tot.c : zmk(0.0, 0.0));
    const bool first = zabs2(N[0][1]) + zabs2(N[0][0]) >= zabs2(N[1][1]) + zabs2(N[1][0]);
    y0[0] = first ? N[0][1] : N[1][1];
    y0[1] = first ? zneg(N[0][0]) : zneg(N[1][0]);
    if (ziszero(y0[0]) && ziszero(y0[1])) y0[0] = zmk(1.0, 0.0);
    const double s = ldexp(1.0, -psd_gev_ilogb(zabs1(y0[0]) > zabs1(y0[1]) ? y0[0] : y0[1]));
    y0[0] = zscal(s, y0[0]);
    y0[1] = zscal(s, y0[1]);
}

#define PSD_GEV_LDS (4 * 64 * sizeof(psd_gm<2>) + 64 * sizeof(int))

// One row block (i, B) of column col.j; rows >= i1 of the chunk are done.
template <bool CPLX, int B>
PSD_D void psd_gev_row(const psd_gev_args& g, const psd_ev_col<CPLX>& col, char* lds, int i, int i1, bool own) {
    const psd_ev_args& a = g.e;
    const psd_gev_src<CPLX> src{g, col};
    const int j = col.j, p = a.p, ke = a.kend[j];
    const int kin = ke < a.r1 ? ke : a.r1;
    psd_gm<B>* F = (psd_gm<B>*)lds;  // [2][64] inclusive forward scan
    psd_gm<B>* Sf = F + 128;         // [2][64] inclusive backward scan
    int* red = (int*)(lds + 4 * 64 * sizeof(psd_gm<2>));
    // r_l(I) = R_l(I) + the in-chunk rows below I (of X_l, or X_{l+1} for an inverted factor), the segment maps
    PSD_PAR_FOR(t, 64) {
        int lo, hi;
        psd_ev_seg(t, p, lo, hi);
        psd_gm<B> seg = psd_gm_ident<B>();
        for (int l = lo; l < hi; ++l) {
            if (!own) {
                const int lx = g.sgn[l] ? l : (l + 1 == p ? 0 : l + 1);
                for (int q = 0; q < B; ++q) {
                    psd_z s = col.r(l, i + q);
                    for (int k = i1; k < kin; ++k) s = zadd(s, zmul(col.w(l, i + q, k), col.x(lx, k)));
                    col.setr(l, i + q, s);
                }
            }
            seg = psd_gm_compose(psd_gev_map<CPLX, B>(src, col, l, i, own), seg);
        }
        F[t] = seg;
        Sf[t] = seg;
    }
    PSD_SYNC();
    // inclusive scans over the lanes (Hillis-Steele, fixed order): F[t] = seg t after .. after seg 0,
    // Sf[t] = seg 63 after .. after seg t (the own block needs only the forward one)
    int cur = 0;
    for (int d = 1; d < 64; d <<= 1) {
        PSD_PAR_FOR(t, 64) {
            F[64 * (1 - cur) + t] = t >= d ? psd_gm_compose(F[64 * cur + t], F[64 * cur + t - d]) : F[64 * cur + t];
            if (!own)
                Sf[64 * (1 - cur) + t] = t + d < 64 ? psd_gm_compose(Sf[64 * cur + t + d], Sf[64 * cur + t])
                                                    : Sf[64 * cur + t];
        }
        PSD_SYNC();
        cur = 1 - cur;
    }
    const psd_gm<B>* inc = F + 64 * cur;
    const psd_gm<B>* suf = Sf + 64 * cur;
    psd_z y0[2] = {zmk(1.0, 0.0), zmk(0.0, 0.0)};
    if (own && B == 2) psd_gev_null(inc[63], y0);
    // the largest entry y_l(I) will have: a column growing past 2^PSD_EV_BIG is scaled down first
    PSD_PAR_FOR(t, 64) {
        int mx, np;
        psd_gev_lane<CPLX, B>(src, col, inc, suf, t, 64, i, own, y0, false, 0, mx, np);
        red[t] = mx;
        if (t == 0 && np) a.cnt[3 * j] += np;
    }
    PSD_SYNC();
    int big = -100000;
    for (int t = 0; t < 64; ++t) big = red[t] > big ? red[t] : big;
    const int shift = big > PSD_EV_BIG ? big - 200 : 0;
    if (shift) PSD_ONE { a.cnt[3 * j + 1] += 1; }
    PSD_PAR_FOR(t, 64) {
        int lo, hi, mx, np;
        psd_ev_seg(t, p, lo, hi);
        if (shift) col.rescale(lo, hi, i1, i, shift);
        psd_gev_lane<CPLX, B>(src, col, inc, suf, t, 64, i, own, y0, true, shift, mx, np);
    }
    PSD_SYNC();
}

// One workgroup (one wavefront) per column of [jlo, ns): the rows of the chunk [r0, r1), bottom up.
template <bool CPLX>
PSD_D void psd_gev_solve_body(const psd_gev_args& g) {
    PSD_LDS_DECL;
    const psd_ev_args& a = g.e;
    const int j = a.jlo + PSD_BLOCK_X;
    psd_ev_col<CPLX> col(a, j);
    const int kk = a.k0[j], mm = a.m[j];
    if (kk < a.r0) return;
    const bool own = kk < a.r1;
    int i1 = own ? kk + mm : a.r1;
    while (i1 > a.r0) {
        const bool isown = own && i1 == kk + mm;
        const int b = isown ? mm : ((a.bsz[i1 - 1] == 0) ? 2 : 1);
        const int i = i1 - b;
        if (isown && b == 1) {  // x_l[k] = 1 for every l
            PSD_PAR_FOR(l, a.p) { col.setx(l, i, zmk(1.0, 0.0)); }
            PSD_SYNC();
        } else if (b == 1) {
            psd_gev_row<CPLX, 1>(g, col, psd_lds, i, i1, false);
        } else {
            psd_gev_row<CPLX, 2>(g, col, psd_lds, i, i1, isown);
        }
        i1 = i;
    }
}
PSD_KERNEL psd_gev_solve_d(psd_gev_args g) { psd_gev_solve_body<false>(g); }
PSD_KERNEL psd_gev_solve_z(psd_gev_args g) { psd_gev_solve_body<true>(g); }

// [p][n][3] elements (E doubles each): T_l(i, i), T_l(i + 1, i), T_l(i, i + 1) (zero past the last row)
PSD_KERNEL psd_gev_gather(const double* T, int n, int p, int E, double* out) {
    PSD_PAR_FOR(t, PSD_NTHREADS) {
        const size_t idx = (size_t)PSD_BLOCK_X * PSD_NTHREADS + t;
        if (idx < (size_t)p * n) {
            const size_t l = idx / n;
            const int i = (int)(idx % n);
            const double* b = T + l * n * n * E;
            for (int e = 0; e < E; ++e) {
                out[(idx * 3) * E + e] = b[((size_t)i * n + i) * E + e];
                out[(idx * 3 + 1) * E + e] = i + 1 < n ? b[((size_t)i * n + i + 1) * E + e] : 0.0;
                out[(idx * 3 + 2) * E + e] = i + 1 < n ? b[((size_t)(i + 1) * n + i) * E + e] : 0.0;
            }
        }
    }
}
