// Eigenvectors of a periodic Schur decomposition by periodic back-substitution (the periodic form of LAPACK xTREVC),
// followed by the back-transform V_l = Z_l X_l.  Replaces the loop of ordschur! calls of eigvecs(ps, select; shifted)
// (src/vectors.jl:25-138 of the reference) for factors resident in HBM; the host driver is psd_evec_host.inl.
//
// Working form: the LEFT orientation W_j y_j = mu y_{j+1} (j cyclic, 0-based here), W_j the triangular factors (one of
// them quasi-triangular: `six`), mu = lambda^(1/p).  A right-oriented decomposition runs the sequence in reverse; the
// host maps the user's factors onto working indices (wmap) and back.  y_j is zero below the eigenvalue's own block.
//
// Storage: X = [p][n][ns] as two real planes (re, im), one column per solve column (a conjugate pair of a real
// decomposition is one solve column; its partner is the conjugate, written at the end).  The columns are sorted by the
// row of their own block, so the columns that still need rows r >= r0 are a suffix [jlo, ns) of the list.
//
// The rows are processed bottom-up in chunks [r0, r1) of at most PSD_EV_CH rows that do not split a 2x2 block:
//   * psd_ev_gemm:  R_j(r0:r1, c) = W_j(r0:r1, r1:kend) X_j(r1:kend, c) for every working factor j and column panel
//                   (v_mfma_f64_16x16x4_f64; a real W times the two planes is two real products, a complex W four).  K
//                   stops at the end of the panel's last column: the blocks of zeros below the own rows are skipped.
//   * psd_ev_solve: one wavefront per column, its lanes over the factors: the own block where it lies in the chunk,
//                   then each row block I of the chunk bottom-up: r_j(I) = R_j(I) + W_j(I, in-chunk rows below I) y_j(..)
//                   for every j at once, the cyclic recurrence y_{j+1}(I) = (D_j y_j(I) + r_j(I)) / mu as a scan of
//                   affine maps over the lanes (log2 64 steps), giving y_0(I) = G y_0(I) + c round the period; then
//                   (I - G) y_0(I) = c, G = prod D_j / mu^p, and every y_j(I) from the scan's prefixes.
// The same GEMM kernel then forms V_l = Z_l X_l (output interleaved, column-major), and psd_ev_norm normalises V_1.
//
// Rules (xTREVC's): |1 - G| (a 1x1 row: (lambda - lambda_i) / lambda) or a pivot of the 2x2 solve below
// smin = max(eps * max(1, |I - G|), tiny) is replaced by smin and counted.  A column whose values grow past 2^PSD_EV_BIG
// is scaled by a power of two (exact: the normalisation at the end removes it) and counted.  mu = 0: the column is not
// computed and comes back as NaN.  No atomics, no cross-workgroup waits; every reduction runs in a fixed order.
#pragma once
#include "psd_complex.h"

#define PSD_EV_RB 32   // rows of the GEMM tile (and of the R buffer)
#define PSD_EV_TN 64   // columns of a GEMM panel
#define PSD_EV_TK 16   // K step of the GEMM
#define PSD_EV_BIG 500 // log2 of the growth bound of a column
#define PSD_EV_CH 16   // rows of a chunk of the back-substitution (<= PSD_EV_RB)

struct psd_ev_gemm_args {
    const double* A;  // [p] blocks of column-major matrices (E doubles per element), ld lda, block stride astride
    const double* Br; // [p] blocks of row-major K x ldb planes (re)
    const double* Bi; // (im)
    const int* amap;  // z -> A block, B block, C block
    const int* bmap;
    const int* cmap;
    const int* kend;  // per column: one past its last non-zero row
    double* Cr;       // mode 0: planes [block][crows][ldb] (row i - i0); mode 1: interleaved column-major, ld ldc
    double* Ci;
    const double* sr; // mode 1: per-column factor (or nullptr)
    const double* si;
    const int* ocol;  // mode 1: output column of solve column c; pair[c]: also write the conjugate at ocol + 1
    const int* pair;
    size_t astride, bstride, cstride;
    int lda, ldb, ldc;
    int i0, M;        // rows i0 .. i0 + M - 1 of A
    int kbeg;         // K starts here (the rows above are not part of the product)
    int jlo, ncol;    // columns jlo .. ncol - 1
    int mode;
    int crows;
};

template <bool CPLX>
PSD_HD double psd_ev_ld(const double* a, size_t o, double& im) {
    if (CPLX) {
        im = a[2 * o + 1];
        return a[2 * o];
    }
    im = 0.0;
    return a[o];
}

// epilogue of one product element (row i, solve column j): mode 0 stores the planes, mode 1 the interleaved output
PSD_HD void psd_ev_store(const psd_ev_gemm_args& g, int z, int i, int j, double vr, double vi) {
    if (g.mode == 0) {
        const size_t o = g.cmap[z] * g.cstride + (size_t)(i - g.i0) * g.ldb + j;
        g.Cr[o] = vr;
        g.Ci[o] = vi;
        return;
    }
    if (g.sr) {
        const double a = g.sr[j], b = g.si[j];
        const double wr = a * vr - b * vi, wi = a * vi + b * vr;
        vr = wr;
        vi = wi;
    }
    double* C = g.Cr + g.cmap[z] * g.cstride;
    const size_t o = (size_t)g.ocol[j] * g.ldc + i;
    C[2 * o] = vr;
    C[2 * o + 1] = vi;
    if (g.pair[j]) {
        C[2 * (o + g.ldc)] = vr;
        C[2 * (o + g.ldc) + 1] = -vi;
    }
}

#ifndef PSD_HOSTSIM
typedef double psd_ev_d4 __attribute__((ext_vector_type(4)));

// C(32 x 64 tile) = A(i0.., K) B(K, cols), grid (row tiles, column panels, factors), 256 threads: wave w computes rows
// 16 (w & 1) and columns 32 (w >> 1) of the tile (two 16 x 16 MFMA tiles), operands staged through LDS in K steps of 16.
template <bool CPLX>
__global__ void __launch_bounds__(256) psd_ev_gemm(psd_ev_gemm_args g) {
    constexpr int E = CPLX ? 2 : 1;
    __shared__ double As[E][PSD_EV_TK][PSD_EV_RB + 1];
    __shared__ double Bs[2][PSD_EV_TK][PSD_EV_TN + 1];
    const int z = blockIdx.z;
    const int ti = blockIdx.x * PSD_EV_RB, tj = g.jlo + blockIdx.y * PSD_EV_TN;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wi = (wave & 1) * 16, wj = (wave >> 1) * 32;
    const int jlast = min(tj + PSD_EV_TN, g.ncol) - 1;
    const int kend = g.kend[jlast];  // columns sorted by their own row: the last one of the panel ends lowest
    const double* A = g.A + g.amap[z] * g.astride;
    const double* Br = g.Br + g.bmap[z] * g.bstride;
    const double* Bi = g.Bi + g.bmap[z] * g.bstride;
    psd_ev_d4 cr[2], ci[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        cr[b] = psd_ev_d4{0.0, 0.0, 0.0, 0.0};
        ci[b] = psd_ev_d4{0.0, 0.0, 0.0, 0.0};
    }
    for (int k0 = g.kbeg; k0 < kend; k0 += PSD_EV_TK) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {  // A(i0 + ti + i, k0 + k): 32 x 16, contiguous in i
            const int e = tid + 256 * q, i = e & 31, k = e >> 5;
            double re = 0.0, im = 0.0;
            if (ti + i < g.M && k0 + k < kend)
                re = psd_ev_ld<CPLX>(A, (size_t)(k0 + k) * g.lda + g.i0 + ti + i, im);
            As[0][k][i] = re;
            if (CPLX) As[E - 1][k][i] = im;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // B(k0 + k, tj + j): 16 x 64, contiguous in j
            const int e = tid + 256 * q, j = e & 63, k = e >> 6;
            double re = 0.0, im = 0.0;
            if (tj + j < g.ncol && k0 + k < kend) {
                const size_t o = (size_t)(k0 + k) * g.ldb + tj + j;
                re = Br[o];
                im = Bi[o];
            }
            Bs[0][k][j] = re;
            Bs[1][k][j] = im;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < PSD_EV_TK; kk += 4) {
            const int kr = kk + (lane >> 4), col = lane & 15;
            const double ar = As[0][kr][wi + col];
            const double ai = CPLX ? As[E - 1][kr][wi + col] : 0.0;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const double br = Bs[0][kr][wj + 16 * b + col], bi = Bs[1][kr][wj + 16 * b + col];
                cr[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, cr[b], 0, 0, 0);
                ci[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ci[b], 0, 0, 0);
                if (CPLX) {
                    cr[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, bi, cr[b], 0, 0, 0);
                    ci[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ci[b], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // C/D fragment of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = ti + wi + (lane >> 4) + 4 * r, j = tj + wj + 16 * b + (lane & 15);
            if (i < g.M && j < g.ncol) psd_ev_store(g, z, g.i0 + i, j, cr[b][r], ci[b][r]);
        }
}
#else
// test-tier stand-in for the matrix-core kernel: the same products in plain loops (K ascending)
template <bool CPLX>
static void psd_ev_gemm_sim(const psd_ev_gemm_args& g, int nz) {
    for (int z = 0; z < nz; ++z) {
        const double* A = g.A + g.amap[z] * g.astride;
        const double* Br = g.Br + g.bmap[z] * g.bstride;
        const double* Bi = g.Bi + g.bmap[z] * g.bstride;
        for (int tj = g.jlo; tj < g.ncol; tj += PSD_EV_TN) {
            const int jend = tj + PSD_EV_TN < g.ncol ? tj + PSD_EV_TN : g.ncol;
            const int kend = g.kend[jend - 1];
            for (int j = tj; j < jend; ++j)
                for (int i = 0; i < g.M; ++i) {
                    double vr = 0.0, vi = 0.0;
                    for (int k = g.kbeg; k < kend; ++k) {
                        double ai;
                        const double ar = psd_ev_ld<CPLX>(A, (size_t)k * g.lda + g.i0 + i, ai);
                        const size_t o = (size_t)k * g.ldb + j;
                        vr += ar * Br[o] - ai * Bi[o];
                        vi += ar * Bi[o] + ai * Br[o];
                    }
                    psd_ev_store(g, z, g.i0 + i, j, vr, vi);
                }
        }
    }
}
#endif

struct psd_ev_args {
    const double* T;   // [p][n][n] user order
    const int* wmap;   // working factor j -> block of T
    const int* bsz;    // per row: 1, 2 (first row of a 2x2 block of the quasi-triangular factor), 0 (its second row)
    const int* k0;     // per column: first row of the own block
    const int* m;      // size of the own block
    const int* kend;   // k0 + m
    const double* mu;  // per column (re, im): mu = lambda^(1/p)
    const double* lam; // per column: lambda
    const double* ev;  // per row: the eigenvalue of the row's 1x1 block (re, im)
    double* Xr;        // [p][n][ns]
    double* Xi;
    double* Rr;        // [p][PSD_EV_RB][ns]
    double* Ri;
    int* cnt;          // per column: [3]: perturbed pivots, rescalings, zero eigenvalue
    int n, p, ns, six, r0, r1, jlo;
};

template <bool CPLX>
struct psd_ev_col {
    const psd_ev_args& a;
    int j;
    size_t nn;
    PSD_HD psd_ev_col(const psd_ev_args& a_, int j_) : a(a_), j(j_), nn((size_t)a_.n * a_.n) {}
    // W_l(i, k), upper part only (the sub-diagonal of the quasi-triangular factor through D)
    PSD_HD psd_z w(int l, int i, int k) const {
        double im;
        const double re = psd_ev_ld<CPLX>(a.T + (size_t)a.wmap[l] * nn * (CPLX ? 2 : 1), (size_t)k * a.n + i, im);
        return zmk(re, im);
    }
    PSD_HD size_t xo(int l, int i) const { return ((size_t)l * a.n + i) * a.ns + j; }
    PSD_HD psd_z x(int l, int i) const { return zmk(a.Xr[xo(l, i)], a.Xi[xo(l, i)]); }
    PSD_HD void setx(int l, int i, psd_z v) const {
        a.Xr[xo(l, i)] = v.re;
        a.Xi[xo(l, i)] = v.im;
    }
    PSD_HD size_t ro(int l, int i) const { return ((size_t)l * PSD_EV_RB + (i - a.r0)) * a.ns + j; }
    PSD_HD psd_z r(int l, int i) const { return zmk(a.Rr[ro(l, i)], a.Ri[ro(l, i)]); }
    PSD_HD void setr(int l, int i, psd_z v) const {
        a.Rr[ro(l, i)] = v.re;
        a.Ri[ro(l, i)] = v.im;
    }
    // D_l of the row block (i, b): the 2x2 block is full only in the quasi-triangular factor
    PSD_HD void d(int l, int i, int b, psd_z D[2][2]) const {
        D[0][0] = w(l, i, i);
        D[0][1] = D[1][0] = D[1][1] = zmk(0.0, 0.0);
        if (b == 2) {
            D[0][1] = w(l, i, i + 1);
            D[1][1] = w(l, i + 1, i + 1);
            D[1][0] = (l == a.six) ? w(l, i + 1, i) : zmk(0.0, 0.0);
        }
    }
    // factors lo .. hi-1 of the column (rows xlo .. kend-1, the chunk's pending R rows r0 .. rhi-1) times 2^-s
    PSD_HD void rescale(int lo, int hi, int xlo, int rhi, int s) const {
        const int ke = a.kend[j];
        for (int l = lo; l < hi; ++l) {
            for (int i = xlo; i < ke; ++i) setx(l, i, zscal(ldexp(1.0, -s), x(l, i)));
            for (int i = a.r0; i < rhi; ++i) setr(l, i, zscal(ldexp(1.0, -s), r(l, i)));
        }
    }
};

// (M) y = c for a complex 2x2 M by complete pivoting (xLALN2); pivots below smin are replaced by smin
PSD_HD int psd_ev_solve2(psd_z M[2][2], psd_z c[2], double smin, psd_z y[2]) {
    int pi = 0, pj = 0;
    double best = -1.0;
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 2; ++k)
            if (zabs1(M[i][k]) > best) {
                best = zabs1(M[i][k]);
                pi = i;
                pj = k;
            }
    int np = 0;
    psd_z u11 = M[pi][pj];
    if (zabs(u11) < smin) {
        u11 = zmk(smin, 0.0);
        ++np;
    }
    const int qi = 1 - pi, qj = 1 - pj;
    const psd_z l21 = zdiv(M[qi][pj], u11);
    const psd_z u12 = M[pi][qj];
    psd_z u22 = zsub(M[qi][qj], zmul(l21, u12));
    if (zabs(u22) < smin) {
        u22 = zmk(smin, 0.0);
        ++np;
    }
    const psd_z c2 = zsub(c[qi], zmul(l21, c[pi]));
    const psd_z yq = zdiv(c2, u22);
    const psd_z yp = zdiv(zsub(c[pi], zmul(u12, yq)), u11);
    y[pj] = yp;
    y[qj] = yq;
    return np;
}

// The cyclic recurrence of one row block, y_{l+1} = A_l y_l + c_l with A_l = D_l / mu, c_l = r_l / mu, is a chain of
// affine maps.  A map is kept as 2^s (A x + c) with A, c normalised, so that products over many factors neither overflow
// nor underflow; a vector with its exponent is the map with A = 0.  Composition is associative: the wavefront of a column
// composes the maps by a scan over its lanes (each lane a contiguous segment of factors) instead of walking the factors
// one after the other.
struct psd_ev_map {
    psd_z A[2][2];
    psd_z c[2];
    int s;
};

PSD_HD void psd_ev_mnorm(psd_ev_map& m) {
    double mx = 0.0;
    for (int i = 0; i < 2; ++i) {
        mx = fmax(mx, zabs1(m.c[i]));
        for (int k = 0; k < 2; ++k) mx = fmax(mx, zabs1(m.A[i][k]));
    }
    if (mx > 0.0 && mx < INFINITY && (mx > 0x1p64 || mx < 0x1p-64)) {
        const int e = ilogb(mx);
        const double f = ldexp(1.0, -e);
        for (int i = 0; i < 2; ++i) {
            m.c[i] = zscal(f, m.c[i]);
            for (int k = 0; k < 2; ++k) m.A[i][k] = zscal(f, m.A[i][k]);
        }
        m.s += e;
    }
}

PSD_HD psd_ev_map psd_ev_ident() {
    psd_ev_map m;
    for (int i = 0; i < 2; ++i) {
        m.c[i] = zmk(0.0, 0.0);
        for (int k = 0; k < 2; ++k) m.A[i][k] = zmk(i == k ? 1.0 : 0.0, 0.0);
    }
    m.s = 0;
    return m;
}

// m2 after m1: 2^(s2 + t) (A2 A1 2^(s1 - t) x + A2 c1 2^(s1 - t) + c2 2^-t), t = max(s1, 0): no factor above 1
PSD_HD psd_ev_map psd_ev_compose(const psd_ev_map& m2, const psd_ev_map& m1) {
    const int t = m1.s > 0 ? m1.s : 0;
    const double f = ldexp(1.0, m1.s - t), g = ldexp(1.0, -t);
    psd_ev_map r;
    for (int i = 0; i < 2; ++i) {
        for (int k = 0; k < 2; ++k)
            r.A[i][k] = zscal(f, zadd(zmul(m2.A[i][0], m1.A[0][k]), zmul(m2.A[i][1], m1.A[1][k])));
        r.c[i] = zadd(zscal(f, zadd(zmul(m2.A[i][0], m1.c[0]), zmul(m2.A[i][1], m1.c[1]))), zscal(g, m2.c[i]));
    }
    r.s = m2.s + t;
    psd_ev_mnorm(r);
    return r;
}

// a vector (b entries) with exponent e as a map
PSD_HD psd_ev_map psd_ev_vec(const psd_z* y, int b, int e) {
    psd_ev_map v = psd_ev_ident();
    v.A[0][0] = v.A[1][1] = zmk(0.0, 0.0);
    for (int q = 0; q < b; ++q) v.c[q] = y[q];
    v.s = e;
    psd_ev_mnorm(v);
    return v;
}

// log2 of the largest entry of a vector-map (a very small number for zero)
PSD_HD int psd_ev_vexp(const psd_ev_map& v) {
    const double mx = fmax(zabs1(v.c[0]), zabs1(v.c[1]));
    return mx > 0.0 ? v.s + ilogb(mx) : -100000;
}

// the factors of lane t: a contiguous segment [lo, hi) of the p factors
PSD_HD void psd_ev_seg(int t, int p, int& lo, int& hi) {
    const int L = (p + 63) / 64;
    lo = t * L < p ? t * L : p;
    hi = lo + L < p ? lo + L : p;
}

// y_0(I) of one row block from the total map round the period, y_0 = G y_0 + c with G = 2^S A, c = 2^S c: the own block's
// null vector (b == 2) or unit (b == 1), else the solve with the pivot rule above.  y: b entries, e0 its exponent; returns
// the number of perturbed pivots.  ev: the eigenvalues of the rows (re, im), lam the column's.
PSD_HD int psd_ev_y0(const psd_ev_map& tot, bool isown, int b, int i, psd_z lam, const double* ev, psd_z y[2], int& e0) {
    y[0] = zmk(1.0, 0.0);
    y[1] = zmk(0.0, 0.0);
    e0 = 0;
    int npert = 0;
    const double eps = PSD_DBL_EPS, tiny = PSD_DBL_MIN;
    const double sI = tot.s > 0 ? ldexp(1.0, -tot.s) : 1.0, sG = tot.s > 0 ? 1.0 : ldexp(1.0, tot.s);
    if (isown && b == 2) {  // the null vector of G - I, up to the power of two: (N01, -N00) or (N11, -N10)
        psd_z N[2][2];
        for (int q = 0; q < 2; ++q)
            for (int k = 0; k < 2; ++k) N[q][k] = zsub(zscal(sG, tot.A[q][k]), zmk(q == k ? sI : 0.0, 0.0));
        const bool first = zabs2(N[0][1]) + zabs2(N[0][0]) >= zabs2(N[1][1]) + zabs2(N[1][0]);
        y[0] = first ? N[0][1] : N[1][1];
        y[1] = first ? zneg(N[0][0]) : zneg(N[1][0]);
        if (ziszero(y[0]) && ziszero(y[1])) y[0] = zmk(1.0, 0.0);
    } else if (!isown && b == 1) {
        const psd_z li = zmk(ev[2 * i], ev[2 * i + 1]);
        psd_z d1 = zdiv(zsub(lam, li), lam);  // 1 - G = (lambda - lambda_i) / lambda
        const double smin = fmax(eps * fmax(1.0, zabs(d1)), tiny);
        if (!(zabs(d1) >= smin)) {
            d1 = zmk(smin, 0.0);
            ++npert;
        }
        y[0] = zdiv(tot.c[0], d1);
        e0 = tot.s;
    } else if (!isown) {  // 2^S > 1: (2^-S I - A) y = c; else (I - 2^S A) y = c and y_0 = 2^S y
        psd_z M[2][2], cc[2];
        double mx = 0.0;
        for (int q = 0; q < 2; ++q) {
            for (int k = 0; k < 2; ++k) {
                M[q][k] = zsub(zmk(q == k ? sI : 0.0, 0.0), zscal(sG, tot.A[q][k]));
                mx = fmax(mx, zabs(M[q][k]));
            }
            cc[q] = tot.c[q];
        }
        npert += psd_ev_solve2(M, cc, fmax(eps * fmax(sI, mx), tiny), y);
        e0 = tot.s > 0 ? 0 : tot.s;
    }
    return npert;
}

// the power of two a column is scaled down by once its largest entry reaches 2^big
PSD_HD int psd_ev_shift(int big) { return big > PSD_EV_BIG ? big - 200 : 0; }

#define PSD_EV_LDS (2 * 64 * sizeof(psd_ev_map) + 64 * sizeof(int))

// One workgroup (one wavefront) per column of [jlo, ns): the rows of the chunk [r0, r1), bottom up.  Every factor l is
// owned by one lane (psd_ev_seg) in every region, so its X and R entries are only ever touched by that lane.
template <bool CPLX>
PSD_D void psd_ev_solve_body(const psd_ev_args& a) {
    PSD_LDS_DECL;
    psd_ev_map* buf = (psd_ev_map*)psd_lds;  // [2][64]
    int* red = (int*)(buf + 128);
    const int j = a.jlo + PSD_BLOCK_X;
    psd_ev_col<CPLX> col(a, j);
    const int kk = a.k0[j], mm = a.m[j], ke = a.kend[j], p = a.p;
    const psd_z mu = zmk(a.mu[2 * j], a.mu[2 * j + 1]);
    const psd_z lam = zmk(a.lam[2 * j], a.lam[2 * j + 1]);
    if (kk < a.r0) return;
    if (ziszero(mu)) {  // the recurrence divides by mu: the column is returned as NaN
        PSD_ONE {
            if (kk < a.r1) a.cnt[3 * j + 2] = 1;
        }
        return;
    }
    const psd_z rmu = zdiv(zmk(1.0, 0.0), mu);
    const bool own = kk < a.r1;
    int i1 = own ? kk + mm : a.r1;  // rows >= i1 of this chunk are done
    while (i1 > a.r0) {
        const bool isown = own && i1 == kk + mm;
        const int b = isown ? mm : ((a.bsz[i1 - 1] == 0) ? 2 : 1);
        const int i = i1 - b;
        const int kin = ke < a.r1 ? ke : a.r1;
        // r_l(I) = R_l(I) + the rows of the chunk below I (kept in R), the maps of the factors, composed per segment
        PSD_PAR_FOR(t, 64) {
            int lo, hi;
            psd_ev_seg(t, p, lo, hi);
            psd_ev_map seg = psd_ev_ident();
            for (int l = lo; l < hi; ++l) {
                psd_ev_map m = psd_ev_ident();
                psd_z D[2][2];
                col.d(l, i, b, D);
                for (int q = 0; q < 2; ++q)
                    for (int k = 0; k < 2; ++k) m.A[q][k] = (q < b && k < b) ? zmul(D[q][k], rmu) : zmk(0.0, 0.0);
                if (!isown)
                    for (int q = 0; q < b; ++q) {
                        psd_z s = col.r(l, i + q);
                        for (int k = i1; k < kin; ++k) s = zadd(s, zmul(col.w(l, i + q, k), col.x(l, k)));
                        col.setr(l, i + q, s);
                        m.c[q] = zmul(s, rmu);
                    }
                psd_ev_mnorm(m);
                seg = psd_ev_compose(m, seg);
            }
            buf[t] = seg;
        }
        PSD_SYNC();
        // inclusive scan over the lanes (Hillis-Steele, fixed order): buf[t] = segment t after ... after segment 0
        int cur = 0;
        for (int d = 1; d < 64; d <<= 1) {
            PSD_PAR_FOR(t, 64) {
                buf[64 * (1 - cur) + t] = t >= d ? psd_ev_compose(buf[64 * cur + t], buf[64 * cur + t - d])
                                                 : buf[64 * cur + t];
            }
            PSD_SYNC();
            cur = 1 - cur;
        }
        psd_ev_map* inc = buf + 64 * cur;
        // y_0(I): round the period, y_0 = G y_0 + c with G = 2^S A, c = 2^S c of the total map
        const psd_ev_map tot = inc[63];
        psd_z y[2];
        int e0;
        const int npert = psd_ev_y0(tot, isown, b, i, lam, a.ev, y, e0);
        PSD_ONE {
            if (npert) a.cnt[3 * j] += npert;
        }
        const psd_ev_map v0 = psd_ev_vec(y, b, e0);
        // the largest entry y_l(I) will have: a column growing past 2^PSD_EV_BIG is scaled down first
        PSD_PAR_FOR(t, 64) {
            int lo, hi;
            psd_ev_seg(t, p, lo, hi);
            psd_ev_map v = t > 0 ? psd_ev_compose(inc[t - 1], v0) : v0;
            int mx = -100000;
            for (int l = lo; l < hi; ++l) {
                const int e = psd_ev_vexp(v);
                mx = e > mx ? e : mx;
                psd_ev_map m = psd_ev_ident();
                psd_z D[2][2];
                col.d(l, i, b, D);
                for (int q = 0; q < 2; ++q)
                    for (int k = 0; k < 2; ++k) m.A[q][k] = (q < b && k < b) ? zmul(D[q][k], rmu) : zmk(0.0, 0.0);
                if (!isown)
                    for (int q = 0; q < b; ++q) m.c[q] = zmul(col.r(l, i + q), rmu);
                psd_ev_mnorm(m);
                v = psd_ev_compose(m, v);
            }
            red[t] = mx;
        }
        PSD_SYNC();
        int big = -100000;
        for (int t = 0; t < 64; ++t) big = red[t] > big ? red[t] : big;
        const int shift = psd_ev_shift(big);
        if (shift) PSD_ONE { a.cnt[3 * j + 1] += 1; }
        // store y_l(I) scaled by 2^-shift, as the rows below and the pending R rows of the chunk are (the maps stay in
        // the old scale: only the stored values move)
        PSD_PAR_FOR(t, 64) {
            int lo, hi;
            psd_ev_seg(t, p, lo, hi);
            if (shift) col.rescale(lo, hi, i1, i, shift);
            psd_ev_map v = t > 0 ? psd_ev_compose(inc[t - 1], v0) : v0;
            for (int l = lo; l < hi; ++l) {
                for (int q = 0; q < b; ++q) col.setx(l, i + q, zscal(ldexp(1.0, v.s - shift), v.c[q]));
                psd_ev_map m = psd_ev_ident();
                psd_z D[2][2];
                col.d(l, i, b, D);
                for (int q = 0; q < 2; ++q)
                    for (int k = 0; k < 2; ++k) m.A[q][k] = (q < b && k < b) ? zmul(D[q][k], rmu) : zmk(0.0, 0.0);
                if (!isown)
                    for (int q = 0; q < b; ++q) m.c[q] = zmul(col.r(l, i + q), rmu);
                psd_ev_mnorm(m);
                v = psd_ev_compose(m, v);
            }
        }
        PSD_SYNC();
        i1 = i;
    }
}
PSD_KERNEL psd_ev_solve_d(psd_ev_args a) { psd_ev_solve_body<false>(a); }
PSD_KERNEL psd_ev_solve_z(psd_ev_args a) { psd_ev_solve_body<true>(a); }

// the sub-diagonal of the quasi-triangular factor (real decompositions): defines the 2x2 row blocks
PSD_KERNEL psd_ev_subdiag(const double* T, int n, double* out) {
    PSD_PAR_FOR(t, PSD_NTHREADS) {
        const int i = PSD_BLOCK_X * PSD_NTHREADS + t;
        if (i < n - 1) out[i] = T[(size_t)i * n + i + 1];
    }
}

// one solve column of psd_ev_norm: v its n entries (interleaved; the partner's n behind them), zero: a zero eigenvalue
PSD_HD void psd_ev_norm_col(double* v, int n, bool pair, bool zero, double& sr, double& si) {
    if (zero) {  // (the other factors follow from s = NaN)
        for (int i = 0; i < (pair ? 2 * n : n); ++i) v[2 * i] = v[2 * i + 1] = NAN;
        sr = si = NAN;
    } else {
        double big = 0.0;
        int imax = 0;
        for (int i = 0; i < n; ++i) big = fmax(big, zabs1(zmk(v[2 * i], v[2 * i + 1])));
        double ss = 0.0, amax = -1.0;
        for (int i = 0; i < n; ++i) {  // (scaled by the largest component: no overflow in the sum of squares)
            const double a2 = zabs2(zscal(1.0 / big, zmk(v[2 * i], v[2 * i + 1])));
            ss += a2;
            if (a2 > amax) {
                amax = a2;
                imax = i;
            }
        }
        const double nrm = big * sqrt(ss), am = big * sqrt(amax);
        const psd_z s = zscal(1.0 / (am * nrm), zconj(zmk(v[2 * imax], v[2 * imax + 1])));
        for (int i = 0; i < n; ++i) {
            psd_z u = zmul(s, zmk(v[2 * i], v[2 * i + 1]));
            if (i == imax) u = zmk(am / nrm, 0.0);
            v[2 * i] = u.re;
            v[2 * i + 1] = u.im;
            if (pair) {
                v[2 * ((size_t)n + i)] = u.re;
                v[2 * ((size_t)n + i) + 1] = -u.im;
            }
        }
        sr = s.re;
        si = s.im;
    }
}

// ||V_1(:, c)||_2 and the phase: the largest-modulus entry (lowest row on a tie) becomes real and positive.  One lane
// per solve column; s = conj(v_max) / (|v_max| ||v||) goes to sr/si for the other factors; V_1 is scaled here (and the
// conjugate partner rewritten).  A zero-eigenvalue column is set to NaN.
PSD_KERNEL psd_ev_norm(double* V, int n, int ns, const int* ocol, const int* pair,
                       const int* cnt, double* sr, double* si) {
    PSD_PAR_FOR(t, PSD_NTHREADS) {
        const int j = PSD_BLOCK_X * PSD_NTHREADS + t;
        if (j < ns) {
            psd_ev_norm_col(V + 2 * (size_t)ocol[j] * n, n, pair[j] != 0, cnt[3 * j + 2] != 0, sr[j], si[j]);
        }
    }
}
