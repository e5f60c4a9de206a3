// LEFT eigenvectors and eigenvalue condition numbers of many small periodic Schur decompositions (the side = 'L' of
// xTREVC and the S of xTRSNA, in periodic form), for the batches of psd_bevec.h / psd_zbevec.h.  The host drivers are in
// psd_bevec_host.inl and psd_zbevec_host.inl (the left entries) and psd_lbevec_host.inl (the condition numbers).
//
// Left vectors need no second solver.  With the caller's form A_l = Z_{l+1} T_l Z_l^H (orient 'L'; 'R' alike with the
// roles of l and l + 1 exchanged) the left relation w_{l+1}^H A_l = mu w_l^H reads A_l^H w_{l+1} = conj(mu) w_l: the RIGHT
// relation of the factors A_l^H in the opposite orientation, of which
//     T'_l = J T_l^H J,   Z'_l = Z_l J        (J: the reversal permutation)
// is a periodic Schur form with the same factor indexing and the same schurindex: upper (quasi-)triangular, the 2x2
// blocks still standardised, the eigenvalues conjugated and reversed.  psd_lbev_flip writes T' and Z' of a group into
// workspace (the caller's buffers are never written); the solve, the back-transform and the normalisation of psd_bevec.h
// then run on them unchanged, with tables the host builds for the flipped form (rows and selection reversed, eigenvalues
// conjugated, roots conj(psd_ev_root(lambda)) so that the vectors belong to the caller's root).  Their columns come out
// in the flipped order, which is exactly the caller's order reversed, inside conjugate pairs too: psd_lbev_reverse turns
// the nvec columns of every block round in place.
//
// psd_bev_cond: s[q][j][l], the reciprocal condition number of eigenvalue j with respect to factor l, from the right and
// left vectors of every factor.  One wavefront per (problem, column); every sum runs in a fixed order (a lane's stride
// over the rows ascending, then the halving tree over the lanes), no atomics: s does not depend on the batch, bit for bit.
#pragma once
#include "psd_bevec.h"

#define PSD_LBEV_TILE 32  // the flip works on 32 x 32 tiles, 256 threads
#define PSD_LBEV_LDS(cplx) (sizeof(double) * ((cplx) ? 2 : 1) * PSD_LBEV_TILE * (PSD_LBEV_TILE + 1))
#define PSD_LBEV_TILES_MAX 1024  // most workgroups per matrix (larger orders: a workgroup takes several tiles)

// F_m = J T_m^H J for the matrices m < nmat of T, F_{nmat + m} = Z_m J for those of Z (n x n column-major blocks, E doubles
// per element): grid (2 nmat, tiles), PSD_BEV_NT threads.  The flip-adjoint is F(r, c) = conj(T(n-1-c, n-1-r)): a tile is
// read along the source's columns into LDS (padded rows: no bank conflicts on the transposed read) and written along F's
// columns, so both sides are contiguous.  Z J reverses columns only and needs no tile.
template <bool CPLX>
PSD_D void psd_lbev_flip_body(const double* T, const double* Z, double* F, int n, int nmat) {
    PSD_LDS_DECL;
    constexpr int E = CPLX ? 2 : 1, TS = PSD_LBEV_TILE, LD = PSD_LBEV_TILE + 1;
    double* tile = (double*)psd_lds;  // [TS][LD] elements of E doubles
    const int m = PSD_BLOCK_X, nt = (n + TS - 1) / TS;
    const size_t nn = (size_t)n * n * E;
    const bool adj = m < nmat;
    const double* S = adj ? T + (size_t)m * nn : Z + (size_t)(m - nmat) * nn;
    double* D = F + (size_t)m * nn;
    for (int tl = PSD_BLOCK_Y; tl < nt * nt; tl += PSD_GRID_Y) {
        const int r0 = (tl % nt) * TS, c0 = (tl / nt) * TS;
        if (!adj) {
            PSD_PAR_FOR(t, TS * TS) {
                const int r = r0 + t % TS, c = c0 + t / TS;
                if (r < n && c < n)
                    for (int e = 0; e < E; ++e) D[((size_t)c * n + r) * E + e] = S[((size_t)(n - 1 - c) * n + r) * E + e];
            }
            continue;
        }
        // tile[ty][tx] = T(n-1-(c0+tx), n-1-(r0+ty)) = conj(F(r0+ty, c0+tx))
        PSD_PAR_FOR(t, TS * TS) {
            const int tx = t % TS, ty = t / TS;
            if (c0 + tx < n && r0 + ty < n)
                for (int e = 0; e < E; ++e)
                    tile[((size_t)ty * LD + tx) * E + e] = S[((size_t)(n - 1 - r0 - ty) * n + (n - 1 - c0 - tx)) * E + e];
        }
        PSD_SYNC();
        PSD_PAR_FOR(t, TS * TS) {
            const int tx = t % TS, ty = t / TS;
            if (r0 + tx < n && c0 + ty < n) {
                const size_t o = ((size_t)(c0 + ty) * n + r0 + tx) * E, s = ((size_t)tx * LD + ty) * E;
                D[o] = tile[s];
                if (CPLX) D[o + 1] = -tile[s + 1];
            }
        }
        PSD_SYNC();  // (the tile is reused)
    }
}

PSD_KERNEL_B(PSD_BEV_NT) psd_lbev_flip(const double* T, const double* Z, double* F, int n, int nmat) {
    psd_lbev_flip_body<false>(T, Z, F, n, nmat);
}
PSD_KERNEL_B(PSD_BEV_NT) psd_zlbev_flip(const double* T, const double* Z, double* F, int n, int nmat) {
    psd_lbev_flip_body<true>(T, Z, F, n, nmat);
}

// the first nvec[q] columns of every block of V [gc][nmat][maxvec][n] complex turned round in place: column j <-> column
// nvec[q] - 1 - j.  Grid (gc * nmat, tiles of PSD_NTHREADS pairs of elements)
PSD_KERNEL psd_lbev_reverse(double* V, const int* nvec, int n, int nmat, int maxvec) {
    const int b = PSD_BLOCK_X, nv = nvec[b / nmat], half = nv / 2;
    double* B = V + (size_t)b * 2 * n * maxvec;
    for (int e0 = PSD_BLOCK_Y * PSD_NTHREADS; e0 < half * n; e0 += PSD_GRID_Y * PSD_NTHREADS) {
        PSD_PAR_FOR(t, PSD_NTHREADS) {
            const int e = e0 + t;
            if (e < half * n) {
                const int j = e / n, i = e - j * n;
                const size_t a = 2 * ((size_t)j * n + i), c = 2 * ((size_t)(nv - 1 - j) * n + i);
                const double ar = B[a], ai = B[a + 1];
                B[a] = B[c];
                B[a + 1] = B[c + 1];
                B[c] = ar;
                B[c + 1] = ai;
            }
        }
    }
}

struct psd_bev_cond_args {
    const double* V;   // [nb][p][maxvec][n] complex interleaved: the right vectors of every factor
    const double* W;   // the left vectors, likewise
    const int* nvec;   // [nb]
    double* s;         // [nb][maxvec][p]
    int n, p, maxvec, left;
};

#define PSD_BEV_COND_LDS (4 * 64 * sizeof(double))

// left:  s[l] = |w_l^H v_l| / (||w_{l+1}|| ||v_l||);  right:  s[l] = |w_l^H v_l| / (||w_l|| ||v_{l+1}||)  (l + 1 cyclic).
// Grid nb * maxvec, one wavefront each; the columns at and beyond nvec[q] get zeros
PSD_KERNEL_B(64) psd_bev_cond(psd_bev_cond_args g) {
    PSD_LDS_DECL;
    double* red = (double*)psd_lds;  // [4][64]: re, im of w^H v, ||w||^2, ||v||^2
    const int n = g.n, p = g.p, q = PSD_BLOCK_X / g.maxvec, j = PSD_BLOCK_X - q * g.maxvec;
    double* out = g.s + ((size_t)q * g.maxvec + j) * p;
    if (j >= g.nvec[q]) {
        PSD_PAR_FOR(l, p) out[l] = 0.0;
        return;
    }
    const size_t blk = 2 * (size_t)n * g.maxvec;
    const double* Vq = g.V + (size_t)q * p * blk + 2 * (size_t)j * n;
    const double* Wq = g.W + (size_t)q * p * blk + 2 * (size_t)j * n;
    for (int l = 0; l < p; ++l) {
        const int l1 = l + 1 < p ? l + 1 : 0;
        const double* v = Vq + (size_t)l * blk;
        const double* w = Wq + (size_t)l * blk;
        const double* wn = Wq + (size_t)(g.left ? l1 : l) * blk;  // the vectors of the two norms
        const double* vn = Vq + (size_t)(g.left ? l : l1) * blk;
        PSD_PAR_FOR(t, 64) {
            double dr = 0.0, di = 0.0, ww = 0.0, vv = 0.0;
            for (int i = t; i < n; i += 64) {
                const psd_z d = zmul(zconj(zmk(w[2 * i], w[2 * i + 1])), zmk(v[2 * i], v[2 * i + 1]));
                dr += d.re;
                di += d.im;
                ww += zabs2(zmk(wn[2 * i], wn[2 * i + 1]));
                vv += zabs2(zmk(vn[2 * i], vn[2 * i + 1]));
            }
            red[t] = dr;
            red[64 + t] = di;
            red[128 + t] = ww;
            red[192 + t] = vv;
        }
        PSD_SYNC();
        for (int h = 32; h > 0; h >>= 1) {
            PSD_PAR_FOR(t, h) {
                for (int k = 0; k < 4; ++k) red[64 * k + t] += red[64 * k + t + h];
            }
            PSD_SYNC();
        }
        PSD_ONE { out[l] = hypot(red[0], red[64]) / (sqrt(red[128]) * sqrt(red[192])); }
        PSD_SYNC();
    }
}
