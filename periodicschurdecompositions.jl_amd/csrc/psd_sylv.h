// Periodic Sylvester solve for ONE periodic Schur form of any order: the single-problem path of the family of
// psd_bsylv.h (whose batch kernel stops at PSD_BSYL_NMAX).  The host driver is psd_sylv_host.inl.
//
// The rows of T11 and the columns of T22 are cut at multiples of a tile width t; a boundary that would cut a 2x2 block
// of the quasi-triangular factor moves down by one (the host reads that factor's sub-diagonal once, psd_syl_subdiag).
// The tiles (I, J) of X with (nI - 1 - I) + J = d (S^H: I + (nJ - 1 - J) = d) are independent of each other: anti-diagonal
// d of the walk.  Per anti-diagonal two launches:
//   psd_syl_update<CPLX>  grid (tiles of the anti-diagonal x sub-blocks, p), 256 threads.  Left-looking: the right-hand
//                         side of equation e on tile (I, J) receives
//                             C_e[I, J] += - sum_{I' after I} A_e[I, I'] Xa[I', J] + sum_{J' before J} Xb[I, J'] B_e[J', J]
//                         (S^H: the rows before I, the columns after J, the factors conjugate-transposed), the factors
//                         and unknowns of equation e as psd_bsyl_equation names them.  One workgroup owns a 32 x 32
//                         sub-block of one C tile and writes it once; its four wavefronts own a 16 x 16 fragment each
//                         (v_mfma_f64_16x16x4_f64, the fragment maps of psd_ck_gemm).  K runs ascending in steps of 16
//                         over the first sum, then over the second, into one accumulator, which is added to C at the
//                         end: no atomics, no read-modify-write between workgroups, the bits do not depend on the
//                         schedule.  Operands go through LDS rows of 48 doubles (consecutive k rows of a fragment read
//                         fall into the two halves of the banks), zero-filled beyond the ragged edges; the staging
//                         loop runs along whichever index is contiguous in global memory.  ComplexF64: four real
//                         products on de-interleaved planes, as psd_ev_gemm.
//   psd_syl_solve<CPLX>   grid (tiles of the anti-diagonal), one wavefront per tile: the body of psd_bsyl_solve on the
//                         tile's row and column range (psd_bsyl_real_range / psd_bsyl_cplx_range), the in-tile sums
//                         over the tile only.  LDS: psd_bsyl_lds_bytes(p).
// A tile that finds its problem singular stores PSD_INFO_SINGULAR in *flag; every later launch of the call reads the word
// first and does nothing.  The host reads it once, at the end, and fills X with NaNs.
//
// Under PSD_HOSTSIM psd_syl_update is a serial body with the same grid, the same operands and K ascending.
#pragma once
#include "psd_bsylv.h"

#define PSD_SYL_TILE 16       // default tile width (profiles/sylv/README.md: not yet the result of a sweep)
#define PSD_SYL_TILE_MIN 2
#define PSD_SYL_TILE_MAX 128  // (PSD_SYL_TILE in the environment: a width in this range, anything else the default)
#define PSD_SYL_UB 32         // update: edge of a workgroup's sub-block of C
#define PSD_SYL_UK 16         // update: K step
#define PSD_SYL_ULD 48        // update: LDS row (48 % 32 == 16)
#define PSD_SYL_NT 256

struct psd_syl_args {
    const double* T;  // [p][n][n] column-major blocks, user order (CPLX: interleaved)
    double* X;        // [p][m k] elements: block l is m x k column-major, ld m
    const int* rb;    // [nI + 1] row boundaries of T11, 0 .. m
    const int* cb;    // [nJ + 1] column boundaries of T22 (local), 0 .. k
    int* flag;        // PSD_INFO_SINGULAR once a tile found the problem singular; never cleared
    int n, p, m, qsub, left, trans, fromT;
    int nI, nJ, d;    // the partition and the anti-diagonal of this launch
    int nsb;          // update: sub-blocks per tile and dimension
};

// tiles on anti-diagonal d, and tile x of it (a counts the block rows in walk order, b the block columns)
PSD_HD int psd_syl_diag_lo(int nJ, int d) { return d - (nJ - 1) > 0 ? d - (nJ - 1) : 0; }
PSD_HD int psd_syl_diag_tiles(int nI, int nJ, int d) {
    const int hi = d < nI - 1 ? d : nI - 1;
    return hi - psd_syl_diag_lo(nJ, d) + 1;
}
PSD_HD void psd_syl_tile_of(const psd_syl_args& g, int x, int& I, int& J) {
    const int a = psd_syl_diag_lo(g.nJ, g.d) + x, b = g.d - a;
    I = g.trans ? a : g.nI - 1 - a;
    J = g.trans ? g.nJ - 1 - b : b;
}

// sub[i] = T_q(i + 1, i), i < n - 1, of the quasi-triangular factor: one block
PSD_KERNEL_B(64) psd_syl_subdiag(const double* Tq, double* sub, int n) {
    PSD_PAR_FOR(i, n - 1) { sub[i] = Tq[(size_t)i * n + i + 1]; }
}

template <bool CPLX>
PSD_KERNEL_B(64) psd_syl_solve(psd_syl_args g) {
    if (psd_atomic_load(g.flag) != 0) return;
    int I, J;
    psd_syl_tile_of(g, PSD_BLOCK_X, I, J);
    const psd_bsyl_range rg{g.rb[I], g.rb[I + 1], g.cb[J], g.cb[J + 1]};
    const size_t xb = (size_t)g.m * (g.n - g.m);
    bool ok;
    if (CPLX) ok = psd_bsyl_cplx_range(g.T, g.X, xb, g.n, g.p, g.m, g.left != 0, g.trans != 0, g.fromT, rg);
    else ok = psd_bsyl_real_range(g.T, g.X, xb, g.n, g.p, g.m, g.qsub, g.left != 0, g.trans != 0, g.fromT, rg);
    if (!ok) {
        PSD_ONE { psd_atomic_store(g.flag, PSD_INFO_SINGULAR); }
    }
}

// The two products of one sub-block of equation e: product s is sum_k L_s(i, k) R_s(k, j), k < klen, with
// L_s(i, k) = (lre, lim) .* L[i lsx + k lsk] and R_s(k, j) = (rre, rim) .* R[j rsx + k rsk] (element strides; the factors
// are the signs of the real and the imaginary part: the minus of the first sum and the conjugates of S^H)
struct psd_syl_prod {
    const double *L, *R;
    size_t lsx, lsk, rsx, rsk;
    int klen;
    double lre, lim, rre, rim;
};
struct psd_syl_block {
    int bi0, bj0, mi, nj;  // first row and (local) column of the sub-block, its extent; mi == 0: nothing to do
    psd_syl_prod pr[2];
};

template <bool CPLX>
PSD_D psd_syl_block psd_syl_block_of(const psd_syl_args& g, int bx, int e) {
    constexpr int E = CPLX ? 2 : 1;
    psd_syl_block b;
    b.mi = 0;
    const int sb = bx % (g.nsb * g.nsb), si = sb % g.nsb, sj = sb / g.nsb;
    int I, J;
    psd_syl_tile_of(g, bx / (g.nsb * g.nsb), I, J);
    const int i0 = g.rb[I], i1 = g.rb[I + 1], j0 = g.cb[J], j1 = g.cb[J + 1];
    b.bi0 = i0 + PSD_SYL_UB * si;
    b.bj0 = j0 + PSD_SYL_UB * sj;
    b.nj = 0;
    if (b.bi0 >= i1 || b.bj0 >= j1) return b;
    b.mi = i1 - b.bi0 < PSD_SYL_UB ? i1 - b.bi0 : PSD_SYL_UB;
    b.nj = j1 - b.bj0 < PSD_SYL_UB ? j1 - b.bj0 : PSD_SYL_UB;
    const int n = g.n, m = g.m, k = n - m;
    const bool trans = g.trans != 0;
    const size_t nn = (size_t)n * n, xb = (size_t)m * k;
    const psd_bsyl_eq eq = psd_bsyl_equation(e, g.p, g.left != 0, trans);
    const double* A = g.T + E * (size_t)eq.fa * nn;
    const double* B = g.T + E * (size_t)eq.fb * nn;
    const double* Xa = g.X + E * (size_t)eq.ua * xb;
    const double* Xb = g.X + E * (size_t)eq.ub * xb;
    // - A[I, rows after I] Xa[rows after I, J]   (S^H: - A[rows before I, I]^H Xa[rows before I, J])
    psd_syl_prod& p0 = b.pr[0];
    const int ka = trans ? 0 : i1;
    p0.klen = trans ? i0 : m - i1;
    if (!trans) {
        p0.L = A + E * ((size_t)ka * n + b.bi0);
        p0.lsx = 1;
        p0.lsk = (size_t)n;
    } else {
        p0.L = A + E * ((size_t)b.bi0 * n + ka);
        p0.lsx = (size_t)n;
        p0.lsk = 1;
    }
    p0.lre = -1.0;
    p0.lim = trans ? 1.0 : -1.0;
    p0.R = Xa + E * ((size_t)b.bj0 * m + ka);
    p0.rsx = (size_t)m;
    p0.rsk = 1;
    p0.rre = p0.rim = 1.0;
    // + Xb[I, columns before J] B[columns before J, J]   (S^H: + Xb[I, columns after J] B[J, columns after J]^H)
    psd_syl_prod& p1 = b.pr[1];
    const int kb = trans ? j1 : 0;
    p1.klen = trans ? k - j1 : j0;
    p1.L = Xb + E * ((size_t)kb * m + b.bi0);
    p1.lsx = 1;
    p1.lsk = (size_t)m;
    p1.lre = p1.lim = 1.0;
    if (!trans) {
        p1.R = B + E * ((size_t)(m + b.bj0) * n + m + kb);
        p1.rsx = (size_t)n;
        p1.rsk = 1;
    } else {
        p1.R = B + E * ((size_t)(m + kb) * n + m + b.bj0);
        p1.rsx = 1;
        p1.rsk = (size_t)n;
    }
    p1.rre = 1.0;
    p1.rim = trans ? -1.0 : 1.0;
    return b;
}

// C_e(i, j) of the sub-block += acc: what was there, or with fromT -T12_e(i, j)
template <bool CPLX>
PSD_D void psd_syl_store(const psd_syl_args& g, int e, int i, int j, double vr, double vi) {
    const size_t o = (size_t)e * g.m * (g.n - g.m) + (size_t)j * g.m + i;
    const size_t ot = (size_t)e * g.n * g.n + (size_t)(g.m + j) * g.n + i;
    if (CPLX) {
        const double cr = g.fromT ? -g.T[2 * ot] : g.X[2 * o], ci = g.fromT ? -g.T[2 * ot + 1] : g.X[2 * o + 1];
        g.X[2 * o] = cr + vr;
        g.X[2 * o + 1] = ci + vi;
    } else {
        const double cr = g.fromT ? -g.T[ot] : g.X[o];
        g.X[o] = cr + vr;
    }
}

#ifndef PSD_HOSTSIM
typedef double psd_syl_d4 __attribute__((ext_vector_type(4)));

// buf[k][x] = sign .* M[x sx + k sk], x < nx, k < nk, zero beyond; planes re | im.  The loop runs along the index that is
// contiguous in global memory (the k-fast form stores with a stride of a row: an eight-way conflict on 1 / 16 of the
// traffic of a K step, against uncoalesced global loads)
template <bool CPLX>
__device__ __forceinline__ void psd_syl_stage(double* buf, const double* M, size_t sx, size_t sk, int nx, int nk, double sre,
                                              double sim) {
    const bool kfast = sk == 1;
    for (int e = threadIdx.x; e < PSD_SYL_UK * PSD_SYL_UB; e += PSD_SYL_NT) {
        const int k = kfast ? e % PSD_SYL_UK : e / PSD_SYL_UB, x = kfast ? e / PSD_SYL_UK : e % PSD_SYL_UB;
        double re = 0.0, im = 0.0;
        if (x < nx && k < nk) {
            const size_t o = (size_t)x * sx + (size_t)k * sk;
            if (CPLX) {
                re = sre * M[2 * o];
                im = sim * M[2 * o + 1];
            } else {
                re = sre * M[o];
            }
        }
        buf[k * PSD_SYL_ULD + x] = re;
        if (CPLX) buf[PSD_SYL_UK * PSD_SYL_ULD + k * PSD_SYL_ULD + x] = im;
    }
}

template <bool CPLX>
__global__ void __launch_bounds__(PSD_SYL_NT) psd_syl_update(psd_syl_args g) {
    constexpr int E = CPLX ? 2 : 1;
    __shared__ double Ls[E * PSD_SYL_UK * PSD_SYL_ULD], Rs[E * PSD_SYL_UK * PSD_SYL_ULD];
    constexpr int plane = PSD_SYL_UK * PSD_SYL_ULD;
    if (psd_atomic_load(g.flag) != 0) return;
    const int e = blockIdx.y;
    const psd_syl_block b = psd_syl_block_of<CPLX>(g, blockIdx.x, e);
    if (b.mi == 0) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int fi = wave & 1, fj = wave >> 1, col = lane & 15, kq = lane >> 4;
    const bool mine = 16 * fi < b.mi && 16 * fj < b.nj;  // (a fragment wholly beyond the edge: the wavefront only stages)
    psd_syl_d4 cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < 2; ++s) {
        const psd_syl_prod& pr = b.pr[s];
        for (int k0 = 0; k0 < pr.klen; k0 += PSD_SYL_UK) {
            psd_syl_stage<CPLX>(Ls, pr.L + E * (size_t)k0 * pr.lsk, pr.lsx, pr.lsk, b.mi, pr.klen - k0, pr.lre, pr.lim);
            psd_syl_stage<CPLX>(Rs, pr.R + E * (size_t)k0 * pr.rsk, pr.rsx, pr.rsk, b.nj, pr.klen - k0, pr.rre, pr.rim);
            __syncthreads();
            if (mine) {
#pragma unroll
                for (int kk = 0; kk < PSD_SYL_UK; kk += 4) {
                    const int lo = (kk + kq) * PSD_SYL_ULD + 16 * fi + col, ro = (kk + kq) * PSD_SYL_ULD + 16 * fj + col;
                    const double ar = Ls[lo], br = Rs[ro];
                    cr = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, cr, 0, 0, 0);
                    if (CPLX) {
                        const double ai = Ls[plane + lo], bi = Rs[plane + ro];
                        cr = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, bi, cr, 0, 0, 0);
                        ci = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ci, 0, 0, 0);
                        ci = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ci, 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }
    }
    if (!mine) return;
    // C/D fragment of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 16 * fi + kq + 4 * r, j = 16 * fj + col;
        if (i < b.mi && j < b.nj) psd_syl_store<CPLX>(g, e, b.bi0 + i, b.bj0 + j, cr[r], CPLX ? ci[r] : 0.0);
    }
}
#else
// test-tier stand-in for the matrix-core kernel: the same grid and operands, plain loops, K ascending
template <bool CPLX>
static void psd_syl_update(psd_syl_args g) {
    if (psd_atomic_load(g.flag) != 0) return;
    const int e = PSD_BLOCK_Y;
    const psd_syl_block b = psd_syl_block_of<CPLX>(g, PSD_BLOCK_X, e);
    for (int j = 0; j < b.nj; ++j)
        for (int i = 0; i < b.mi; ++i) {
            double vr = 0.0, vi = 0.0;
            for (int s = 0; s < 2; ++s) {
                const psd_syl_prod& pr = b.pr[s];
                for (int k = 0; k < pr.klen; ++k) {
                    const size_t ol = (size_t)i * pr.lsx + (size_t)k * pr.lsk, orr = (size_t)j * pr.rsx + (size_t)k * pr.rsk;
                    if (CPLX) {
                        const double xr = pr.lre * pr.L[2 * ol], xi = pr.lim * pr.L[2 * ol + 1];
                        const double yr = pr.rre * pr.R[2 * orr], yi = pr.rim * pr.R[2 * orr + 1];
                        vr += xr * yr;
                        vr += -xi * yi;
                        vi += xr * yi;
                        vi += xi * yr;
                    } else {
                        vr += (pr.lre * pr.L[ol]) * (pr.rre * pr.R[orr]);
                    }
                }
            }
            psd_syl_store<CPLX>(g, e, b.bi0 + i, b.bj0 + j, vr, vi);
        }
}
#endif
