// Eigenvectors of MANY small signed ComplexF64 periodic Schur decompositions of one shape (n, p) and one signature, zero
// and infinite eigenvalues included: the batched form of psd_gevec.h for the decompositions psd_z_gpschur_batch /
// psd_z_gordschur_batch leave.  The host driver is psd_zgbevec_host.inl.  The algebra — the homogeneous maps psd_gm<1>
// with their composition and normalisation, the three cases of psd_gev_map, the pivot and exponent rules of psd_gev_lane —
// is that of psd_gevec.h, called from here; the layout — the unit of work (problem, solve column), C = 64 / LW units per
// wavefront, lane li of a sub-group the owner of factor li or of the segment psd_ev_seg(li), the tables of psd_bev_args —
// is that of psd_bev_solve_body (psd_bevec.h).  The back-transform and the normalisation are psd_zbev_backtransform and
// psd_bev_norm; slot 2 of their counters ("emit a NaN column") is never set here: a zero or infinite eigenvalue gives a
// valid column, counted in a flag array of its own (zc).
//
// psd_zgbev_solve: one launch for the whole back-substitution of every selected column of every problem of a group.  A
// complex form is triangular in every factor: every row block is one row.  The first step of a unit is its own row k,
// x_l[k] = 1 for every l, and the flag of a zero scalar a_l = T_l(k, k); the scalars are read from the factors on the
// device, so nothing is gathered, read back or uploaded before the solve.  One further step per row I above, for every
// unit at once:
//   A  r_l(I) = W_l(I, rows below) x_lx(rows below), lx = l for a forward factor and l + 1 (cyclic) for an inverted one:
//      one task per (unit, factor), dealt over all 64 lanes, one dot product in ascending k each.  The rows of X_{l+1} an
//      inverted factor reads were written by another lane of the same wavefront, before the last PSD_SYNC.
//   B  the maps of the owned factors, composed per lane, then a segmented forward and a segmented backward inclusive scan
//      over the sub-groups (Hillis-Steele, log2 LW steps, fixed order, all sub-groups in the same instructions; the lanes
//      li >= p hold identity maps).  Both directions: an open chain (a zero c) takes y_l from the period rotated to
//      start at l, as psd_gev_row does.
//   C  y_l(I) from (C - A^(l)) y_l = B^(l) with the smin rule (psd_gev_lane): the perturbed pivots, counted at factor 0,
//      and the largest exponent the column reaches, reduced over the sub-group.
//   D  rescaling where due (psd_ev_col::rescale), y_l(I) stored to X.
// No atomics, no cross-workgroup waits; a unit's result does not depend on the units that share its wavefront, so a
// problem's vectors are the same bits wherever it stands in a batch.  LDS: four arrays of 64 psd_gm<1> (two
// double-buffered scans), the r slots and the unit bookkeeping, 15.3 KiB; r of a unit lives in a global buffer for p > 64
// (as psd_bev_solve).  Registers and scratch: profiles/batch/README.md.
#pragma once
#include "psd_gevec.h"
#include "psd_zbevec.h"

struct psd_zgbev_args {
    psd_bev_args b;   // (dtab unused: no roots, no eigenvalues)
    const int* sgn;   // [p] per working factor: 1 forward, 0 inverted
    int* zc;          // [gc][n] per solve column: 1 if a scalar a_l is zero (a zero or infinite eigenvalue)
};

#define PSD_ZGBEV_LDS (4 * 64 * sizeof(psd_gm<1>) + 128 * sizeof(psd_z) + 5 * 64 * sizeof(int))

// what the maps of a unit take from it (psd_gev_src of the single path): a_l from the diagonal of the factor at the
// column's own row, r_l(I) from the unit's slots
struct psd_zgbev_src {
    const psd_ev_col<true>& col;
    const int* sgn;
    const psd_z* rv;  // [2 l]: r_l(I) of the current step
    int k;            // the column's own row
    PSD_HD psd_z a(int l) const { return col.w(l, k, k); }
    PSD_HD bool fwd(int l) const { return sgn[l] != 0; }
    PSD_HD psd_z r(int l, int) const { return rv[2 * l]; }
};

PSD_KERNEL_B(64) psd_zgbev_solve(psd_zgbev_args g) {
    PSD_LDS_DECL;
    const psd_bev_args& a = g.b;
    psd_gm<1>* F = (psd_gm<1>*)psd_lds;  // [2][64]: the forward scan
    psd_gm<1>* Sf = F + 128;             // [2][64]: the backward scan
    psd_z* rl = (psd_z*)(Sf + 128);      // [64][2]: r_l(I), p <= 64
    int* red = (int*)(rl + 128);         // [64]
    int* ci1 = red + 64;                 // [C]: the rows >= ci1 of the unit are done (0: nothing left)
    int* cq = ci1 + 64;
    int* cj = cq + 64;
    int* cnb = cj + 64;
    const int n = a.n, p = a.p, LW = psd_bev_lw(p), C = 64 / LW;
    const int* units = a.itab + psd_bev_ihead(p) + (size_t)a.gc * psd_bev_istride(n);
    PSD_PAR_FOR(t, C) {
        const int u = PSD_BLOCK_X * C + t;
        int q = 0, j = 0, i1 = 0, nblk = 0;
        if (u < a.nunits) {
            q = units[2 * u];
            j = units[2 * u + 1];
            const int* tab = a.itab + psd_bev_ihead(p) + (size_t)q * psd_bev_istride(n);
            i1 = tab[3 * n + j];
            nblk = tab[6 * n + j];
        }
        cq[t] = q;
        cj[t] = j;
        ci1[t] = i1;
        cnb[t] = nblk;
    }
    PSD_SYNC();
    int nstep = 0;
    for (int c = 0; c < C; ++c) nstep = cnb[c] > nstep ? cnb[c] : nstep;
    // r_l(I) of unit c, factor l: [2 l] of the unit's block
    psd_z* const rg = p <= 64 ? nullptr : (psd_z*)a.R + (size_t)PSD_BLOCK_X * p * 2;
    for (int step = 0; step < nstep; ++step) {
        // A: the update products, dealt over the 64 lanes
        PSD_PAR_FOR(t, 64) {
            const int cp = C * p;
            for (int tau = t; tau < cp; tau += 64) {
                const int c = tau / p, l = tau - c * p;
                const psd_bev_blk k = psd_bev_block<true>(a, cq, cj, ci1, c);
                if (!k.act || k.isown) continue;
                psd_ev_args e;
                psd_bev_colargs<true>(a, k.q, e);
                const psd_ev_col<true> col(e, k.j);
                const int lx = g.sgn[l] ? l : (l + 1 == p ? 0 : l + 1);
                psd_z s = zmk(0.0, 0.0);
                for (int kk = k.i1; kk < k.ke; ++kk) s = zadd(s, zmul(col.w(l, k.i, kk), col.x(lx, kk)));
                (rg ? rg : rl + 2 * LW * c)[2 * l] = s;
            }
        }
        PSD_SYNC();
        // B: the maps of the owned factors, then the segmented scans
        PSD_PAR_FOR(t, 64) {
            const int c = t / LW, li = t - c * LW;
            const psd_bev_blk k = psd_bev_block<true>(a, cq, cj, ci1, c);
            psd_gm<1> seg = psd_gm_ident<1>();
            if (k.act && !k.isown) {
                psd_ev_args e;
                psd_bev_colargs<true>(a, k.q, e);
                const psd_ev_col<true> col(e, k.j);
                const psd_zgbev_src src{col, g.sgn, rg ? rg : rl + 2 * LW * c, k.ke - 1};
                int lo, hi;
                psd_ev_seg(li, p, lo, hi);
                for (int l = lo; l < hi; ++l) seg = psd_gm_compose(psd_gev_map<true, 1>(src, col, l, k.i, false), seg);
            }
            F[t] = seg;
            Sf[t] = seg;
        }
        PSD_SYNC();
        int cur = 0;
        for (int d = 1; d < LW; d <<= 1) {
            PSD_PAR_FOR(t, 64) {
                const int li = t & (LW - 1);
                F[64 * (1 - cur) + t] = li >= d ? psd_gm_compose(F[64 * cur + t], F[64 * cur + t - d]) : F[64 * cur + t];
                Sf[64 * (1 - cur) + t] = li + d < LW ? psd_gm_compose(Sf[64 * cur + t + d], Sf[64 * cur + t])
                                                     : Sf[64 * cur + t];
            }
            PSD_SYNC();
            cur = 1 - cur;
        }
        const psd_gm<1>* inc = F + 64 * cur;
        const psd_gm<1>* suf = Sf + 64 * cur;
        const psd_z y0[2] = {zmk(1.0, 0.0), zmk(0.0, 0.0)};
        // C: the largest entry y_l(I) will have, the perturbed pivots; the own row: whether a scalar of the lane is zero
        PSD_PAR_FOR(t, 64) {
            const int c = t / LW, li = t - c * LW;
            const psd_bev_blk k = psd_bev_block<true>(a, cq, cj, ci1, c);
            int mx = -100000;
            if (k.act) {
                psd_ev_args e;
                psd_bev_colargs<true>(a, k.q, e);
                const psd_ev_col<true> col(e, k.j);
                const psd_zgbev_src src{col, g.sgn, rg ? rg : rl + 2 * LW * c, k.ke - 1};
                if (k.isown) {
                    int lo, hi;
                    psd_ev_seg(li, p, lo, hi);
                    mx = 0;
                    for (int l = lo; l < hi; ++l) mx |= ziszero(src.a(l)) ? 1 : 0;
                } else {
                    int np;
                    psd_gev_lane<true, 1>(src, col, inc + c * LW, suf + c * LW, li, LW, k.i, false, y0, false, 0, mx, np);
                    if (li == 0 && np) a.cnt[3 * ((size_t)k.q * n + k.j)] += np;
                }
            }
            red[t] = mx;
        }
        PSD_SYNC();
        // D: a column growing past 2^PSD_EV_BIG is scaled down first; then y_l(I), in the scale of the stored rows
        PSD_PAR_FOR(t, 64) {
            const int c = t / LW, li = t - c * LW;
            const psd_bev_blk k = psd_bev_block<true>(a, cq, cj, ci1, c);
            if (k.act) {
                psd_ev_args e;
                psd_bev_colargs<true>(a, k.q, e);
                const psd_ev_col<true> col(e, k.j);
                int lo, hi;
                psd_ev_seg(li, p, lo, hi);
                if (k.isown) {  // x_l[k] = 1 for every l
                    for (int l = lo; l < hi; ++l) col.setx(l, k.i, zmk(1.0, 0.0));
                    if (li == 0) {
                        int z = 0;
                        for (int s = 0; s < LW; ++s) z |= red[c * LW + s];
                        g.zc[(size_t)k.q * n + k.j] = z;
                    }
                } else {
                    const psd_zgbev_src src{col, g.sgn, rg ? rg : rl + 2 * LW * c, k.ke - 1};
                    int big = -100000;
                    for (int s = 0; s < LW; ++s) big = red[c * LW + s] > big ? red[c * LW + s] : big;
                    const int shift = psd_ev_shift(big);
                    if (shift && li == 0) a.cnt[3 * ((size_t)k.q * n + k.j) + 1] += 1;
                    if (shift) col.rescale(lo, hi, k.i1, 0, shift);
                    int mx, np;
                    psd_gev_lane<true, 1>(src, col, inc + c * LW, suf + c * LW, li, LW, k.i, false, y0, true, shift, mx, np);
                }
            }
        }
        PSD_SYNC();
        PSD_PAR_FOR(t, C) {
            const psd_bev_blk k = psd_bev_block<true>(a, cq, cj, ci1, t);
            if (k.act) ci1[t] = k.i;
        }
        PSD_SYNC();
    }
}

// the diagonals of the factors of a whole batch: out [nb * p][n] complex, out(m, i) = T_m(i, i)
PSD_KERNEL psd_zgbev_diag(const double* T, int n, size_t nmat, double* out) {
    PSD_PAR_FOR(t, PSD_NTHREADS) {
        const size_t e = (size_t)PSD_BLOCK_X * PSD_NTHREADS + t;
        if (e < nmat * n) {
            const size_t m = e / n, i = e - m * n;
            out[2 * e] = T[2 * (m * n * n + i * n + i)];
            out[2 * e + 1] = T[2 * (m * n * n + i * n + i) + 1];
        }
    }
}
