// Eigenvectors of MANY small signed Float64 periodic Schur decompositions of one shape (n, p) and one signature, zero and
// infinite eigenvalues included: the batched form of psd_gevec.h for the decompositions psd_d_gpschur_batch /
// psd_d_gordschur_batch leave.  The host driver is psd_gbevec_host.inl.  The algebra — the homogeneous maps psd_gm<B> with
// their composition and normalisation, the three cases of psd_gev_map, the pivot and exponent rules of psd_gev_lane, the
// null vector of the own 2x2 block (psd_gev_null) — is that of psd_gevec.h, called from here at both block widths; the
// layout — the unit of work (problem, solve column), C = 64 / LW units per wavefront, lane li of a sub-group the owner of
// factor li or of the segment psd_ev_seg(li), the tables of psd_bev_args, stage A dealt over all 64 lanes — is that of
// psd_bev_solve_body (psd_bevec.h) and psd_zgbev_solve (psd_zgbevec.h).  The back-transform and the normalisation are
// psd_bev_backtransform and psd_bev_norm; slot 2 of their counters ("emit a NaN column") is never set here: a zero or
// infinite eigenvalue gives a valid column, and the host counts it from the scalars.
//
// psd_gbev_solve: one launch for the whole back-substitution of every selected column of every problem of a group.  A
// real form is quasi-triangular in one factor: a row block is one row or two, and so is the own block of a column (a
// conjugate pair is one solve column).  The scalars a_l of every solve column (the diagonal entries, or the pair scalars)
// come from the host with the group's tables: [problem][solve column][working factor] complex in dtab.  One step per row
// block, bottom up, for every unit of the wavefront at once; the units of one wavefront stand on blocks of different
// width in the same step, so stages B to D are instantiated at both widths and a sub-group takes the branch of its block
// (a 1x1 map is never padded into a 2x2 one: psd_gm_norm would see the padding), every PSD_SYNC outside the branches:
//   A  r_l(I) = W_l(I, rows below) x_lx(rows below), lx = l for a forward factor and l + 1 (cyclic) for an inverted one:
//      one task per (unit, factor, row of the block), dealt over all 64 lanes, one dot product in ascending k each.  The
//      rows of X_{l+1} an inverted factor reads were written by another lane of the same wavefront, before the last
//      PSD_SYNC.
//   B  the maps of the owned factors, composed per lane, then a segmented forward and (off the own block) a segmented
//      backward inclusive scan over the sub-groups (Hillis-Steele, log2 LW steps, fixed order; the lanes li >= p hold
//      identity maps).  A sub-group's scan slots hold LW psd_gm<2>, or, in the same bytes, LW psd_gm<1>.
//   C  the own 2x2 block: y_0 the null vector round the period from the sub-group's total; else y_l(I) from
//      (C - A^(l)) y_l = B^(l) with the smin rule (psd_gev_lane): the perturbed pivots, counted at factor 0, and the
//      largest exponent the column reaches, reduced over the sub-group.
//   D  rescaling where due (psd_ev_col::rescale), y_l(I) stored to X; the own 1x1 block: x_l[k] = 1 for every l.
// No atomics, no cross-workgroup waits; a unit's result does not depend on the units that share its wavefront, so a
// problem's vectors are the same bits wherever it stands in a batch.  LDS: four arrays of 64 psd_gm<2> (two
// double-buffered scans, 28 KiB), the r slots and the unit bookkeeping, 31.3 KiB; r of a unit lives in a global buffer for
// p > 64 (as psd_bev_solve).  Registers and scratch: profiles/batch/README.md.
#pragma once
#include "psd_gevec.h"
#include "psd_bevec.h"

struct psd_gbev_args {
    psd_bev_args b;   // dtab: [gc][n][p] complex, the scalar a of working factor l for solve column j of problem q
    const int* sgn;   // [p] per working factor: 1 forward, 0 inverted
};

#define PSD_GBEV_LDS (4 * 64 * sizeof(psd_gm<2>) + 128 * sizeof(psd_z) + 5 * 64 * sizeof(int))

// what the maps of a unit take from it (psd_gev_src of the single path): a_l from the uploaded scalars of the unit,
// r_l(row) from the unit's slots
struct psd_gbev_src {
    const double* ac;  // [2 l]: a_l (re, im)
    const int* sgn;
    const psd_z* rv;   // [2 l + q]: r_l(i + q) of the current step
    int i;             // the first row of the current block
    PSD_HD psd_z a(int l) const { return zmk(ac[2 * l], ac[2 * l + 1]); }
    PSD_HD bool fwd(int l) const { return sgn[l] != 0; }
    PSD_HD psd_z r(int l, int row) const { return rv[2 * l + (row - i)]; }
};

// scan array `arr` (0, 1: the forward scan's two buffers; 2, 3: the backward scan's) of the sub-group that starts at lane
// t0, as maps of width B
template <int B>
PSD_D psd_gm<B>* psd_gbev_slots(char* lds, int arr, int t0) {
    return (psd_gm<B>*)(lds + ((size_t)arr * 64 + t0) * sizeof(psd_gm<2>));
}

// stage B of lane li of a sub-group standing on a block of width B: the composed maps of its factors
template <int B>
PSD_D void psd_gbev_seg(const psd_gbev_src& src, const psd_ev_col<false>& col, const psd_bev_blk& k, int li, char* lds,
                        int t0) {
    int lo, hi;
    psd_ev_seg(li, col.a.p, lo, hi);
    psd_gm<B> seg = psd_gm_ident<B>();
    for (int l = lo; l < hi; ++l) seg = psd_gm_compose(psd_gev_map<false, B>(src, col, l, k.i, k.isown), seg);
    psd_gbev_slots<B>(lds, 0, t0)[li] = seg;
    if (!k.isown) psd_gbev_slots<B>(lds, 2, t0)[li] = seg;
}

// one Hillis-Steele step (distance d) of both scans of a sub-group, from buffer cur into the other (the own block needs
// only the forward scan)
template <int B>
PSD_D void psd_gbev_scan(char* lds, int t0, int li, int LW, int d, int cur, bool own) {
    const psd_gm<B>* F0 = psd_gbev_slots<B>(lds, cur, t0);
    psd_gm<B>* F1 = psd_gbev_slots<B>(lds, 1 - cur, t0);
    F1[li] = li >= d ? psd_gm_compose(F0[li], F0[li - d]) : F0[li];
    if (!own) {
        const psd_gm<B>* S0 = psd_gbev_slots<B>(lds, 2 + cur, t0);
        psd_gm<B>* S1 = psd_gbev_slots<B>(lds, 3 - cur, t0);
        S1[li] = li + d < LW ? psd_gm_compose(S0[li + d], S0[li]) : S0[li];
    }
}

// stages C (store = false: returns the largest exponent of the lane's factors, np the perturbed pivots) and D (store =
// true) of lane li
template <int B>
PSD_D int psd_gbev_lane(const psd_gbev_src& src, const psd_ev_col<false>& col, const psd_bev_blk& k, char* lds, int t0,
                        int li, int LW, int cur, bool store, int shift, int& np) {
    const psd_gm<B>* inc = psd_gbev_slots<B>(lds, cur, t0);
    const psd_gm<B>* suf = psd_gbev_slots<B>(lds, 2 + cur, t0);
    psd_z y0[2] = {zmk(1.0, 0.0), zmk(0.0, 0.0)};
    if (k.isown && B == 2) psd_gev_null(inc[LW - 1], y0);
    int mx;
    psd_gev_lane<false, B>(src, col, inc, suf, li, LW, k.i, k.isown, y0, store, shift, mx, np);
    return mx;
}

PSD_KERNEL_B(64) psd_gbev_solve(psd_gbev_args g) {
    PSD_LDS_DECL;
    const psd_bev_args& a = g.b;
    psd_z* rl = (psd_z*)(psd_lds + 4 * 64 * sizeof(psd_gm<2>));  // [64][2]: r_l(I), p <= 64
    int* red = (int*)(rl + 128);                                 // [64]
    int* ci1 = red + 64;  // [C]: the rows >= ci1 of the unit are done (0: nothing left)
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
    // r_l(I) of unit c, factor l, row q of the block: [2 l + q] of the unit's block
    psd_z* const rg = p <= 64 ? nullptr : (psd_z*)a.R + (size_t)PSD_BLOCK_X * p * 2;
    for (int step = 0; step < nstep; ++step) {
        // A: the update products, dealt over the 64 lanes
        PSD_PAR_FOR(t, 64) {
            const int cp = C * p;
            for (int tau = t; tau < 2 * cp; tau += 64) {
                const int qr = tau / cp, c = (tau - qr * cp) / p, l = tau - qr * cp - c * p;
                const psd_bev_blk k = psd_bev_block<false>(a, cq, cj, ci1, c);
                if (!k.act || k.isown || qr >= k.b) continue;
                psd_ev_args e;
                psd_bev_colargs<false>(a, k.q, e);
                const psd_ev_col<false> col(e, k.j);
                const int lx = g.sgn[l] ? l : (l + 1 == p ? 0 : l + 1);
                psd_z s = zmk(0.0, 0.0);
                for (int kk = k.i1; kk < k.ke; ++kk) s = zadd(s, zmul(col.w(l, k.i + qr, kk), col.x(lx, kk)));
                (rg ? rg : rl + 2 * LW * c)[2 * l + qr] = s;
            }
        }
        PSD_SYNC();
        // B: the maps of the owned factors, then the segmented scans (the own 1x1 block has neither)
        PSD_PAR_FOR(t, 64) {
            const int c = t / LW, li = t - c * LW;
            const psd_bev_blk k = psd_bev_block<false>(a, cq, cj, ci1, c);
            if (k.act && !(k.isown && k.b == 1)) {
                psd_ev_args e;
                psd_bev_colargs<false>(a, k.q, e);
                const psd_ev_col<false> col(e, k.j);
                const psd_gbev_src src{a.dtab + 2 * ((size_t)k.q * n + k.j) * p, g.sgn, rg ? rg : rl + 2 * LW * c, k.i};
                if (k.b == 2) psd_gbev_seg<2>(src, col, k, li, psd_lds, c * LW);
                else psd_gbev_seg<1>(src, col, k, li, psd_lds, c * LW);
            }
        }
        PSD_SYNC();
        int cur = 0;
        for (int d = 1; d < LW; d <<= 1) {
            PSD_PAR_FOR(t, 64) {
                const int c = t / LW, li = t - c * LW;
                const psd_bev_blk k = psd_bev_block<false>(a, cq, cj, ci1, c);
                if (k.act && !(k.isown && k.b == 1)) {
                    if (k.b == 2) psd_gbev_scan<2>(psd_lds, c * LW, li, LW, d, cur, k.isown);
                    else psd_gbev_scan<1>(psd_lds, c * LW, li, LW, d, cur, false);
                }
            }
            PSD_SYNC();
            cur = 1 - cur;
        }
        // C: the largest entry y_l(I) will have, the perturbed pivots
        PSD_PAR_FOR(t, 64) {
            const int c = t / LW, li = t - c * LW;
            const psd_bev_blk k = psd_bev_block<false>(a, cq, cj, ci1, c);
            int mx = -100000;
            if (k.act && !(k.isown && k.b == 1)) {
                psd_ev_args e;
                psd_bev_colargs<false>(a, k.q, e);
                const psd_ev_col<false> col(e, k.j);
                const psd_gbev_src src{a.dtab + 2 * ((size_t)k.q * n + k.j) * p, g.sgn, rg ? rg : rl + 2 * LW * c, k.i};
                int np;
                if (k.b == 2) mx = psd_gbev_lane<2>(src, col, k, psd_lds, c * LW, li, LW, cur, false, 0, np);
                else mx = psd_gbev_lane<1>(src, col, k, psd_lds, c * LW, li, LW, cur, false, 0, np);
                if (li == 0 && np) a.cnt[3 * ((size_t)k.q * n + k.j)] += np;
            }
            red[t] = mx;
        }
        PSD_SYNC();
        // D: a column growing past 2^PSD_EV_BIG is scaled down first; then y_l(I), in the scale of the stored rows
        PSD_PAR_FOR(t, 64) {
            const int c = t / LW, li = t - c * LW;
            const psd_bev_blk k = psd_bev_block<false>(a, cq, cj, ci1, c);
            if (k.act) {
                psd_ev_args e;
                psd_bev_colargs<false>(a, k.q, e);
                const psd_ev_col<false> col(e, k.j);
                int lo, hi;
                psd_ev_seg(li, p, lo, hi);
                if (k.isown && k.b == 1) {  // x_l[k] = 1 for every l
                    for (int l = lo; l < hi; ++l) col.setx(l, k.i, zmk(1.0, 0.0));
                } else {
                    const psd_gbev_src src{a.dtab + 2 * ((size_t)k.q * n + k.j) * p, g.sgn, rg ? rg : rl + 2 * LW * c, k.i};
                    int big = -100000;
                    for (int s = 0; s < LW; ++s) big = red[c * LW + s] > big ? red[c * LW + s] : big;
                    const int shift = psd_ev_shift(big);
                    if (shift && li == 0) a.cnt[3 * ((size_t)k.q * n + k.j) + 1] += 1;
                    if (shift) col.rescale(lo, hi, k.i1, 0, shift);
                    int np;
                    if (k.b == 2) psd_gbev_lane<2>(src, col, k, psd_lds, c * LW, li, LW, cur, true, shift, np);
                    else psd_gbev_lane<1>(src, col, k, psd_lds, c * LW, li, LW, cur, true, shift, np);
                }
            }
        }
        PSD_SYNC();
        PSD_PAR_FOR(t, C) {
            const psd_bev_blk k = psd_bev_block<false>(a, cq, cj, ci1, t);
            if (k.act) ci1[t] = k.i;
        }
        PSD_SYNC();
    }
}
