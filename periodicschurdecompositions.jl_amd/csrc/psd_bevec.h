// Eigenvectors of MANY small periodic Schur decompositions of one shape (n, p) by periodic back-substitution: the batched
// form of psd_evec.h for the decompositions psd_d_pschur_batch leaves (Float64, all-true signature, order 8 ... 128).  The
// host driver is psd_bevec_host.inl.  The algebra — the affine maps of the cyclic recurrence, the pivot rule (psd_ev_y0,
// psd_ev_solve2), the power-of-two rescaling (psd_ev_shift, psd_ev_col::rescale), the epilogue of the back-transform
// (psd_ev_store) and the normalisation (psd_ev_norm_col) — is that of psd_evec.h, called from here; what is new is how
// the work is laid out.  The solve body is a template: its complex instantiation, for the decompositions
// psd_z_pschur_batch leaves, and the complex back-transform are in psd_zbevec.h (driver psd_zbevec_host.inl).
//
// At these orders the single path is launch-bound (a GEMM and a solve launch per 16-row chunk, two host round trips,
// five allocations, per problem) and its solve kernel gives one lane to each factor, so that at p = 4 sixty of the 64
// lanes idle.  Here one launch performs the whole back-substitution of every selected column of every problem of a group.
//
// Lane layout of psd_bev_solve.  The unit of work is (problem, solve column); the host lists the units of a group in one
// table.  A workgroup is one wavefront and carries C = 64 / LW units side by side, LW = nextpow2(p) lanes each for
// p <= 32 (p = 4: sixteen columns per wavefront), the whole wavefront for p > 32.  Lane li of a sub-group owns factor li
// (p <= 64; the lanes li >= p hold identity maps, so nextpow2(p) != p costs idle lanes inside the sub-group in the scan
// alone) or the contiguous segment psd_ev_seg(li) of the factors (p > 64).  Every unit walks its own row blocks bottom
// up; the wavefront runs as many steps as its deepest unit has blocks.  One step, for every unit at once:
//   A  the update products r_l(I) = W_l(I, rows below) y_l(rows below), one task per (unit, factor, row of the block).
//      The tasks of the wavefront are dealt over ALL 64 lanes, whichever factor a lane owns in the scan: with p = 5 the
//      three lanes per sub-group that sit out the scan take their share, with p = 40 the 24 lanes past the factors do.
//      A task is one dot product in ascending k, so its bits do not depend on the lane that ran it.
//   B  the maps of the owned factors, composed per lane, then a segmented Hillis-Steele scan over the sub-groups
//      (log2 LW steps, fixed order), all sub-groups in the same instructions.
//   C  y_0(I) from the sub-group's total (psd_ev_y0), the exponent the column reaches over its factors.
//   D  rescaling where due, y_l(I) from the prefixes, stored to X.
// No atomics, no cross-workgroup waits, no register spills (the compiler still reports 80 bytes of scratch per lane:
// profiles/batch/README.md); a unit's result does not depend on which other units share its
// wavefront, so a problem's vectors are the same bits wherever it stands in a batch.
//
// T and X stay in global memory (L1 / L2): a wavefront may hold columns of several problems, and T of one problem at the
// cap (p n^2 doubles: 512 KiB at n = 128, p = 4) does not fit the LDS.  X is written by the owning lane and read by the
// task lanes of the same wavefront behind PSD_SYNC (one workgroup, one CU, one L1).  r lives in LDS (p <= 64) or in a
// global buffer owned by the unit (p > 64).
//
// Back-transform V_l = Z_l X_l: plain FMAs, one thread per output element, one workgroup per 256 elements of a (problem,
// factor).  The tiles are at most 128 x 128 with a triangular K range, a few MFLOP at the cap and a few KFLOP at n = 8,
// where a 16 x 16 x 4 matrix-core tile would be three quarters padding and need an LDS staging pass per (problem,
// factor); the kernel is bound by the latency of its first loads either way, and the grid of nb p workgroups fills the
// machine.  The serial simulation runs the same text.
#pragma once
#include "psd_evec.h"

#define PSD_BEV_NMAX 128  // largest order of the batched kernels (above: the single path, problem by problem); conservative: measured ahead of it up to 256, profiles/batch/README.md
#define PSD_BEV_NT 256    // threads of the back-transform, normalisation and sub-diagonal kernels

// Tables of a group, uploaded once.  Integers: [wmap p | vmap p | 0 | per problem PSD_BEV_ISTRIDE | units (q, j) pairs];
// a problem's block is [bsz n | k0 n | m n | kend n | ocol n | pair n | nblk n | ns].  Doubles, per problem:
// [mu 2n | lambda 2n (both per solve column) | ev 2n (per row)].
PSD_HD int psd_bev_istride(int n) { return 7 * n + 1; }
PSD_HD int psd_bev_ihead(int p) { return 2 * p + 1; }
PSD_HD int psd_bev_dstride(int n) { return 6 * n; }

// lanes of a sub-group: nextpow2(p) up to 32, else the wavefront
PSD_HD int psd_bev_lw(int p) {
    int w = 1;
    while (w < p && w < 64) w <<= 1;
    return w;
}

struct psd_bev_args {
    const double* T;     // [gc][p][n][n], user order
    const int* itab;
    const double* dtab;
    double* X;           // [gc][2][p][n][nsm] (re | im planes per problem)
    double* R;           // p > 64: [units][p][2] complex
    int* cnt;            // [gc][n][3]: perturbed pivots, rescalings, zero eigenvalue, per solve column
    int n, p, nsm, nunits, gc, six;
};

#define PSD_BEV_LDS (192 * sizeof(psd_ev_map) + 128 * sizeof(psd_z) + 5 * 64 * sizeof(int))

// the single path's view of problem q: psd_ev_col then addresses its factors, X and tables (CPLX: T interleaved complex)
template <bool CPLX>
PSD_D void psd_bev_colargs(const psd_bev_args& a, int q, psd_ev_args& e) {
    const int n = a.n;
    const size_t xs = (size_t)a.p * n * a.nsm;
    const int* tab = a.itab + psd_bev_ihead(a.p) + (size_t)q * psd_bev_istride(n);
    const double* dt = a.dtab + (size_t)q * psd_bev_dstride(n);
    e.T = a.T + (size_t)q * a.p * n * n * (CPLX ? 2 : 1);
    e.wmap = a.itab;
    e.bsz = tab;
    e.k0 = tab + n;
    e.m = tab + 2 * n;
    e.kend = tab + 3 * n;
    e.mu = dt;
    e.lam = dt + 2 * n;
    e.ev = dt + 4 * n;
    e.Xr = a.X + (size_t)q * 2 * xs;
    e.Xi = e.Xr + xs;
    e.Rr = e.Ri = nullptr;
    e.cnt = nullptr;
    e.n = n;
    e.p = a.p;
    e.ns = a.nsm;
    e.six = a.six;
    e.r0 = e.r1 = e.jlo = 0;
}

// the row block a unit works on in this step: rows [i, i + b), the rows >= i1 done
struct psd_bev_blk {
    int q, j, i1, i, b, ke;
    bool act, isown;
};
// (a complex form has no 2x2 blocks: every block is one row, whatever the table says)
template <bool CPLX>
PSD_D psd_bev_blk psd_bev_block(const psd_bev_args& a, const int* cq, const int* cj, const int* ci1, int c) {
    psd_bev_blk k;
    k.q = cq[c];
    k.j = cj[c];
    k.i1 = ci1[c];
    k.act = k.i1 > 0;
    k.i = k.b = k.ke = 0;
    k.isown = false;
    if (k.act) {
        const int* tab = a.itab + psd_bev_ihead(a.p) + (size_t)k.q * psd_bev_istride(a.n);
        k.ke = tab[3 * a.n + k.j];
        k.isown = k.i1 == k.ke;
        k.b = CPLX ? 1 : (k.isown ? tab[2 * a.n + k.j] : (tab[k.i1 - 1] == 0 ? 2 : 1));
        k.i = k.i1 - k.b;
    }
    return k;
}

// the map of factor l in the block: y_{l+1}(I) = (D_l y_l(I) + r_l(I)) / mu
template <bool CPLX>
PSD_D psd_ev_map psd_bev_fmap(const psd_ev_col<CPLX>& col, const psd_bev_blk& k, int l, psd_z rmu, const psd_z* r) {
    psd_ev_map m = psd_ev_ident();
    psd_z D[2][2];
    const int b = CPLX ? 1 : k.b;  // (complex: D[q][kk] with q, kk > 0 is not loaded)
    col.d(l, k.i, b, D);
    for (int q = 0; q < 2; ++q)
        for (int kk = 0; kk < 2; ++kk) m.A[q][kk] = (q < b && kk < b) ? zmul(D[q][kk], rmu) : zmk(0.0, 0.0);
    if (!k.isown)
        for (int q = 0; q < 2; ++q)  // (constant bounds: the maps stay in registers)
            if (q < b) m.c[q] = zmul(r[2 * l + q], rmu);
    psd_ev_mnorm(m);
    return m;
}

// The body of psd_bev_solve (real: 1x1 and 2x2 row blocks) and of psd_zbev_solve (psd_zbevec.h; complex: the block width
// is 1 at compile time, so stage A has C p tasks and the second row of a block is never looked at).
template <bool CPLX>
PSD_D void psd_bev_solve_body(const psd_bev_args& a) {
    PSD_LDS_DECL;
    psd_ev_map* buf = (psd_ev_map*)psd_lds;  // [2][64]: the scan
    psd_ev_map* v0s = buf + 128;             // [C]: y_0(I) of a unit
    psd_z* rl = (psd_z*)(v0s + 64);          // [64][2]: r_l(I), p <= 64
    int* red = (int*)(rl + 128);             // [64]
    int* ci1 = red + 64;                     // [C]: the rows >= ci1 of the unit are done (0: nothing left)
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
            const double* dt = a.dtab + (size_t)q * psd_bev_dstride(n);
            if (dt[2 * j] == 0.0 && dt[2 * j + 1] == 0.0) {  // the recurrence divides by mu: the column is returned as NaN
                a.cnt[3 * ((size_t)q * n + j) + 2] = 1;
            } else {
                i1 = tab[3 * n + j];
                nblk = tab[6 * n + j];
            }
        }
        cq[t] = q;
        cj[t] = j;
        ci1[t] = i1;
        cnb[t] = nblk;
    }
    PSD_SYNC();
    int nstep = 0;
    for (int c = 0; c < C; ++c) nstep = cnb[c] > nstep ? cnb[c] : nstep;
    // r_l(I) of unit c, factor l: [2 l + q] of the unit's block
    psd_z* const rg = p <= 64 ? nullptr : (psd_z*)a.R + (size_t)PSD_BLOCK_X * p * 2;
    for (int step = 0; step < nstep; ++step) {
        // A: the update products, dealt over the 64 lanes
        PSD_PAR_FOR(t, 64) {
            const int cp = C * p;
            for (int tau = t; tau < (CPLX ? 1 : 2) * cp; tau += 64) {
                const int qr = tau / cp, c = (tau - qr * cp) / p, l = tau - qr * cp - c * p;
                const psd_bev_blk k = psd_bev_block<CPLX>(a, cq, cj, ci1, c);
                if (!k.act || k.isown || qr >= k.b) continue;
                psd_ev_args e;
                psd_bev_colargs<CPLX>(a, k.q, e);
                const psd_ev_col<CPLX> col(e, k.j);
                psd_z s = zmk(0.0, 0.0);
                for (int kk = k.i1; kk < k.ke; ++kk) s = zadd(s, zmul(col.w(l, k.i + qr, kk), col.x(l, kk)));
                (rg ? rg : rl + 2 * LW * c)[2 * l + qr] = s;
            }
        }
        PSD_SYNC();
        // B: the maps of the owned factors, then the segmented scan
        PSD_PAR_FOR(t, 64) {
            const int c = t / LW, li = t - c * LW;
            const psd_bev_blk k = psd_bev_block<CPLX>(a, cq, cj, ci1, c);
            psd_ev_map seg = psd_ev_ident();
            if (k.act) {
                psd_ev_args e;
                psd_bev_colargs<CPLX>(a, k.q, e);
                const psd_ev_col<CPLX> col(e, k.j);
                const psd_z rmu = zdiv(zmk(1.0, 0.0), zmk(e.mu[2 * k.j], e.mu[2 * k.j + 1]));
                const psd_z* r = rg ? rg : rl + 2 * LW * c;
                int lo, hi;
                psd_ev_seg(li, p, lo, hi);
                for (int l = lo; l < hi; ++l) seg = psd_ev_compose(psd_bev_fmap(col, k, l, rmu, r), seg);
            }
            buf[t] = seg;
        }
        PSD_SYNC();
        int cur = 0;
        for (int d = 1; d < LW; d <<= 1) {
            PSD_PAR_FOR(t, 64) {
                buf[64 * (1 - cur) + t] = (t & (LW - 1)) >= d ? psd_ev_compose(buf[64 * cur + t], buf[64 * cur + t - d])
                                                              : buf[64 * cur + t];
            }
            PSD_SYNC();
            cur = 1 - cur;
        }
        const psd_ev_map* inc = buf + 64 * cur;
        // C: y_0(I) round the period, and the largest entry y_l(I) will have
        PSD_PAR_FOR(t, 64) {
            const int c = t / LW, li = t - c * LW;
            const psd_bev_blk k = psd_bev_block<CPLX>(a, cq, cj, ci1, c);
            int mx = -100000;
            if (k.act) {
                psd_ev_args e;
                psd_bev_colargs<CPLX>(a, k.q, e);
                const psd_ev_col<CPLX> col(e, k.j);
                const psd_z rmu = zdiv(zmk(1.0, 0.0), zmk(e.mu[2 * k.j], e.mu[2 * k.j + 1]));
                const psd_z* r = rg ? rg : rl + 2 * LW * c;
                psd_z y[2];
                int e0;
                const int npert = psd_ev_y0(inc[c * LW + LW - 1], k.isown, k.b, k.i, zmk(e.lam[2 * k.j], e.lam[2 * k.j + 1]),
                                            e.ev, y, e0);
                const psd_ev_map v0 = psd_ev_vec(y, 2, e0);  // (y[1] = 0 on a 1x1 block)
                if (li == 0) {
                    v0s[c] = v0;
                    if (npert) a.cnt[3 * ((size_t)k.q * n + k.j)] += npert;
                }
                int lo, hi;
                psd_ev_seg(li, p, lo, hi);
                psd_ev_map v = li > 0 ? psd_ev_compose(inc[t - 1], v0) : v0;
                for (int l = lo; l < hi; ++l) {
                    const int ex = psd_ev_vexp(v);
                    mx = ex > mx ? ex : mx;
                    if (l + 1 < hi) v = psd_ev_compose(psd_bev_fmap(col, k, l, rmu, r), v);
                }
            }
            red[t] = mx;
        }
        PSD_SYNC();
        // D: a column growing past 2^PSD_EV_BIG is scaled down first; then y_l(I), in the scale of the stored rows
        PSD_PAR_FOR(t, 64) {
            const int c = t / LW, li = t - c * LW;
            const psd_bev_blk k = psd_bev_block<CPLX>(a, cq, cj, ci1, c);
            if (k.act) {
                psd_ev_args e;
                psd_bev_colargs<CPLX>(a, k.q, e);
                const psd_ev_col<CPLX> col(e, k.j);
                const psd_z rmu = zdiv(zmk(1.0, 0.0), zmk(e.mu[2 * k.j], e.mu[2 * k.j + 1]));
                const psd_z* r = rg ? rg : rl + 2 * LW * c;
                int big = -100000;
                for (int s = 0; s < LW; ++s) big = red[c * LW + s] > big ? red[c * LW + s] : big;
                const int shift = psd_ev_shift(big);
                if (shift && li == 0) a.cnt[3 * ((size_t)k.q * n + k.j) + 1] += 1;
                int lo, hi;
                psd_ev_seg(li, p, lo, hi);
                if (shift) col.rescale(lo, hi, k.i1, 0, shift);
                const psd_ev_map v0 = v0s[c];
                psd_ev_map v = li > 0 ? psd_ev_compose(inc[t - 1], v0) : v0;
                for (int l = lo; l < hi; ++l) {
                    for (int q = 0; q < 2; ++q)
                        if (q < k.b) col.setx(l, k.i + q, zscal(ldexp(1.0, v.s - shift), v.c[q]));
                    if (l + 1 < hi) v = psd_ev_compose(psd_bev_fmap(col, k, l, rmu, r), v);
                }
            }
        }
        PSD_SYNC();
        PSD_PAR_FOR(t, C) {
            const psd_bev_blk k = psd_bev_block<CPLX>(a, cq, cj, ci1, t);
            if (k.act) ci1[t] = k.i;
        }
        PSD_SYNC();
    }
}

// (one wavefront per workgroup: the launch bound lifts the register cap of the 1024-thread default, so nothing spills)
PSD_KERNEL_B(64) psd_bev_solve(psd_bev_args a) { psd_bev_solve_body<false>(a); }

// the sub-diagonals of the quasi-triangular factors (block `blk` of every problem): out [nb][n]
PSD_KERNEL psd_bev_subdiag(const double* T, int n, int p, int blk, int nb, double* out) {
    PSD_PAR_FOR(t, PSD_NTHREADS) {
        const size_t e = (size_t)PSD_BLOCK_X * PSD_NTHREADS + t;
        if (e < (size_t)nb * n) {
            const size_t q = e / n, i = e - q * n;
            out[e] = (int)i < n - 1 ? T[(q * p + blk) * n * n + i * n + i + 1] : 0.0;
        }
    }
}

struct psd_bev_bt_args {
    const double* Z;   // [gc][p][n][n], user order
    const double* X;
    const int* itab;
    const double* S;   // [gc][2][n]: the column factors of the normalisation (re | im), or nullptr
    const int* cnt;    // (a zero-eigenvalue column has no X: it is left to the normalisation, which makes it NaN)
    double* V;         // [gc][nmat][maxvec][n] complex interleaved
    int n, p, nsm, nmat, maxvec, z0, nz;
};

// V_z = Z_z X_vmap(z) for the factors z0 .. z0 + nz - 1 of every problem: grid (gc * nz, tiles of PSD_BEV_NT elements)
PSD_KERNEL psd_bev_backtransform(psd_bev_bt_args g) {
    const int n = g.n, q = PSD_BLOCK_X / g.nz, z = g.z0 + PSD_BLOCK_X % g.nz;
    const int* tab = g.itab + psd_bev_ihead(g.p) + (size_t)q * psd_bev_istride(n);
    const int ns = tab[7 * n], xl = g.itab[g.p + z];
    const size_t xs = (size_t)g.p * n * g.nsm;
    const double* Z = g.Z + ((size_t)q * g.p + z) * n * n;
    const double* Xr = g.X + (size_t)q * 2 * xs + (size_t)xl * n * g.nsm;
    const double* Xi = Xr + xs;
    psd_ev_gemm_args s;
    s.mode = 1;
    s.Cr = g.V + ((size_t)q * g.nmat + z) * 2 * n * g.maxvec;
    s.cmap = g.itab + 2 * g.p;  // (the zero of the table: Cr is the block already)
    s.cstride = 0;
    s.ldc = n;
    s.ocol = tab + 4 * n;
    s.pair = tab + 5 * n;
    s.sr = g.S ? g.S + (size_t)q * 2 * n : nullptr;
    s.si = g.S ? g.S + (size_t)q * 2 * n + n : nullptr;
    PSD_PAR_FOR(t, PSD_NTHREADS) {
        const int e = PSD_BLOCK_Y * PSD_NTHREADS + t;
        if (e < ns * n) {
            const int j = e / n, i = e - j * n, ke = g.cnt[3 * ((size_t)q * n + j) + 2] ? 0 : tab[3 * n + j];
            double vr = 0.0, vi = 0.0;
            for (int k = 0; k < ke; ++k) {  // (X is zero below the column's own block: K stops there)
                const double zz = Z[(size_t)k * n + i];
                vr += zz * Xr[(size_t)k * g.nsm + j];
                vi += zz * Xi[(size_t)k * g.nsm + j];
            }
            psd_ev_store(s, 0, i, j, vr, vi);
        }
    }
}

// psd_ev_norm for every solve column of every problem: one lane each
PSD_KERNEL psd_bev_norm(double* V, const int* itab, const int* cnt, double* S, int n, int p, int gc, int nmat, int maxvec) {
    PSD_PAR_FOR(t, PSD_NTHREADS) {
        const size_t e = (size_t)PSD_BLOCK_X * PSD_NTHREADS + t;
        if (e < (size_t)gc * n) {
            const size_t q = e / n;
            const int j = (int)(e - q * n);
            const int* tab = itab + psd_bev_ihead(p) + q * psd_bev_istride(n);
            if (j < tab[7 * n])
                psd_ev_norm_col(V + q * nmat * 2 * n * maxvec + 2 * (size_t)tab[4 * n + j] * n, n, tab[5 * n + j] != 0,
                                cnt[3 * e + 2] != 0, S[q * 2 * n + j], S[q * 2 * n + n + j]);
        }
    }
}
