// Batched eigenvalue reordering, Float64, all-true signature: ordschur!(P, select) (rordschur.jl:3-132) for many small
// periodic Schur forms of one shape in one launch — the follow-up of psd_d_pschur_batch (psd_batch_host.inl).
//
// One wavefront carries one problem from the first scan step to the last swap without leaving the kernel: the driver
// scan (psd_rord_scan), one window of swaps out of LDS (psd_rord_move, as it is), and the window's recorded block
// transforms applied to the off-window part of that problem by the same wavefront, until the scan runs out of rows or
// a swap is rejected.  The parallelism is across problems, as in psd_bhess and psd_bev_solve.  Nothing is shared
// between workgroups: no atomics, no waits, and a problem's result does not depend on where it stands in a batch.
//
// Hand-offs between the lanes through device memory (the window store, the transform lists, the descriptor, the
// off-window update) are ordered by PSD_SYNC(), which drains the wavefront's stores before its next loads.
#pragma once
#include "psd_rord.h"

#define PSD_BORD_WMIN 6    // least window PSD_BORD_W may ask of psd_bord (a 2x2 block and its target need more than 4 rows)
#define PSD_BORD_NMAX 128  // largest order of the batched kernel (above: rordschur_dev problem by problem); profiles/batch/README.md

// The transform lists of a window hold PSD_RORD_CAP records per owner.  A window of psd_rord_move records one per swap:
// a 1x1 or intact 2x2 block crosses at most W - 1 neighbours, the halves of a split pair two swaps per neighbour over
// at most W - 2 rows.  These spans keep every window of the batched kernel inside the lists (psd_rord_move reads the
// span from st.W; the LDS stays laid out for the launch's W, which the host keeps at or below PSD_BORD_SPAN1).
// psd_rord_move bounds its span the same way for every caller (PSD_RORD_SPAN1 / PSD_RORD_SPAN2, psd_rord.h); the spans
// here are at or below those, so the batched kernel's windows are what they were.
#define PSD_BORD_SPAN1 (PSD_RORD_CAP + 1)
#define PSD_BORD_SPAN2 (PSD_RORD_CAP / 2 + 2)

struct psd_bord_args {
    double* H;  // [nb][p][n][n] internal right order, the quasi-triangular factor first
    double* Z;  // [nb][p][n][n] or nullptr
    psd_rostate* st;       // [nb]
    psd_apply_desc* desc;  // [nb]
    psd_tq* tq;            // [nb][p][PSD_RORD_CAP]
    int* cnt;              // [nb][p]
    const unsigned char* select;  // [nb][n]
    double* wr;    // [nb][n]
    double* wi;    // [nb][n]
    double* xscr;  // [nb][n][p][8]
    int* infos;    // [nb]
    int n, p, wantZ, W;
    int maxwin;  // windows after which a problem gives up with PSD_LIST_OVERFLOW (never reached: every window swaps)
};

PSD_D psd_roparams psd_bord_params(const psd_bord_args& A, int q) {
    const size_t nn = (size_t)A.n * A.n;
    psd_roparams P;
    P.H = A.H + (size_t)q * A.p * nn;
    P.Z = A.Z ? A.Z + (size_t)q * A.p * nn : nullptr;
    P.st = A.st + q;
    P.desc = A.desc + q;
    P.tq = A.tq + (size_t)q * A.p * PSD_RORD_CAP;
    P.cnt = A.cnt + (size_t)q * A.p;
    P.select = A.select + (size_t)q * A.n;
    P.wr = A.wr + (size_t)q * A.n;
    P.wi = A.wi + (size_t)q * A.n;
    P.xscr = A.xscr + (size_t)q * A.n * A.p * 8;
    P.S = nullptr;
    P.alpha = nullptr;
    P.beta = nullptr;
    P.ascale = nullptr;
    P.mb = nullptr;
    P.slots = nullptr;
    return P;
}

// The three roles of psd_rord_apply for one problem, by one wavefront: owner m acts on the columns lc0..lc1 of T_m from
// the left, on the rows rr0..rr1 of T_{m-1} and zr0..zr1 of Z_m from the right.  A work item is one such column or row
// restricted to the window's span plo..phi: a lane copies its strip to LDS, runs the owner's list over it — per element
// the dot products of psd_rord_apply in the same order — and writes it back.  The items of all owners and roles are
// dealt to the lanes together, L per pass (tile: L strips of at most W doubles, in the window area, which is free here).
//
// SIGNED (psd_gbord, psd_gbord.h): the side follows the signature as in psd_rord_apply — owner m acts on T_m from the
// left only if S[m], otherwise from the right on its rows, and on T_{m-1} from the right only if S[m-1], otherwise from
// the left on its columns.  Every factor T_f so gets one update of its columns lc0..lc1 and one of its rows rr0..rr1,
// each by f or by its successor f+1 (cyclically); the items are dealt by factor: the columns of T_f (owner f if S[f],
// else f+1), its rows (owner f+1 if S[f], else f), the rows of Z_f (owner f).
template <bool SIGNED>
PSD_D void psd_bord_apply(const psd_roparams& P, int n, int p, double* tile, int L) {
    const psd_apply_desc d = *P.desc;
    if (!d.active) return;
    const int S = d.phi - d.plo + 1;
    const int nc = (d.lc1 >= d.lc0) ? (d.lc1 - d.lc0 + 1) : 0;
    const int nr = (d.rr1 >= d.rr0) ? (d.rr1 - d.rr0 + 1) : 0;
    const int nz = (d.zr1 >= d.zr0) ? (d.zr1 - d.zr0 + 1) : 0;
    const int per = nc + nr + nz, items = p * per;
    const size_t nn = (size_t)n * n;
    for (int i0 = 0; i0 < items; i0 += L) {
        PSD_PAR_FOR(t, L) {
            const int i = i0 + t;
            if (i < items) {
                const int m = i / per + 1, k = i - (m - 1) * per;
                const int mm1 = (m == 1) ? p : (m - 1);
                double* x;  // first element of the strip, sx doubles from one to the next
                size_t sx;
                if (k < nc) {
                    x = P.H + (size_t)(m - 1) * nn + (size_t)(d.lc0 + k - 1) * n + (d.plo - 1);
                    sx = 1;
                } else if (k < nc + nr) {
                    x = P.H + (size_t)((SIGNED ? m : mm1) - 1) * nn + (size_t)(d.plo - 1) * n + (d.rr0 + (k - nc) - 1);
                    sx = (size_t)n;
                } else {
                    x = P.Z + (size_t)(m - 1) * nn + (size_t)(d.plo - 1) * n + (d.zr0 + (k - nc - nr) - 1);
                    sx = (size_t)n;
                }
                double* v = tile + t;
                for (int r = 0; r < S; ++r) v[r * L] = x[r * sx];
                int own = m;  // whose list runs over the strip
                if constexpr (SIGNED) {  // the columns of T_m: m if S[m], else its successor; the rows: the other one
                    if (k < nc + nr && (k < nc) != psd_rosig(P, m)) own = (m == p) ? 1 : (m + 1);
                }
                const int cnt = P.cnt[own - 1] < PSD_RORD_CAP ? P.cnt[own - 1] : PSD_RORD_CAP;
                const psd_tq* list = P.tq + (size_t)(own - 1) * PSD_RORD_CAP;
                for (int e = 0; e < cnt; ++e) {
                    const psd_tq& tr = list[e];
                    const int r = tr.pos - d.plo, mm = tr.m;
                    double a[4], b[4];
                    for (int q = 0; q < mm; ++q) a[q] = v[(r + q) * L];
                    for (int rr = 0; rr < mm; ++rr) {
                        double s = 0.0;
                        for (int q = 0; q < mm; ++q) s += tr.q[rr * 4 + q] * a[q];
                        b[rr] = s;
                    }
                    for (int q = 0; q < mm; ++q) v[(r + q) * L] = b[q];
                }
                for (int r = 0; r < S; ++r) x[r * sx] = v[r * L];
            }
        }
    }
}

// One problem from the first scan to the last swap, by one wavefront; P: its parameters, the others the members of the
// launch's psd_bord_args of these names, info: where the problem's code goes.  SIGNED: P.S
// is the signature of the batch (psd_gbord.h), which the flags SL of the left-oriented sequence X_l = T_{sigma(l)} and
// the sides of the off-window update follow as in psd_rord_step / psd_rord_apply; otherwise every flag is 1.
template <bool SIGNED>
PSD_D void psd_bord_body(const psd_roparams P, const int n, const int p, const int wantZ, const int W, const int maxwin,
                         int* info) {
    PSD_LDS_DECL;
    psd_rostate st;
    st.n = n; st.p = p; st.wantZ = wantZ; st.W = W;
    st.phase = PSD_ROPH_SCAN; st.info = 0;
    st.j = 0; st.jdest = 0; st.pairskip = 0;
    st.here = 0; st.nbsrc = 1; st.splitsrc = 0; st.jtarget = 0; st.jsrc0 = 0; st.pend1x1 = 0;
    st.nswaps = 0; st.nwindows = 0;
    for (int e = 0; e < 6; ++e) st.cyc[e] = 0;
    long long cyc[6] = {0, 0, 0, 0, 0, 0};
    double* ldsd = (double*)psd_lds;
    const size_t winb = (size_t)p * W * (W + 1);
    double* scr = ldsd + winb;
    double* wk = scr + (size_t)p * PSD_RORD_SCR;
    double* flagbuf = wk + (size_t)p * 52;
    double* ws = flagbuf + 4;
    int* lcnt = (int*)(ws + 192 + psd_rord_tree_doubles(p));
    unsigned char* SL = (unsigned char*)(lcnt + p);
    if constexpr (SIGNED) {
        PSD_PAR_FOR(t, p) { SL[t] = psd_rosig(P, psd_ord_sigma(p, t + 1)) ? 1 : 0; }
    } else {
        PSD_PAR_FOR(t, p) { SL[t] = 1; }
    }
    PSD_SYNC();
    const int L = (winb / (size_t)W < (size_t)PSD_STEP_NT) ? (int)(winb / (size_t)W) : PSD_STEP_NT;  // (>= W + 1)
    for (;;) {
        psd_rord_scan(P, st);
        if (st.phase != PSD_ROPH_MOVE) break;
        if (st.nwindows >= maxwin) {
            st.info = PSD_LIST_OVERFLOW;
            st.phase = PSD_ROPH_DONE;
            break;
        }
        const int span = (st.nbsrc == 2) ? PSD_BORD_SPAN2 : PSD_BORD_SPAN1;
        st.W = (W < span) ? W : span;
        psd_rord_move(P, st, ldsd, scr, wk, flagbuf, ws, lcnt, SL, cyc);
        st.W = W;
        if (st.phase == PSD_ROPH_DONE) break;  // rejected swap: the factors are as they were before this window
        PSD_SYNC();
        if (psd_list_overflow(lcnt, p, PSD_RORD_CAP)) {
            st.info = PSD_LIST_OVERFLOW;
            st.phase = PSD_ROPH_DONE;
            break;
        }
        psd_bord_apply<SIGNED>(P, n, p, ldsd, L);
        PSD_SYNC();
    }
    PSD_SYNC();
    PSD_ONE {
        *P.st = st;
        *info = st.info;
    }
}

// grid = problems of the group, one wavefront each; LDS = rord_lds_bytes(p, W)
PSD_KERNEL_B(PSD_STEP_NT) psd_bord(psd_bord_args A) {
    const int q = PSD_BLOCK_X;
    psd_bord_body<false>(psd_bord_params(A, q), A.n, A.p, A.wantZ, A.W, A.maxwin, A.infos + q);
}

// psd_rord_values for a batch: grid = (ceil(n / 64), nb), 64 threads.  Problems with a non-zero info are skipped.
PSD_KERNEL psd_bord_values(psd_bord_args A) {
    const int q = PSD_BLOCK_Y;
    if (A.infos[q] != 0) return;
    const psd_roparams P = psd_bord_params(A, q);
    const int NT = PSD_NTHREADS;
    PSD_PAR_FOR(t, NT) {
        const int j = 1 + PSD_BLOCK_X * NT + t;
        if (j <= A.n) psd_rord_value_at(P, A.n, A.p, j);
    }
}

// psd_rord_cleanup for a batch: grid = (n, nb)
PSD_KERNEL psd_bord_cleanup(psd_bord_args A) {
    const int q = PSD_BLOCK_Y;
    if (A.infos[q] != 0) return;
    psd_rord_cleanup_col(psd_bord_params(A, q), A.n, PSD_BLOCK_X + 1);
}

// User order <-> internal order of the [nb][p] blocks of `blk` doubles (ord_slots): internal block j is user block
// slot[j].  gather != 0: dst (internal) from src (user); otherwise dst (user) from src (internal).  grid = nb * p
PSD_KERNEL psd_bord_permute(double* dst, const double* src, const int* slot, size_t blk, int p, int gather) {
    const int q = PSD_BLOCK_X / p, j = PSD_BLOCK_X % p;
    const size_t bi = ((size_t)q * p + j) * blk, bu = ((size_t)q * p + slot[j]) * blk;
    double* d = dst + (gather ? bi : bu);
    const double* s = src + (gather ? bu : bi);
    PSD_PAR_FOR(e, blk) { d[e] = s[e]; }
}
