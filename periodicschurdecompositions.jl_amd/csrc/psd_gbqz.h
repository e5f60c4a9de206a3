// Batched real SIGNED periodic Hessenberg reduction and QZ iteration: _phessenberg!(A, S) (generalized.jl:988-1082) and
// pschur!(H1, Hs, S) for Float64 (rgeneralized.jl:49-1083, after MB03BD) for many small problems of one shape (n, p) and
// ONE signature S in one launch per stage — the kernels behind psd_d_gphessenberg_batch / psd_d_gpschur_batch
// (psd_gbatch_host.inl).  The real counterpart of psd_zgbqz.h, built from the bodies of psd_rgz.h and psd_hess.h: T_1
// comes out quasi-triangular, the Z_l orthogonal, conjugate pairs as exact conjugates.
//
// psd_gbhess1: ONE workgroup owns ONE problem and walks stage 1 of sghess_dev (generalized.jl:988-1033): for l = p..2 the
// anti-transpose of A_l and the flips of A_{l-1} and Q_l when !S[l], the reflector chain of A_l — psd_hess_refl_body, then
// the blocks of psd_hess_apply2 (psd_hess_apply_body on A_l from the left, on Q_l from the right and on the neighbour
// A_{l-1}: from the right for S[l-1], from the left otherwise) —, psd_tril_zero, and the flips undone.  A workgroup
// barrier stands where a launch boundary stood; the reflector that the single call hands from launch to launch through
// c->vbuf lives in LDS.
//   The single call forms reflector i + 1 behind block 0 of link i's update (psd_hess_apply2 with vnext), here it is taken
//   after ALL blocks of link i.  The real psd_hess_apply2 allows the argument of psd_zgbhess1: that reflector reads and
//   rewrites column i + 1 of A_l, rows i + 1..n, and among the blocks of the launch only block 0 touches that column (the
//   left blocks own four columns of A_l each, block 0 columns i + 1..i + 4; every other block works on Q_l or A_{l-1},
//   which are other matrices), and block 0 has updated it before it forms the reflector.  The column holds the same
//   values after all blocks as behind block 0, the body and its reduction order (PSD_HESS_NT threads) are the same, so
//   the reflector is the same one, bit for bit.  Nothing has to be handled.
//
// psd_gbqz: ONE wavefront (64 threads, PSD_STEP_NT) carries ONE problem from psd_gq_init_body's state to PSD_GPH_DONE
// without leaving the kernel.  A tick is what giterate_dev launches per tick without trains: psd_gq_step_body (deflation
// tests 1-3, the controlled zero shift, Cases II / III directly on HBM, 1x1 splits, 2x2 blocks of both kinds, one window
// of the double-shift sweep chased out of LDS), psd_gq_apply_item over the roles, factors and tiles of psd_gq_apply, the
// deferred side of H_1 (psd_gq_defer_body).  With hessmode = 1 it is stage 2 of the reduction in its serial form
// (psd_gq_hess_window, what PSD_HESS_SERIAL=1 selects in the single call), with hessmode = 0 the iteration.  No trains
// (train_want = 1; cst, cep and tshift are null: PSD_GPH_TWAIT is never entered), no pipeline over the factors.
//
// Geometry and sweep form: the SINGLE-WAVE sweep (gcoff = gtaboff = 0, what PSD_GSCAN=0 selects in the single call) in a
// workgroup of one wavefront.  The step body runs its state machine on one wavefront in either form; the scan form adds
// three helper wavefronts that wait on a command block in LDS between sweep windows.  In a kernel that never leaves the
// problem they would hold three of the compute unit's SIMDs for the problem's whole life while the windows they help with
// are, at the orders this kernel is for, a small part of a tick — the decisions, the 2x2 solvers and the apply items are
// single-wave or PSD_PAR_FOR code that a helper parked in psd_gs3_helper cannot join —, and they would put hardware
// barriers of four wavefronts next to hand-offs that PSD_SYNC() keys on blockDim.x.  The parallelism of a batch is across
// problems: with one wavefront each a compute unit holds as many problems as their LDS allows.  The apply item is written
// for PSD_GAPPLY_NT = 128 threads through PSD_PAR_FOR and its tile in LDS is 128 wide; 64 threads walk it in two strides,
// the arithmetic of every line is the same.  The difference between the two sweep forms at small n has not been
// measured.  The single call with PSD_GSCAN=0, trains off and PSD_HESS_SERIAL=1 does the same arithmetic in the same
// order.  Nothing is shared between workgroups: no atomics, no waits, and a problem's result does not depend on where it
// stands in a batch.
//
// Hand-offs between the lanes through device memory (the rotation lists and their counts, the descriptor, the state, dG,
// xscr, the window store followed by the off-window update, the Case II / III rotations on HBM) are ordered by
// PSD_SYNC(), as in psd_zgbqz.h.  Every loop is bounded: the tick loop by `cap` (the bound of giterate_dev's host loop),
// past which the problem ends with PSD_ZB_TICKCAP; a list overflow ends it with PSD_LIST_OVERFLOW (psd_gdesc_write).
//
// LDS of psd_gbqz: the step's window image and scratch; the apply item's list and tile reuse that area, which is idle
// between steps.
#pragma once
#include "psd_rgz.h"
#include "psd_bhess.h"
#include "psd_zbqz.h"

// Largest order the one-workgroup / one-wavefront-per-problem kernels of this file take: the cap the other batch kernels
// start from (PSD_BH_NMAX, PSD_ZB_NMAX).  What has and has not been measured for it: gb_nmax, psd_gbatch_host.inl.
#define PSD_GB_NMAX 128

// LDS of the apply items: the rotation list of one owner, then the tile (as giterate_dev's lds_apply)
PSD_HD size_t psd_gbqz_apply_lds_bytes() {
    return PSD_GTR_LDS_BYTES + (size_t)32 * (PSD_GAPPLY_NT + 1) * sizeof(double);
}

// A: [nb][p][n][n] internal order; Q: [nb][p][n][n] or nullptr (set to the identity here, then accumulated);
// S: [p] in internal order, S[0] true.  grid = nb, PSD_HESS_NT threads, psd_bhess_lds_bytes(n)
PSD_KERNEL psd_gbhess1(double* A, double* Q, const unsigned char* S, int n, int p) {
    PSD_LDS_DECL;
    const size_t nn = (size_t)n * n;
    double* Aq = A + (size_t)PSD_BLOCK_X * p * nn;
    double* Qq = Q ? Q + (size_t)PSD_BLOCK_X * p * nn : nullptr;
    double* v = (double*)psd_lds + PSD_HESS_NT + n + 8;  // [0] = tau, [1..m-1] = v (the vbuf of psd_hess_refl_body)
    if (Qq) {
        for (int j = 1; j <= p; ++j)
            for (int c = 1; c <= n; ++c) psd_set_identity_body(Qq, n, c, j);
        PSD_SYNC();
    }
    const int nR = (n + PSD_HESS_RS - 1) / PSD_HESS_RS;
    const int nLm = (n + 3) / 4;
    for (int l = p; l >= 2; --l) {
        double* Al = Aq + (size_t)(l - 1) * nn;
        double* Am = Aq + (size_t)(l - 2) * nn;
        double* Ql = Qq ? Qq + (size_t)(l - 1) * nn : nullptr;
        const bool rq = S[l - 1] == 0;
        const int mrows = (S[l - 2] != 0) ? 0 : 1;
        // (the blocks of one of these launches touch disjoint entries, and the three matrices are different ones)
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1) {
                for (int i = 1; i <= n - 1; ++i) {
                    psd_hess_refl_body(Al, n, i, i, v, (double*)nullptr);
                    PSD_SYNC();
                    // the blocks of psd_hess_apply2: left on A_l, right on Q_l, then the neighbour A_{l-1}
                    const int nL = (n - i + 3) / 4;
                    for (int b = 0; b < nL; ++b) {
                        psd_hess_apply_body(Al, nullptr, n, i, i + 1, v, nL, b);
                        PSD_SYNC();  // (the next block reuses the reduction area)
                    }
                    if (Ql)
                        for (int b = 0; b < nR; ++b) {
                            psd_hess_apply_body(nullptr, Ql, n, i, i + 1, v, nL, nL + b);
                            PSD_SYNC();
                        }
                    if (mrows == 0) {
                        for (int b = 0; b < nR; ++b) {
                            psd_hess_apply_body(nullptr, Am, n, i, 1, v, 0, b);
                            PSD_SYNC();
                        }
                    } else {
                        for (int b = 0; b < nLm; ++b) {
                            psd_hess_apply_body(Am, nullptr, n, i, 1, v, nLm, b);
                            PSD_SYNC();
                        }
                    }
                }
                for (int c = 1; c <= n; ++c) psd_tril_zero_body(Al, n, c);
                PSD_SYNC();
            }
            if (rq) {  // before the chain and, undone, behind it
                for (int c = 1; c <= n; ++c) psd_antitranspose_body(Al, n, c);
                for (int k = 1; k <= n; ++k) psd_flip_body(Am, n, mrows, k);
                if (Ql)
                    for (int k = 1; k <= n; ++k) psd_flip_body(Ql, n, 0, k);
                PSD_SYNC();
            }
        }
    }
}

struct psd_gbqz_args {
    double* H;  // [nb][p][n][n] internal order, the Hessenberg factor first
    double* Z;  // [nb][p][n][n] or nullptr
    const unsigned char* S;  // [p] internal order, one signature for the batch
    psd_gstate* st;          // [nb]
    psd_gapply_desc* desc;   // [nb]
    psd_gtr* tr;             // [nb][p][PSD_GTR_CAP]
    int* cnt;                // [nb][p]
    psd_gtr* dG;             // [nb][n + 2]
    double* xscr;            // [nb][16 p + 16]
    psd_z* alpha;            // [nb][n]
    double* beta;            // [nb][n]
    int* ascale;             // [nb][n]
    int* log;                // [nb][3 maxlog]
    int* infos;              // [nb]
    int n, p, wantT, wantZ, W, maxitfac, maxlog, hessmode;
    long long cap;  // ticks after which a problem gives up with PSD_ZB_TICKCAP
};

PSD_HD size_t psd_gbqz_xscr_doubles(int p) { return (size_t)16 * p + 16; }

PSD_D psd_gparams psd_gbqz_params(const psd_gbqz_args& A, int q) {
    const size_t nn = (size_t)A.n * A.n;
    psd_gparams P;
    P.H = A.H + (size_t)q * A.p * nn;
    P.Z = A.Z ? A.Z + (size_t)q * A.p * nn : nullptr;
    P.S = A.S;
    P.st = A.st + q;
    P.desc = A.desc + q;
    P.tr = A.tr + (size_t)q * A.p * PSD_GTR_CAP;
    P.cnt = A.cnt + (size_t)q * A.p;
    P.dG = A.dG + (size_t)q * (A.n + 2);
    P.alpha = A.alpha + (size_t)q * A.n;
    P.beta = A.beta + (size_t)q * A.n;
    P.ascale = A.ascale + (size_t)q * A.n;
    P.log = A.log + (size_t)q * 3 * A.maxlog;
    P.xscr = A.xscr + (size_t)q * psd_gbqz_xscr_doubles(A.p);
    P.cst = nullptr;
    P.cep = nullptr;
    P.tshift = nullptr;
    P.tick = 0;
    P.zlo = 1;
    P.zhi = A.p;
    P.gcoff = P.gtaboff = 0;  // (the single-wave sweep)
    return P;
}

// grid = problems of the group, one wavefront each; LDS = max(step_lds_bytes(p, W, 8), psd_gbqz_apply_lds_bytes())
PSD_KERNEL_B(PSD_STEP_NT) psd_gbqz(psd_gbqz_args A) {
    const int q = PSD_BLOCK_X;
    const int n = A.n, p = A.p;
    psd_gparams P = psd_gbqz_params(A, q);
    psd_gq_init_body(P, n, p, A.wantT, A.wantZ, A.W, A.maxitfac, A.maxlog, A.hessmode, 1, 0);
    PSD_SYNC();
    const int tiles = (n + PSD_GAPPLY_NT - 1) / PSD_GAPPLY_NT;
    const int dtiles = (n + PSD_STEP_NT - 1) / PSD_STEP_NT;
    const int nroles = A.wantZ ? 3 : 2;
    for (long long tick = 0;; ++tick) {
        if (tick > A.cap) {
            PSD_ONE {
                P.st->info = PSD_ZB_TICKCAP;
                P.st->phase = PSD_GPH_DONE;
            }
            PSD_SYNC();
            break;
        }
        P.tick = (int)tick;
        psd_gq_step_body(P);
        PSD_SYNC();
        if (P.desc->active) {
            // rows of H_l, columns of H_l, columns of Z_l: the grid (tiles, p, 3) of psd_gq_apply
            for (int role = 0; role < nroles; ++role)
                for (int l = 1; l <= p; ++l)
                    for (int bx = 0; bx < tiles; ++bx) {
                        psd_gq_apply_item(P, n, p, role, bx, l);
                        PSD_SYNC();  // (the list and the tile in LDS are reused by the next item)
                    }
            if (P.desc->defer_run) {
                for (int bx = 0; bx < dtiles; ++bx) psd_gq_defer_body(P, n, bx);
                PSD_SYNC();
            }
        }
        if (P.st->phase == PSD_GPH_DONE) break;
    }
    PSD_ONE { A.infos[q] = P.st->info; }
}
