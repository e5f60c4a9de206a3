// Batched complex SIGNED periodic Hessenberg reduction and QZ iteration: _phessenberg!(A, S) and pschur!(H1, Hs, S) for
// ComplexF64 (generalized.jl:988-1082, 166-931) for many small problems of one shape (n, p) and ONE signature S in one
// launch per stage — the kernels behind psd_z_gphessenberg_batch / psd_z_gpschur_batch (psd_zgbatch_host.inl).  The
// signed counterpart of psd_zbhess.h / psd_zbqz.h, built from the bodies of psd_zgz.h and psd_zhess.h.
//
// psd_zgbhess1: ONE workgroup owns ONE problem and walks stage 1 of zsghess_dev (generalized.jl:988-1033): for l = p..2
// the anti-transpose of A_l and the flips of A_{l-1} and Q_l when !S[l], the reflector chain of A_l — psd_zhess_refl_body,
// then the blocks of psd_zhess_apply_body on A_l (left), Q_l (right) and the neighbour A_{l-1} (right for S[l-1], left
// otherwise) —, psd_ztril_zero, and the flips undone.  A workgroup barrier stands where a launch boundary stood; the
// reflector that the single call hands from launch to launch through device memory lives in LDS.  The single call
// computes the next reflector behind block 0 of the update; the column it reads is touched by that block alone, so the
// reflector taken after all blocks is the same one, bit for bit.
//
// psd_zgbqz: ONE wavefront carries ONE problem from psd_zgq_init_body's state to PSD_GPH_DONE without leaving the
// kernel.  A tick is what zgiterate_dev launches per tick without trains: psd_zgq_step_body (decisions, Cases II / III
// directly on HBM, one window chased out of LDS), psd_zgq_apply_item over the roles, factors and tiles of psd_zgq_apply,
// the deferred side of H_1 (psd_zgq_defer_body); behind the last tick the phase passes for l = p..2
// (psd_zgq_phase_body).  With hessmode = 1 it is stage 2 of the reduction in its serial form (psd_zgq_hess_window, what
// PSD_HESS_SERIAL=1 selects in the single call), with hessmode = 0 the iteration.  No trains (train_want = 1, no cursor
// states: PSD_GPH_TWAIT is never entered), no pipeline over the factors: the single call with both off does the same
// arithmetic in the same order.  Nothing is shared between workgroups: no atomics, no waits, and a problem's result does
// not depend on where it stands in a batch.
//
// Hand-offs between the lanes through device memory (the rotation lists and their counts, the descriptor, the state, dG,
// the window store followed by the off-window update, the Case II / III rotations on HBM) are ordered by PSD_SYNC(), as
// in psd_zbqz.h.
//
// LDS of psd_zgbqz: the step's window image and scratch; the apply tile reuses that area, which is idle between steps.
#pragma once
#include "psd_zgz.h"
#include "psd_zbqz.h"

// LDS of the apply items: the rotation list of one owner, then the tile (as zgiterate_dev's lds_apply)
PSD_HD size_t psd_zgbqz_apply_lds_bytes() {
    return sizeof(psd_ztr) * PSD_GTR_CAP + (size_t)32 * (PSD_ZAPPLY_NT + 1) * sizeof(psd_z);
}

// A: [nb][p][n][n] internal order; Q: [nb][p][n][n] or nullptr (set to the identity here, then accumulated);
// S: [p] in internal order, S[0] true.  grid = nb, PSD_HESS_NT threads, psd_zbhess_lds_bytes(n)
PSD_KERNEL psd_zgbhess1(psd_z* A, psd_z* Q, const unsigned char* S, int n, int p) {
    PSD_LDS_DECL;
    const size_t nn = (size_t)n * n;
    psd_z* Aq = A + (size_t)PSD_BLOCK_X * p * nn;
    psd_z* Qq = Q ? Q + (size_t)PSD_BLOCK_X * p * nn : nullptr;
    psd_z* v = (psd_z*)psd_lds + PSD_HESS_NT + n + 8;  // [0] = tau, [1..m-1] = v (the vbuf of psd_zhess_refl_body)
    if (Qq) {
        for (int j = 1; j <= p; ++j)
            for (int c = 1; c <= n; ++c) psd_zset_identity_body(Qq, n, c, j);
        PSD_SYNC();
    }
    const int nR = (n + PSD_HESS_RS - 1) / PSD_HESS_RS;
    const int nLm = (n + 3) / 4;
    for (int l = p; l >= 2; --l) {
        psd_z* Al = Aq + (size_t)(l - 1) * nn;
        psd_z* Am = Aq + (size_t)(l - 2) * nn;
        psd_z* Ql = Qq ? Qq + (size_t)(l - 1) * nn : nullptr;
        const bool rq = S[l - 1] == 0;
        const int mrows = (S[l - 2] != 0) ? 0 : 1;
        // (the blocks of one of these launches touch disjoint entries, and the three matrices are different ones)
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1) {
                for (int i = 1; i <= n - 1; ++i) {
                    psd_zhess_refl_body(Al, n, i, i, v, (psd_z*)nullptr);
                    PSD_SYNC();
                    // the blocks of psd_zhess_apply2: left on A_l, right on Q_l, then the neighbour A_{l-1}
                    const int nL = (n - i + 3) / 4;
                    for (int b = 0; b < nL; ++b) {
                        psd_zhess_apply_body(Al, nullptr, n, i, i + 1, v, nL, b);
                        PSD_SYNC();  // (the next block reuses the reduction area)
                    }
                    if (Ql)
                        for (int b = 0; b < nR; ++b) {
                            psd_zhess_apply_body(nullptr, Ql, n, i, i + 1, v, nL, nL + b);
                            PSD_SYNC();
                        }
                    if (mrows == 0) {
                        for (int b = 0; b < nR; ++b) {
                            psd_zhess_apply_body(nullptr, Am, n, i, 1, v, 0, b);
                            PSD_SYNC();
                        }
                    } else {
                        for (int b = 0; b < nLm; ++b) {
                            psd_zhess_apply_body(Am, nullptr, n, i, 1, v, nLm, b);
                            PSD_SYNC();
                        }
                    }
                }
                for (int c = 1; c <= n; ++c) psd_ztril_zero_body(Al, n, c);
                PSD_SYNC();
            }
            if (rq) {  // before the chain and, undone, behind it
                for (int c = 1; c <= n; ++c) psd_zantitranspose_body(Al, n, c);
                for (int k = 1; k <= n; ++k) psd_zflip_body(Am, n, mrows, k);
                if (Ql)
                    for (int k = 1; k <= n; ++k) psd_zflip_body(Ql, n, 0, k);
                PSD_SYNC();
            }
        }
    }
}

struct psd_zgbqz_args {
    psd_z* H;  // [nb][p][n][n] internal order, the Hessenberg factor first
    psd_z* Z;  // [nb][p][n][n] or nullptr
    const unsigned char* S;  // [p] internal order, one signature for the batch
    psd_zgstate* st;         // [nb]
    psd_gapply_desc* desc;   // [nb]
    psd_ztr* tr;             // [nb][p][PSD_GTR_CAP]
    int* cnt;                // [nb][p]
    psd_ztr* dG;             // [nb][n + 2]
    psd_z* alpha;            // [nb][n]
    double* beta;            // [nb][n]
    int* ascale;             // [nb][n]
    int* log;                // [nb][3 maxlog]
    int* infos;              // [nb]
    int n, p, wantT, wantZ, W, maxitfac, maxlog, hessmode;
    long long cap;  // ticks after which a problem gives up with PSD_ZB_TICKCAP
};

PSD_D psd_zgparams psd_zgbqz_params(const psd_zgbqz_args& A, int q) {
    const size_t nn = (size_t)A.n * A.n;
    psd_zgparams P;
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
    P.cst = nullptr;
    P.cep = nullptr;
    P.tshift = nullptr;
    P.tick = 0;
    P.zlo = 1;
    P.zhi = A.p;
    return P;
}

// grid = problems of the group, one wavefront each; LDS = max(step_lds_bytes(p, W, 16), psd_zgbqz_apply_lds_bytes())
PSD_KERNEL_B(PSD_STEP_NT) psd_zgbqz(psd_zgbqz_args A) {
    const int q = PSD_BLOCK_X;
    const int n = A.n, p = A.p;
    psd_zgparams P = psd_zgbqz_params(A, q);
    psd_zgq_init_body(P, n, p, A.wantT, A.wantZ, A.W, A.maxitfac, A.maxlog, A.hessmode, 1, 0);
    PSD_SYNC();
    const int tiles = (n + PSD_ZAPPLY_NT - 1) / PSD_ZAPPLY_NT;
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
        psd_zgq_step_body(P);
        PSD_SYNC();
        if (P.desc->active) {
            // rows of H_l, columns of H_l, columns of Z_l: the grid (tiles, p, 3) of psd_zgq_apply
            for (int role = 0; role < nroles; ++role)
                for (int l = 1; l <= p; ++l)
                    for (int bx = 0; bx < tiles; ++bx) {
                        psd_zgq_apply_item(P, n, p, role, bx, l);
                        PSD_SYNC();  // (the list and the tile in LDS are reused by the next item)
                    }
            if (P.desc->defer_run) {
                for (int bx = 0; bx < dtiles; ++bx) psd_zgq_defer_body(P, n, bx);
                PSD_SYNC();
            }
        }
        if (P.st->phase == PSD_GPH_DONE) break;
    }
    const int info = P.st->info;
    if (!A.hessmode && info == 0 && A.wantT) {  // generalized.jl:860-908
        for (int l = p; l >= 2; --l)
            for (int j = 1; j <= n; ++j) {
                psd_zgq_phase_body(P, n, l, A.wantZ, j);
                PSD_SYNC();
            }
    }
    PSD_ONE { A.infos[q] = info; }
}
