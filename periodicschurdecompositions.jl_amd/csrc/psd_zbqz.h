// Batched complex periodic QZ iteration (all signatures +1): pschur!(H1, Hs, S) for ComplexF64 (generalized.jl:166-931)
// for many small Hessenberg-triangular problems of one shape in one launch — the iteration behind psd_z_pschur_batch
// (psd_zbatch_host.inl).
//
// One wavefront carries one problem from psd_zq_init's state to PSD_ZPH_DONE without leaving the kernel.  A tick is
// what ziterate_dev launches per tick with one cursor: psd_zq_step_body (decisions and one window chased out of LDS),
// psd_zq_apply_item over the roles, owners and tiles of psd_zq_apply (the window's rotation lists on the off-window
// rows of H_m, columns of H_{m-1} and columns of Z_m), the deferred side of H_1 (psd_zq_defer_body); behind the last
// tick the phase passes for l = p..2 (psd_zq_phase_body).  The launches become loops over their block indices.  No
// trains, no scan chase, no slices: the single call with trains off and the one-wave chase does the same arithmetic in
// the same order.  The parallelism is across problems, as in psd_zbhess and psd_bord.  Nothing is shared between
// workgroups: no atomics, no waits, and a problem's result does not depend on where it stands in a batch.
//
// Hand-offs between the lanes through device memory (the rotation lists and their counts, the descriptor, the state,
// dG, the window store followed by the off-window update) are ordered by PSD_SYNC(), which drains the wavefront's
// stores before its next loads (psd_bord.h).
//
// LDS: the step's window image and scratch; the apply tile reuses that area, which is idle between steps.
#pragma once
#include "psd_zqz.h"
#include "psd_zbhess.h"

// psd_zstate::info of a problem whose tick loop ran into its bound (the host loop's `cap`): PSD_INFO_RUNTIME + 0xfffe
#define PSD_ZB_TICKCAP (-7778)

struct psd_zbqz_args {
    psd_z* H;  // [nb][p][n][n] internal order, the Hessenberg factor first
    psd_z* Z;  // [nb][p][n][n] or nullptr
    psd_zstate* st;         // [nb]
    psd_zapply_desc* desc;  // [nb]
    psd_ztr* tr;            // [nb][p][PSD_ZTR_CAP]
    int* cnt;               // [nb][p]
    psd_ztr* dG;            // [nb][n + 2]
    psd_z* alpha;           // [nb][n]
    double* beta;           // [nb][n]
    int* ascale;            // [nb][n]
    int* log;               // [nb][3 maxlog]
    int* infos;             // [nb]
    int n, p, wantT, wantZ, W, maxitfac, maxlog;
    long long cap;  // ticks after which a problem gives up with PSD_ZB_TICKCAP
};

// bytes of LDS: the step's (step_lds_bytes(p, W, 16), passed in) or the apply tile's, whichever is larger
PSD_HD size_t psd_zbqz_apply_lds_bytes(int W) {
    return PSD_ZTR_LDS_BYTES + (size_t)((W + 2 < 32) ? (W + 2) : 32) * (PSD_ZAPPLY_NT + 1) * sizeof(psd_z);
}

PSD_D psd_zparams psd_zbqz_params(const psd_zbqz_args& A, int q) {
    const size_t nn = (size_t)A.n * A.n;
    psd_zparams P;
    P.H = A.H + (size_t)q * A.p * nn;
    P.Z = A.Z ? A.Z + (size_t)q * A.p * nn : nullptr;
    P.st = A.st + q;
    P.desc = A.desc + q;
    P.tr = A.tr + (size_t)q * A.p * PSD_ZTR_CAP;
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
    P.zcoff = P.zc3off = 0;
    P.zslG = 1;
    P.zslmem = nullptr;
    P.zslerr = nullptr;
    P.zcdefer = 0;
    return P;
}

// grid = problems of the group, one wavefront each; LDS = max(step_lds_bytes(p, W, 16), psd_zbqz_apply_lds_bytes(W))
PSD_KERNEL_B(PSD_STEP_NT) psd_zbqz(psd_zbqz_args A) {
    const int q = PSD_BLOCK_X;
    const int n = A.n, p = A.p;
    psd_zparams P = psd_zbqz_params(A, q);
    psd_zq_init_body(P, n, p, A.wantT, A.wantZ, A.W, A.maxitfac, A.maxlog, 1, 0);
    PSD_SYNC();
    const int tiles = (n + PSD_ZAPPLY_NT - 1) / PSD_ZAPPLY_NT;
    const int dtiles = (n + PSD_STEP_NT - 1) / PSD_STEP_NT;
    const int nroles = A.wantZ ? 3 : 2;
    for (long long tick = 0;; ++tick) {
        if (tick > A.cap) {
            PSD_ONE {
                P.st->info = PSD_ZB_TICKCAP;
                P.st->phase = PSD_ZPH_DONE;
            }
            PSD_SYNC();
            break;
        }
        P.tick = (int)tick;
        psd_zq_step_body(P);
        PSD_SYNC();
        if (P.desc->active) {
            // rows of H_m, columns of H_{m-1}, columns of Z_m: the grid (tiles, p, 3) of psd_zq_apply
            for (int role = 0; role < nroles; ++role)
                for (int m = 1; m <= p; ++m)
                    for (int bx = 0; bx < tiles; ++bx) {
                        psd_zq_apply_item(P, n, p, role, bx, m);
                        PSD_SYNC();  // (the list and the tile in LDS are reused by the next item)
                    }
            if (P.desc->defer_run) {
                for (int bx = 0; bx < dtiles; ++bx) psd_zq_defer_body(P, n, bx);
                PSD_SYNC();
            }
        }
        if (P.st->phase == PSD_ZPH_DONE) break;
    }
    const int info = P.st->info;
    if (info == 0 && A.wantT) {  // generalized.jl:860-908
        for (int l = p; l >= 2; --l)
            for (int j = 1; j <= n; ++j) {
                psd_zq_phase_body(P, n, l, A.wantZ, j);
                PSD_SYNC();
            }
    }
    PSD_ONE { A.infos[q] = info; }
}
