// Batched eigenvalue reordering, ComplexF64, all-true signature: ordschur!(P, select) (ordschur.jl:11-73) for many small
// periodic Schur forms of one shape in one launch — the follow-up of psd_z_pschur_batch (psd_zbatch_host.inl) and the
// complex counterpart of psd_bord (psd_bord.h).
//
// One wavefront carries one problem from the first scan step to the last swap without leaving the kernel.  A tick is
// what zordschur_dev launches per tick in its serial form (one selected eigenvalue at a time): psd_zord_step_body (scan,
// one window of 1x1 swaps out of LDS, stability tests, rotation lists) and psd_zq_apply_item over the roles, owners and
// tiles of psd_zq_apply (the window's rotation lists on the off-window columns of T_m, rows of T_{m-1} and rows of Z_m).
// The launches become loops over their block indices; the bodies are the single driver's, as they are.  The row role and
// the column role of a window touch disjoint entries, so the order of the items does not matter: the serial single call
// does the same arithmetic.  The parallelism is across problems, as in psd_bord and psd_zbqz.  Nothing is shared between
// workgroups: no atomics, no waits, and a problem's result does not depend on where it stands in a batch.
//
// Hand-offs between the lanes through device memory (the window store, the rotation lists and their counts, the
// descriptor, the state, the off-window update) are ordered by PSD_SYNC(), which drains the wavefront's stores before its
// next loads (psd_bord.h).
//
// LDS: the step's window image and scratch; the apply tile reuses that area between steps (psd_zord_step_body reloads its
// window on every call and keeps nothing in LDS across calls).
#pragma once
#include "psd_zord.h"
#include "psd_zbqz.h"

#define PSD_ZBORD_WMIN 4  // least window PSD_BORD_W may ask of psd_zbord (the narrowest candidate of zordschur_dev)

// psd_ostate::info of a problem that ran into the window bound (never reached: every window makes at least one swap)
#define PSD_ZBORD_WINCAP (-7779)

struct psd_zbord_args {
    psd_z* H;  // [nb][p][n][n] internal right order, the Schur factor first
    psd_z* Z;  // [nb][p][n][n] or nullptr
    psd_ostate* st;         // [nb]
    psd_zapply_desc* desc;  // [nb]
    psd_ztr* tr;            // [nb][p][PSD_ZTR_CAP]
    int* cnt;               // [nb][p]
    const unsigned char* select;  // [nb][n]
    psd_z* alpha;           // [nb][n]
    double* beta;           // [nb][n]
    int* ascale;            // [nb][n]
    int* infos;             // [nb]
    int n, p, wantZ, W;
    int maxwin;  // windows after which a problem gives up with PSD_ZBORD_WINCAP
};

// the fields the ord and apply bodies read, as psd_zbqz_params and zordschur_dev set them: every Z_m is this problem's,
// no slices, no deferral
PSD_D psd_oparams psd_zbord_params(const psd_zbord_args& A, int q) {
    const size_t nn = (size_t)A.n * A.n;
    psd_oparams O;
    psd_zparams& P = O.z;
    P.H = A.H + (size_t)q * A.p * nn;
    P.Z = A.Z ? A.Z + (size_t)q * A.p * nn : nullptr;
    P.st = nullptr;
    P.desc = A.desc + q;
    P.tr = A.tr + (size_t)q * A.p * PSD_ZTR_CAP;
    P.cnt = A.cnt + (size_t)q * A.p;
    P.dG = nullptr;
    P.alpha = A.alpha + (size_t)q * A.n;
    P.beta = A.beta + (size_t)q * A.n;
    P.ascale = A.ascale + (size_t)q * A.n;
    P.log = nullptr;
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
    O.st = A.st + q;
    O.select = A.select + (size_t)q * A.n;
    return O;
}

// grid = problems of the group, one wavefront each; LDS = max(ord_lds_bytes(p, W), psd_zbqz_apply_lds_bytes(W))
PSD_KERNEL_B(PSD_STEP_NT) psd_zbord(psd_zbord_args A) {
    const int q = PSD_BLOCK_X;
    const int n = A.n, p = A.p;
    const psd_oparams O = psd_zbord_params(A, q);
    PSD_ONE {  // (psd_zord_init)
        psd_ostate st;
        st.n = n; st.p = p; st.wantZ = A.wantZ; st.W = A.W;
        st.phase = PSD_OPH_SCAN; st.info = 0;
        st.j = 0; st.js = 0; st.here = 0; st.nswaps = 0; st.nwindows = 0;
        *O.st = st;
        O.z.desc->active = 0;
        O.z.desc->defer_run = 0;
    }
    PSD_SYNC();
    const int tiles = (n + PSD_ZAPPLY_NT - 1) / PSD_ZAPPLY_NT;
    const int nroles = A.wantZ ? 3 : 2;
    for (int win = 0;; ++win) {
        if (win > A.maxwin) {
            PSD_ONE {
                O.st->info = PSD_ZBORD_WINCAP;
                O.st->phase = PSD_OPH_DONE;
            }
            PSD_SYNC();
            break;
        }
        psd_zord_step_body(O);
        PSD_SYNC();
        if (O.z.desc->active) {
            // columns of T_m, rows of T_{m-1}, rows of Z_m: the grid (tiles, p, 3) of psd_zq_apply
            for (int role = 0; role < nroles; ++role)
                for (int m = 1; m <= p; ++m)
                    for (int bx = 0; bx < tiles; ++bx) {
                        psd_zq_apply_item(O.z, n, p, role, bx, m);
                        PSD_SYNC();  // (the list and the tile in LDS are reused by the next item)
                    }
        }
        if (O.st->phase == PSD_OPH_DONE) break;
    }
    const int info = O.st->info;
    PSD_ONE { A.infos[q] = info; }
}

// psd_zord_values for a batch: grid = (ceil(n / 64), nb), 64 threads.  Problems with a non-zero code are skipped.
PSD_KERNEL psd_zbord_values(psd_zbord_args A) {
    const int q = PSD_BLOCK_Y;
    if (A.infos[q] != 0) return;
    const psd_oparams O = psd_zbord_params(A, q);
    const int NT = PSD_NTHREADS;
    PSD_PAR_FOR(t, NT) {
        const int j = 1 + PSD_BLOCK_X * NT + t;
        if (j <= A.n) psd_zord_value_at(O.z, A.n, A.p, j);
    }
}
