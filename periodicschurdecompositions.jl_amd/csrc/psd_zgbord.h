// Batched eigenvalue reordering, ComplexF64, signed signature: ordschur!(P::GeneralizedPeriodicSchur, select)
// (ordschur.jl:11-96, sylswap.jl:638-764) for many small generalized periodic Schur forms of one shape and ONE signature
// in one launch — the follow-up of psd_z_gpschur_batch (psd_zgbatch_host.inl) and the signed counterpart of psd_zbord
// (psd_zbord.h).
//
// One wavefront carries one problem from the first scan step to the last swap without leaving the kernel.  A tick is
// what zgordschur_dev launches per tick in its serial form (one selected eigenvalue at a time): psd_zgord_step_body (scan,
// one window of signed 1x1 swaps out of LDS, stability tests, rotation lists) and psd_zgq_apply_item over the roles,
// factors and tiles of psd_zgq_apply (the window's rotation lists on the off-window rows and columns of the factors and
// the columns of Z_m).  The launches become loops over their block indices; the bodies are the single driver's, as they
// are.  The roles of a window touch disjoint entries, so the order of the items does not matter: the serial single call
// does the same arithmetic.  The parallelism is across problems, as in psd_zbord and psd_zgbqz.  Nothing is shared
// between workgroups: no atomics, no waits, and a problem's result does not depend on where it stands in a batch.
//
// Hand-offs between the lanes through device memory (the window store, the rotation lists and their counts, the
// descriptor, the state, the off-window update) are ordered by PSD_SYNC(), which drains the wavefront's stores before its
// next loads (psd_bord.h).
//
// LDS: the step's window image and scratch; the apply tile reuses that area between steps (psd_zgord_step_body reloads
// its window on every call and keeps nothing in LDS across calls).
#pragma once
#include "psd_zgord.h"
#include "psd_zgbqz.h"

#define PSD_ZGBORD_WMIN 4  // least window PSD_BORD_W may ask of psd_zgbord (the narrowest candidate of zgordschur_dev)

// psd_ostate::info of a problem that ran into the window bound (never reached: every window makes at least one swap)
#define PSD_ZGBORD_WINCAP (-7781)

struct psd_zgbord_args {
    psd_z* H;  // [nb][p][n][n] internal right order, the Schur factor first
    psd_z* Z;  // [nb][p][n][n] or nullptr
    const unsigned char* S;  // [p] internal order, one signature for the batch
    psd_ostate* st;          // [nb]
    psd_gapply_desc* desc;   // [nb]
    psd_ztr* tr;             // [nb][p][PSD_GTR_CAP]
    int* cnt;                // [nb][p]
    const unsigned char* select;  // [nb][n]
    psd_z* alpha;            // [nb][n]
    double* beta;            // [nb][n]
    int* ascale;             // [nb][n]
    int* infos;              // [nb]
    int n, p, wantZ, W;
    int maxwin;  // windows after which a problem gives up with PSD_ZGBORD_WINCAP
};

// the fields the ord, apply and eigenvalue bodies read, as psd_zgbqz_params and zgordschur_dev set them: every Z_m is
// this problem's; the iteration's state, deferral list, log and cursor fields are never read here
PSD_D psd_zgoparams psd_zgbord_params(const psd_zgbord_args& A, int q) {
    const size_t nn = (size_t)A.n * A.n;
    psd_zgoparams O;
    psd_zgparams& P = O.z;
    P.H = A.H + (size_t)q * A.p * nn;
    P.Z = A.Z ? A.Z + (size_t)q * A.p * nn : nullptr;
    P.S = A.S;
    P.st = nullptr;
    P.desc = A.desc + q;
    P.tr = A.tr + (size_t)q * A.p * PSD_GTR_CAP;
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
    O.st = A.st + q;
    O.select = A.select + (size_t)q * A.n;
    return O;
}

// grid = problems of the group, one wavefront each; LDS = max(zgord_lds_bytes(p, W), psd_zgbqz_apply_lds_bytes())
PSD_KERNEL_B(PSD_STEP_NT) psd_zgbord(psd_zgbord_args A) {
    const int q = PSD_BLOCK_X;
    const int n = A.n, p = A.p;
    const psd_zgoparams O = psd_zgbord_params(A, q);
    PSD_ONE {  // (psd_zgord_init)
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
                O.st->info = PSD_ZGBORD_WINCAP;
                O.st->phase = PSD_OPH_DONE;
            }
            PSD_SYNC();
            break;
        }
        psd_zgord_step_body(O);
        PSD_SYNC();
        if (O.z.desc->active) {
            // rows of T_l, columns of T_l, columns of Z_l: the grid (tiles, p, 3) of psd_zgq_apply
            for (int role = 0; role < nroles; ++role)
                for (int l = 1; l <= p; ++l)
                    for (int bx = 0; bx < tiles; ++bx) {
                        psd_zgq_apply_item(O.z, n, p, role, bx, l);
                        PSD_SYNC();  // (the list and the tile in LDS are reused by the next item)
                    }
        }
        if (O.st->phase == PSD_OPH_DONE) break;
    }
    const int info = O.st->info;
    PSD_ONE { A.infos[q] = info; }
}

// psd_zgord_values for a batch: grid = (ceil(n / 64), nb), 64 threads.  Problems with a non-zero code are skipped.
PSD_KERNEL psd_zgbord_values(psd_zgbord_args A) {
    const int q = PSD_BLOCK_Y;
    if (A.infos[q] != 0) return;
    const psd_zgoparams O = psd_zgbord_params(A, q);
    const int NT = PSD_NTHREADS;
    PSD_PAR_FOR(t, NT) {
        const int j = 1 + PSD_BLOCK_X * NT + t;
        if (j <= A.n) psd_zgord_value_at(O.z, A.n, A.p, j);
    }
}
