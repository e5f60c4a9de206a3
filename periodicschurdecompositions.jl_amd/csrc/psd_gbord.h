// Batched eigenvalue reordering, Float64, signed signature: ordschur!(P::GeneralizedPeriodicSchur, select) with 1x1 and
// 2x2 blocks (rordschur.jl:3-132 with the signed block swaps of sylswap.jl:197-538) for many small real generalized
// periodic Schur forms of one shape and ONE signature in one launch — the follow-up of psd_d_gpschur_batch
// (psd_gbatch_host.inl) and the signed counterpart of psd_bord (psd_bord.h).
//
// psd_gbord is psd_bord_body with its signed flag: one wavefront carries one problem from the first scan to the last
// swap; the flags SL of the window's Sylvester systems and the sides of the off-window update follow the signature, as
// in psd_rord_step and psd_rord_apply, and the swap bodies see the signature through psd_roparams::S.  Nothing is
// shared between workgroups: no atomics, no waits, and a problem's result does not depend on where it stands in a batch.
// psd_gbord_values and psd_gbord_cleanup are psd_grord_values / psd_grord_cleanup per problem: the eigenvalues in the
// scaled form (alpha complex, beta, the scaling), the all-true signature included.
#pragma once
#include "psd_bord.h"
#include "psd_grord.h"

struct psd_gbord_args {
    psd_bord_args b;         // (wr and wi are not used)
    const unsigned char* S;  // [p] internal order, one signature for the batch
    psd_z* alpha;            // [nb][n]
    double* beta;            // [nb][n]
    int* ascale;             // [nb][n]
};

PSD_D psd_roparams psd_gbord_params(const psd_gbord_args& A, int q) {
    psd_roparams P = psd_bord_params(A.b, q);
    P.S = A.S;
    P.alpha = A.alpha + (size_t)q * A.b.n;
    P.beta = A.beta + (size_t)q * A.b.n;
    P.ascale = A.ascale + (size_t)q * A.b.n;
    return P;
}

// grid = problems of the group, one wavefront each; LDS = rord_lds_bytes(p, W)
PSD_KERNEL_B(PSD_STEP_NT) psd_gbord(psd_gbord_args A) {
    const int q = PSD_BLOCK_X;
    psd_bord_body<true>(psd_gbord_params(A, q), A.b.n, A.b.p, A.b.wantZ, A.b.W, A.b.maxwin, A.b.infos + q);
}

// psd_grord_values for a batch: grid = (ceil(n / 64), nb), 64 threads.  Problems with a non-zero code are skipped.
PSD_KERNEL psd_gbord_values(psd_gbord_args A) {
    const int q = PSD_BLOCK_Y;
    if (A.b.infos[q] != 0) return;
    const psd_roparams P = psd_gbord_params(A, q);
    const int NT = PSD_NTHREADS;
    PSD_PAR_FOR(t, NT) {
        const int j = 1 + PSD_BLOCK_X * NT + t;
        if (j <= A.b.n) psd_grord_value_at(P, A.b.n, A.b.p, j);
    }
}

// psd_grord_cleanup for a batch: grid = (n, nb)
PSD_KERNEL psd_gbord_cleanup(psd_gbord_args A) {
    const int q = PSD_BLOCK_Y;
    if (A.b.infos[q] != 0) return;
    psd_grord_cleanup_col(psd_gbord_params(A, q), A.b.n, PSD_BLOCK_X + 1);
}
