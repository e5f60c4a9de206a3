// Batched periodic Hessenberg-triangular reduction and Q formation, ComplexF64: many small problems of one shape in one
// launch — the complex counterpart of psd_bhess.h, for the reasons given there.
//
// ONE workgroup owns ONE problem and walks the whole chain of the one-stream form of zhessenberg_dev
// (PeriodicSchurDecompositions.jl:229-247 with the complex reflector of householder.jl:110-156): psd_zhess_refl_body,
// then the blocks of psd_zhess_apply_body — left on A_j, right on A_{j-1} —, a workgroup barrier where a launch
// boundary stood.  The reflector that the single call hands from launch to launch through device memory lives in LDS
// here.  H and tau are the ones the one-launch-per-link form produces, bit for bit.  Unlike the real chain a link of one
// row is not skipped: the complex reflector of a single entry rotates it onto the real axis (tau != 0).
//
// The price is that of psd_bhess.h: one problem's panel updates run on one compute unit, block after block.  Above
// PSD_ZB_NMAX the host driver (psd_zbatch_host.inl) runs the single-problem forms instead, problem by problem.
#pragma once
#include "psd_zhess.h"

// Largest order the one-workgroup-per-problem kernels (and the one-wavefront-per-problem iteration, psd_zbqz.h) take.
// Measured: the largest order of the sweep of tools/pschur_batch_timing.py --complex (nb = 256, p = 8, n = 8 ... 128) at
// which the batched call still beats the loop of single calls — it does at every swept order, 25 x in wall time at
// n = 128 (profiles/batch/README.md).  Orders above 128 have not been swept.
#define PSD_ZB_NMAX 128

// LDS of psd_zbhess: the bodies' reduction area (NT) and staged reflector (n + 8), then this kernel's reflector vector
PSD_HD size_t psd_zbhess_lds_bytes(int n) { return (PSD_HESS_NT + 2 * ((size_t)n + 8)) * sizeof(psd_z); }

// H: [nb][p][n][n] (internal factor order), overwritten LAPACK-style; tau: [nb][p][n], zeroed by the caller.
// grid = nb, PSD_HESS_NT threads, psd_zbhess_lds_bytes(n)
PSD_KERNEL psd_zbhess(psd_z* H, psd_z* tau, int n, int p) {
    PSD_LDS_DECL;
    const size_t nn = (size_t)n * n;
    psd_z* Hq = H + (size_t)PSD_BLOCK_X * p * nn;
    psd_z* tq = tau + (size_t)PSD_BLOCK_X * p * n;
    psd_z* v = (psd_z*)psd_lds + PSD_HESS_NT + n + 8;  // [0] = tau, [1..m-1] = v (the vbuf of psd_zhess_refl_body)
    const int nR = (n + PSD_HESS_RS - 1) / PSD_HESS_RS;
    for (int i = 1; i <= n - 1; ++i)
        for (int j = p; j >= 1; --j) {
            const int r0 = (j == 1) ? (i + 1) : i;
            const int jm1 = (j == 1) ? p : (j - 1);
            psd_z* Aj = Hq + (size_t)(j - 1) * nn;
            psd_z* Am = Hq + (size_t)(jm1 - 1) * nn;
            psd_zhess_refl_body(Aj, n, r0, i, v, tq + (size_t)(j - 1) * n + (i - 1));
            PSD_SYNC();
            // the blocks of psd_zhess_apply: left on A_j, then right on A_{j-1} (p == 1: the same matrix, two launches)
            const int lc0 = i + 1;
            const int nL = (n - lc0 + 1 + 3) / 4;
            for (int b = 0; b < nL; ++b) {
                psd_zhess_apply_body(Aj, nullptr, n, r0, lc0, v, nL, b);
                PSD_SYNC();  // (the next block reuses the reduction area; p == 1: the right update reads these columns)
            }
            for (int b = 0; b < nR; ++b) {
                psd_zhess_apply_body(nullptr, Am, n, r0, lc0, v, nL, nL + b);
                PSD_SYNC();
            }
        }
}

// Q_j = H_{j,1} ... H_{j,n-1} by backward accumulation from the identity (the unblocked branch of zformq_dev), one
// workgroup per (problem, factor).  grid = nb * p, PSD_HESS_NT threads, PSD_HESS_NT complex elements of LDS
PSD_KERNEL psd_zbformq(const psd_z* H, const psd_z* tau, psd_z* Q, int n, int p) {
    const size_t nn = (size_t)n * n;
    const int q = PSD_BLOCK_X / p, j = PSD_BLOCK_X % p + 1;
    const psd_z* Hq = H + (size_t)q * p * nn;
    const psd_z* tq = tau + (size_t)q * p * n;
    psd_z* Qq = Q + (size_t)q * p * nn;
    psd_z* Qj = Qq + (size_t)(j - 1) * nn;
    PSD_PAR_FOR(e, n * n) { Qj[e] = zmk((e / n == e % n) ? 1.0 : 0.0, 0.0); }
    PSD_SYNC();
    for (int i = n - 1; i >= 1; --i) {
        const int tiles = (n - i + 1 + 3) / 4;
        for (int t = 0; t < tiles; ++t) {
            psd_zformq_step_body(Hq, tq, Qq, n, i, j, t);
            PSD_SYNC();
        }
    }
}

// psd_ztriu for a batch: zero the reflector storage below H_1's sub-diagonal / R_j's diagonal.  grid = nb * p
PSD_KERNEL psd_zbtriu(psd_z* H, int n, int p) {
    const int j = PSD_BLOCK_X % p + 1;
    psd_z* A = H + (size_t)PSD_BLOCK_X * n * n;
    const int k = (j == 1) ? 2 : 1;  // first zeroed row of column c: c + k
    PSD_PAR_FOR(e, n * n) {
        if (e % n >= e / n + k) A[e] = zmk(0.0, 0.0);
    }
}
