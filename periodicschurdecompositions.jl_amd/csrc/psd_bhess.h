// Batched periodic Hessenberg-triangular reduction and Q formation (real): many small problems of one shape in one launch.
//
// A single small problem keeps the device launch-bound: the reduction of psd_hess.h is (n - 1) p chain links of two or
// more launches each, and a link of a 32 x 32 problem fills a handful of the 256 compute units.  Here ONE workgroup owns
// ONE problem and walks the whole chain of PSD.jl:229-247 by itself — the launches of hessenberg_dev's column() become
// loops over their block index, a workgroup barrier stands where a launch boundary stood —, so a batch of nb problems is
// one launch of nb workgroups.  The bodies are those of psd_hess.h, called in the order of the one-stream form: H and tau
// are the ones that form produces, bit for bit.
//
// The price: one problem's panel updates run on one compute unit, block after block.  Above PSD_BH_NMAX the host driver
// (psd_batch_host.inl) reduces problem by problem with the multi-workgroup forms instead.
#pragma once
#include "psd_hess.h"

// Largest order the one-workgroup-per-problem kernels take.  128 is UNMEASURED: a placeholder until the sweep of
// tools/pschur_batch_timing.py (--sweep) has run on the device (profiles/batch/README.md).
#define PSD_BH_NMAX 128

// LDS of psd_bhess: the bodies' reduction area (NT) and staged reflector (n + 8), then this kernel's reflector vector
PSD_HD size_t psd_bhess_lds_bytes(int n) { return (PSD_HESS_NT + 2 * ((size_t)n + 8)) * sizeof(double); }

// H: [nb][p][n][n] (internal factor order), overwritten LAPACK-style; tau: [nb][p][n], zeroed by the caller.
// grid = nb, PSD_HESS_NT threads, psd_bhess_lds_bytes(n)
PSD_KERNEL psd_bhess(double* H, double* tau, int n, int p) {
    PSD_LDS_DECL;
    const size_t nn = (size_t)n * n;
    double* Hq = H + (size_t)PSD_BLOCK_X * p * nn;
    double* tq = tau + (size_t)PSD_BLOCK_X * p * n;
    double* v = (double*)psd_lds + PSD_HESS_NT + n + 8;  // [0] = tau, [1..m-1] = v (the vbuf of psd_hess_refl_body)
    const int nR = (n + PSD_HESS_RS - 1) / PSD_HESS_RS;
    for (int i = 1; i <= n - 1; ++i)
        for (int j = p; j >= 1; --j) {
            const int r0 = (j == 1) ? (i + 1) : i;
            if (n - r0 + 1 < 2) continue;  // (psd_hess_refl_g / psd_hess_apply_g return: no reflector)
            const int jm1 = (j == 1) ? p : (j - 1);
            double* Aj = Hq + (size_t)(j - 1) * nn;
            double* Am = Hq + (size_t)(jm1 - 1) * nn;
            psd_hess_refl_body(Aj, n, r0, i, v, tq + (size_t)(j - 1) * n + (i - 1));
            PSD_SYNC();
            // the blocks of psd_hess_apply_g: left on A_j, then right on A_{j-1} (p == 1: the same matrix, modes 1 then 2).
            // Blocks [nL, nLmax) of that launch return at once and are not visited.
            const int lc0 = i + 1;
            const int nL = (n - lc0 + 1 + 3) / 4;
            for (int b = 0; b < nL; ++b) {
                psd_hess_apply_body(Aj, nullptr, n, r0, lc0, v, nL, b);
                PSD_SYNC();  // (the next block reuses the reduction area; p == 1: the right update reads these columns)
            }
            for (int b = 0; b < nR; ++b) {
                psd_hess_apply_body(nullptr, Am, n, r0, lc0, v, nL, nL + b);
                PSD_SYNC();
            }
        }
}

// Q_j = H_{j,1} ... H_{j,n-1} by backward accumulation from the identity (the unblocked branch of formq_dev), one workgroup
// per (problem, factor).  grid = nb * p, PSD_HESS_NT threads, PSD_HESS_NT doubles of LDS
PSD_KERNEL psd_bformq(const double* H, const double* tau, double* Q, int n, int p) {
    const size_t nn = (size_t)n * n;
    const int q = PSD_BLOCK_X / p, j = PSD_BLOCK_X % p + 1;
    const double* Hq = H + (size_t)q * p * nn;
    const double* tq = tau + (size_t)q * p * n;
    double* Qq = Q + (size_t)q * p * nn;
    double* Qj = Qq + (size_t)(j - 1) * nn;
    PSD_PAR_FOR(e, n * n) { Qj[e] = (e / n == e % n) ? 1.0 : 0.0; }
    PSD_SYNC();
    for (int i = n - 1; i >= 1; --i) {
        const int tiles = (n - i + 1 + 3) / 4;
        for (int t = 0; t < tiles; ++t) {
            psd_formq_step_body(Hq, tq, Qq, n, i, j, t);
            PSD_SYNC();
        }
    }
}

// psd_triu for a batch: zero the reflector storage below H_1's sub-diagonal / R_j's diagonal.  grid = nb * p
PSD_KERNEL psd_btriu(double* H, int n, int p) {
    const int j = PSD_BLOCK_X % p + 1;
    double* A = H + (size_t)PSD_BLOCK_X * n * n;
    const int k = (j == 1) ? 2 : 1;  // first zeroed row of column c: c + k
    PSD_PAR_FOR(e, n * n) {
        if (e % n >= e / n + k) A[e] = 0.0;
    }
}

// psd_reverse_blocks for a batch (orientation 'L'): in every problem's [p] blocks of `blk` doubles, reverse the order of
// the `cnt` blocks starting at block `first`.  grid = nb * (cnt / 2)
PSD_KERNEL psd_breverse_blocks(double* X, size_t blk, int p, int first, int cnt) {
    const int half = cnt / 2;
    const int q = PSD_BLOCK_X / half, s = PSD_BLOCK_X % half;
    double* a = X + ((size_t)q * p + first + s) * blk;
    double* b = X + ((size_t)q * p + first + cnt - 1 - s) * blk;
    PSD_PAR_FOR(e, blk) {
        const double t = a[e];
        a[e] = b[e];
        b[e] = t;
    }
}

// n == 1 (PSD.jl:333-352): the eigenvalue of problem q is the product of its p scalars.  grid = ceil(nb / 64), 64 threads
PSD_KERNEL psd_bscalar_product(const double* H, int p, int nb, double* wr, double* wi) {
    PSD_PAR_FOR(t, 64) {
        const int q = PSD_BLOCK_X * 64 + t;
        if (q < nb) {
            double l1 = H[(size_t)q * p];
            for (int j = 1; j < p; ++j) l1 *= H[(size_t)q * p + j];
            wr[q] = l1;
            wi[q] = 0.0;
        }
    }
}
