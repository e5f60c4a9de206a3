// Eigenvectors of MANY small ComplexF64 periodic Schur decompositions of one shape (n, p): the complex column of
// psd_bevec.h, for the decompositions psd_z_pschur_batch leaves (all-true signature).  The host driver is
// psd_zbevec_host.inl.  Layout, tables (psd_bev_istride, psd_bev_ihead, psd_bev_dstride), psd_bev_args and the
// normalisation (psd_bev_norm) are those of the real path; T and Z are [gc][p][n][n] interleaved complex, column-major.
//
// A complex Schur form is triangular in every factor: every row block is one row, every selected row one solve column
// (m = 1, pair = 0, nblk = row + 1), and there is no sub-diagonal to read back.  psd_zbev_solve is the complex
// instantiation of psd_bev_solve_body: stage A deals C p dot products (not 2 C p) over the 64 lanes, each in ascending k.
// No atomics, no cross-workgroup waits; a unit's result does not depend on the units that share its wavefront.
//
// The maps stay psd_ev_map (2x2) with the second row and column zero, as in the single path's psd_ev_solve_body<true>: the
// arithmetic of a map and of a composition is shared with it.  (A scalar map type would cut the LDS traffic of the scan to
// a third: an open item, DESIGN.md.)
#pragma once
#include "psd_bevec.h"

PSD_KERNEL_B(64) psd_zbev_solve(psd_bev_args a) { psd_bev_solve_body<true>(a); }

// V_z = Z_z X_vmap(z) with complex Z for the factors z0 .. z0 + nz - 1 of every problem: grid (gc * nz, tiles of
// PSD_BEV_NT elements), one thread per output element, four FMAs per term of the triangular K range
PSD_KERNEL psd_zbev_backtransform(psd_bev_bt_args g) {
    const int n = g.n, q = PSD_BLOCK_X / g.nz, z = g.z0 + PSD_BLOCK_X % g.nz;
    const int* tab = g.itab + psd_bev_ihead(g.p) + (size_t)q * psd_bev_istride(n);
    const int ns = tab[7 * n], xl = g.itab[g.p + z];
    const size_t xs = (size_t)g.p * n * g.nsm;
    const double* Z = g.Z + ((size_t)q * g.p + z) * 2 * n * n;
    const double* Xr = g.X + (size_t)q * 2 * xs + (size_t)xl * n * g.nsm;
    const double* Xi = Xr + xs;
    psd_ev_gemm_args s;
    s.mode = 1;
    s.Cr = g.V + ((size_t)q * g.nmat + z) * 2 * n * g.maxvec;
    s.cmap = g.itab + 2 * g.p;  // (the zero of the table: Cr is the block already)
    s.cstride = 0;
    s.ldc = n;
    s.ocol = tab + 4 * n;
    s.pair = tab + 5 * n;  // (all zero: no conjugate partners)
    s.sr = g.S ? g.S + (size_t)q * 2 * n : nullptr;
    s.si = g.S ? g.S + (size_t)q * 2 * n + n : nullptr;
    PSD_PAR_FOR(t, PSD_NTHREADS) {
        const int e = PSD_BLOCK_Y * PSD_NTHREADS + t;
        if (e < ns * n) {
            const int j = e / n, i = e - j * n, ke = g.cnt[3 * ((size_t)q * n + j) + 2] ? 0 : tab[3 * n + j];
            double vr = 0.0, vi = 0.0;
            for (int k = 0; k < ke; ++k) {  // (X is zero below the column's own row: K stops there)
                const double zr = Z[2 * ((size_t)k * n + i)], zi = Z[2 * ((size_t)k * n + i) + 1];
                const double xr = Xr[(size_t)k * g.nsm + j], xi = Xi[(size_t)k * g.nsm + j];
                vr += zr * xr - zi * xi;
                vi += zr * xi + zi * xr;
            }
            psd_ev_store(s, 0, i, j, vr, vi);
        }
    }
}
