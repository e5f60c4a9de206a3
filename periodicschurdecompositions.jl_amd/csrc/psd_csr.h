// CSR operators of the periodic Krylov-Schur driver: y = A x for one sparse factor, and the structure check that runs
// before the first product of a call.  Included from psd_krylov.h and written under its rules: uniform control flow with
// PSD_PAR_FOR / PSD_SYNC (the serial host simulation runs the same text), PSD_KR_NT threads per workgroup, no
// floating-point atomics.
//
// Storage: rowptr[n + 1] int64, colind[nnz] int32, both 0-based; val[nnz] Float64, or ComplexF64 as interleaved (re, im).
// Columns of a row may come in any order and may repeat (repeats are added in storage order).
//
// Summation order, fixed by the matrix and the group width G alone: a row is owned by G consecutive lanes (G a power of
// two, 1..64, so a group never leaves its wavefront); lane g adds the entries start + g, start + g + G, ... in that
// order, then a tree over the G lanes halves the group log2 G times.  PSD_KR_NT / G rows per workgroup; a row is never
// split across groups or workgroups, so a few very long rows in a very sparse matrix are correct but run at the speed of
// one group (no second code path for them).
#pragma once

// the group width for n rows and nnz stored entries: the smallest power of two >= nnz / n, in [1, 64].  A function of the
// two counts only (never of the device), so that the bits of a product repeat across machines.
inline int psd_kr_csr_group(int n, int64_t nnz) {
    int G = 1;
    while (G < 64 && (int64_t)G * n < nnz) G *= 2;
    return G;
}

// flag words of the structure check (any non-zero value: invalid)
#define PSD_KR_CSR_BAD_ROWPTR 0
#define PSD_KR_CSR_BAD_COLIND 1
#define PSD_KR_CSR_FLAGS 2
#define PSD_KR_CSR_MAXNNZ ((int64_t)1 << 40)

// ---- structure check of one factor: rowptr[0] == 0, rowptr non-decreasing, rowptr[n] == nnz (the count the host read
// from rowptr[n] and bounded before the launch), every colind in [0, n).  Reads rowptr[0..n] and colind[0..nnz) only, and
// gathers through neither.  Each workgroup takes the tiles bx, bx + grid, ... of PSD_KR_NT indices.
PSD_KERNEL_B(PSD_KR_NT) psd_kr_csr_check(const int64_t* rowptr, const int32_t* colind, int n, int64_t nnz, int* flag) {
    const int64_t total = nnz > (int64_t)n + 1 ? nnz : (int64_t)n + 1;
    for (int64_t base = (int64_t)PSD_BLOCK_X * PSD_KR_NT; base < total; base += (int64_t)PSD_GRID_X * PSD_KR_NT) {
        PSD_PAR_FOR(t, PSD_KR_NT) {
            const int64_t i = base + t;
            if (i <= n) {
                const int64_t a = rowptr[i];
                const bool bad = (i == 0) ? (a != 0) : (i == n ? (a != nnz || a < rowptr[i - 1]) : (a < rowptr[i - 1]));
                if (bad) flag[PSD_KR_CSR_BAD_ROWPTR] = 1;
            }
            if (i < nnz) {
                const int32_t c = colind[i];
                if (c < 0 || c >= n) flag[PSD_KR_CSR_BAD_COLIND] = 1;
            }
        }
    }
}

// ---- y = A x.  grid: ceil(n / (PSD_KR_NT >> lg)) workgroups, G = 1 << lg; LDS: PSD_KR_NT elements.
template <bool Z>
PSD_KERNEL_B(PSD_KR_NT) psd_kr_csr_mv(const int64_t* rowptr, const int32_t* colind, const double* val, const double* x,
                                      double* y, int n, int lg, const int* st) {
    if (psd_kr_stopped(st)) return;
    typedef psd_kr_el<Z> K;
    typedef typename K::E E;
    PSD_LDS_DECL;
    E* s = (E*)psd_lds;
    const E* ve = (const E*)val;
    const E* xe = (const E*)x;
    E* ye = (E*)y;
    const int G = 1 << lg, rows = PSD_KR_NT >> lg;
    const int r0 = PSD_BLOCK_X * rows;
    PSD_PAR_FOR(t, PSD_KR_NT) {
        const int r = r0 + (t >> lg);
        E a = K::zero();
        if (r < n) {
            int64_t k = rowptr[r] + (t & (G - 1));
            const int64_t k1 = rowptr[r + 1];
            // four entries in flight per lane; the additions stay in storage order
            for (; k + 3 * (int64_t)G < k1; k += 4 * (int64_t)G) {
                const int32_t c0 = colind[k], c1 = colind[k + G], c2 = colind[k + 2 * (int64_t)G],
                              c3 = colind[k + 3 * (int64_t)G];
                const E v0 = ve[k], v1 = ve[k + G], v2 = ve[k + 2 * (int64_t)G], v3 = ve[k + 3 * (int64_t)G];
                const E x0 = xe[c0], x1 = xe[c1], x2 = xe[c2], x3 = xe[c3];
                a = K::add(a, K::mul(v0, x0));
                a = K::add(a, K::mul(v1, x1));
                a = K::add(a, K::mul(v2, x2));
                a = K::add(a, K::mul(v3, x3));
            }
            for (; k < k1; k += G) a = K::add(a, K::mul(ve[k], xe[colind[k]]));
        }
        s[t] = a;
    }
    PSD_SYNC();
    for (int h = G >> 1; h > 0; h >>= 1) {
        PSD_PAR_FOR(e, rows * h) {
            const int i = (e / h) * G + (e % h);
            s[i] = K::add(s[i], s[i + h]);
        }
        PSD_SYNC();
    }
    PSD_PAR_FOR(t, rows) {
        const int r = r0 + t;
        if (r < n) ye[r] = s[(size_t)t << lg];
    }
}
