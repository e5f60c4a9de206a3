// Device kernels of the periodic Krylov-Schur driver (partial_pschur, src/krylov.jl:446-798 of the reference).
//
// One Krylov step extends the basis of every factor by one column: for l = 1..p, v = A_l u_{l,j} (the hot path: p dense
// matrix-vector products, p n^2 elements of HBM traffic per step), then v is orthogonalised against the next factor's
// basis (classical Gram-Schmidt with one conditional re-orthogonalisation, krylov.jl:270-293 / :335-357), normalised and
// stored, and its coefficients go into the device copy of the projected factors.  Every decision of that sequence is
// taken on the device: each kernel re-derives it from the same partial sums in the same order (so every workgroup agrees,
// bit for bit), the re-orthogonalisation launches return at once when the first pass was good enough, and a vector that
// stays in the span of the basis stops the rest of the step through a flag in device memory.  The host reads that flag
// once per step.
//
// No floating-point atomics anywhere: every reduction is a fixed tree inside a workgroup followed by an in-order sum over
// the workgroups, so the same inputs give the same bits on every run.
//
// All kernels are written in the uniform-control + PSD_PAR_FOR style of psd_platform.h (the serial host simulation runs
// them unchanged).  Elements: Float64, or ComplexF64 as interleaved (re, im) pairs.
#pragma once
#include "psd_complex.h"

#define PSD_KR_NT 256        // threads per workgroup of every Krylov kernel (one row per thread, two in the real matvec)
#define PSD_KR_BASIS_LDS 65536  // LDS budget of the basis-update row tile

template <bool Z>
struct psd_kr_el;
template <>
struct psd_kr_el<false> {
    typedef double E;
    static PSD_HD E zero() { return 0.0; }
    static PSD_HD E add(E a, E b) { return a + b; }
    static PSD_HD E sub(E a, E b) { return a - b; }
    static PSD_HD E mul(E a, E b) { return a * b; }
    static PSD_HD E cmul(E a, E b) { return a * b; }  // conj(a) * b
    static PSD_HD E scal(double s, E a) { return s * a; }
    static PSD_HD double abs2(E a) { return a * a; }
    static PSD_HD double re(E a) { return a; }
};
template <>
struct psd_kr_el<true> {
    typedef psd_z E;
    static PSD_HD E zero() { return zmk(0.0, 0.0); }
    static PSD_HD E add(E a, E b) { return zadd(a, b); }
    static PSD_HD E sub(E a, E b) { return zsub(a, b); }
    static PSD_HD E mul(E a, E b) { return zmul(a, b); }
    static PSD_HD E cmul(E a, E b) { return zmul(zconj(a), b); }
    static PSD_HD E scal(double s, E a) { return zscal(s, a); }
    static PSD_HD double abs2(E a) { return zabs2(a); }
    static PSD_HD double re(E a) { return a.re; }
};

// a real number as an element
template <bool Z>
PSD_HD typename psd_kr_el<Z>::E psd_kr_real(double x) {
    if constexpr (Z) return zmk(x, 0.0);
    else return x;
}

struct alignas(16) psd_kr_d2 {
    double x, y;
};

// Step state in device memory (int words).  ST_STOP: the step stopped at factor ST_LFAC (0-based) because its vector
// was in the span of the basis (ST_KIND 1) or the start vector was mapped to ~0 (ST_KIND 2, krylov.jl:298-304); every
// later launch of the step returns at once.  ST_NREORTH counts second Gram-Schmidt passes over the whole call.
#define PSD_KR_ST_STOP 0
#define PSD_KR_ST_LFAC 1
#define PSD_KR_ST_KIND 2
#define PSD_KR_ST_NREORTH 3
#define PSD_KR_ST_WORDS 8

// One orthogonalise-normalise-store stage: v against the first `ncols` columns of U, result into column `ncols` of U.
struct psd_kr_args {
    int n, ncols;   // rows; basis columns to orthogonalise against
    int nblk, ldp;  // workgroups of the row kernels; pitch (elements) of the per-workgroup partials
    int lfac;       // factor index recorded in the state when the stage stops the step
    double eta;     // re-orthogonalisation threshold (1/sqrt(2), krylov.jl:148)
    double tol1;    // null-vector threshold of the first column (krylov.jl:298)
    double* U;      // basis, ld n, at least ncols + 1 columns
    double* v;      // work vector [n]
    double* pA;     // [nblk][ldp] partial U^H v of pass 1; slot ldp-1 = partial ||v||^2 before orthogonalisation
    double* pB;     // [nblk][ldp] partial U^H v of pass 2
    double* w1;     // [nblk] partial ||v||^2 after pass 1
    double* w2;     // [nblk] partial ||v||^2 after pass 2
    double* h;      // [ldp] coefficients of this stage
    double* Hcol;   // column of the projected factor (rows 0..ncols) or nullptr
    int* st;        // step state
};

PSD_HD bool psd_kr_stopped(const int* st) { return st && ((volatile const int*)st)[PSD_KR_ST_STOP] != 0; }

// in-order sum of `count` doubles `stride` apart (every lane, uniform)
PSD_HD double psd_kr_sum(const double* x, int count, int stride) {
    double s = 0.0;
    for (int b = 0; b < count; ++b) s += x[(size_t)b * stride];
    return s;
}

struct psd_kr_dec {
    bool reorth, stop;
    int kind;
    double hjj;
};
// The decisions of krylov.jl:277-299 / :340-357 from the partial sums (`final` = false: only whether pass 2 runs).
template <bool Z>
PSD_HD psd_kr_dec psd_kr_decide(const psd_kr_args& a, bool final) {
    constexpr int ES = Z ? 2 : 1;
    psd_kr_dec d;
    d.reorth = d.stop = false;
    d.kind = 0;
    double rn = sqrt(psd_kr_sum(a.pA + (size_t)(a.ldp - 1) * ES, a.nblk, a.ldp * ES));
    if (a.ncols == 0) {  // first column of a step: nothing to orthogonalise against, only the null test
        d.hjj = rn;
        d.stop = rn < a.tol1 || !(rn > 0.0);
        d.kind = d.stop ? 2 : 0;
        return d;
    }
    const double wn1 = sqrt(psd_kr_sum(a.w1, a.nblk, 1));
    d.reorth = wn1 < a.eta * rn;
    if (!final) {
        d.hjj = 0.0;
        return d;
    }
    double wn = wn1;
    if (d.reorth) {
        rn = wn1;
        wn = sqrt(psd_kr_sum(a.w2, a.nblk, 1));
    }
    d.stop = wn <= a.eta * rn;
    d.kind = d.stop ? 1 : 0;
    d.hjj = wn;
    return d;
}

// block tree sum of s[0..PSD_KR_NT) into s[0] (s in LDS; every lane wrote its slot before the call)
template <class E, class K>
PSD_D void psd_kr_tree(E* s) {
    PSD_SYNC();
    for (int h = PSD_KR_NT / 2; h > 0; h >>= 1) {
        PSD_PAR_FOR(t, h) s[t] = K::add(s[t], s[t + h]);
        PSD_SYNC();
    }
}

// ---- periodic matvec, stage 1: part[cy][r] = sum over the columns c of chunk cy of A[r, c] u[c] -----------------------
// grid (row tiles of PSD_KR_NT * RP rows, column chunks of ccols).  RP = 2 (Float64, n even): two rows per lane through
// one 16-byte load, so one wavefront reads 1 KiB of a column per instruction.  Straight to VGPRs, no LDS: the matrix is
// read exactly once.
template <bool Z, int RP>
PSD_KERNEL_B(PSD_KR_NT) psd_kr_mv(const double* A, const double* u, double* part, int n, int ccols, const int* st) {
    if (psd_kr_stopped(st)) return;
    typedef psd_kr_el<Z> K;
    typedef typename K::E E;
    const E* Ae = (const E*)A;
    const E* ue = (const E*)u;
    E* pe = (E*)part;
    const int c0 = PSD_BLOCK_Y * ccols;
    const int c1 = (c0 + ccols < n) ? c0 + ccols : n;
    PSD_PAR_FOR(t, PSD_KR_NT) {
        const int r = (PSD_BLOCK_X * PSD_KR_NT + t) * RP;
        if (r < n) {
            if constexpr (RP == 2 && !Z) {
                // (r even, n even: the pair never straddles a column and the address is 16-byte aligned)
                double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
                const double* col = A + (size_t)c0 * n + r;
                int c = c0;
#pragma unroll 8
                for (; c + 1 < c1; c += 2) {
                    const psd_kr_d2 x = *(const psd_kr_d2*)col;
                    const psd_kr_d2 y = *(const psd_kr_d2*)(col + n);
                    col += 2 * (size_t)n;
                    const double u0 = u[c], u1 = u[c + 1];
                    a0 += x.x * u0;
                    a1 += x.y * u0;
                    b0 += y.x * u1;
                    b1 += y.y * u1;
                }
                if (c < c1) {
                    const psd_kr_d2 x = *(const psd_kr_d2*)col;
                    a0 += x.x * u[c];
                    a1 += x.y * u[c];
                }
                part[(size_t)PSD_BLOCK_Y * n + r] = a0 + b0;
                part[(size_t)PSD_BLOCK_Y * n + r + 1] = a1 + b1;
            } else {
                E a0 = K::zero(), b0 = K::zero();
                int c = c0;
#pragma unroll 8
                for (; c + 1 < c1; c += 2) {
                    a0 = K::add(a0, K::mul(Ae[(size_t)c * n + r], ue[c]));
                    b0 = K::add(b0, K::mul(Ae[(size_t)(c + 1) * n + r], ue[c + 1]));
                }
                if (c < c1) a0 = K::add(a0, K::mul(Ae[(size_t)c * n + r], ue[c]));
                pe[(size_t)PSD_BLOCK_Y * n + r] = K::add(a0, b0);
            }
        }
    }
}

// ---- stage 2 (and pass 2): v = sum of the nchunk partials in chunk order (nchunk = 0: v as it stands), then the
// per-workgroup partials of U^H v (first ncols slots) and of ||v||^2 (slot ldp-1) into dp.  gate: pass 2, runs only when
// the first pass left less than eta of the norm.  grid: nblk workgroups of PSD_KR_NT rows.
template <bool Z>
PSD_KERNEL_B(PSD_KR_NT) psd_kr_dots(psd_kr_args a, const double* part, int nchunk, int gate) {
    if (psd_kr_stopped(a.st)) return;
    if (gate && !psd_kr_decide<Z>(a, false).reorth) return;
    typedef psd_kr_el<Z> K;
    typedef typename K::E E;
    PSD_LDS_DECL;
    E* s = (E*)psd_lds;
    E* vv = s + PSD_KR_NT;
    E* ve = (E*)a.v;
    const E* Ue = (const E*)a.U;
    const E* pe = (const E*)part;
    E* dp = (E*)(gate ? a.pB : a.pA);
    const int n = a.n, bx = PSD_BLOCK_X;
    PSD_PAR_FOR(t, PSD_KR_NT) {
        const int r = bx * PSD_KR_NT + t;
        E y = K::zero();
        if (r < n) {
            if (nchunk > 0) {
                for (int q = 0; q < nchunk; ++q) y = K::add(y, pe[(size_t)q * n + r]);
                ve[r] = y;
            } else {
                y = ve[r];
            }
        }
        vv[t] = y;
    }
    PSD_SYNC();
    const int nslot = gate ? a.ncols : a.ncols + 1;  // (pass 2 needs no norm before it)
    for (int i = 0; i < nslot; ++i) {
        PSD_PAR_FOR(t, PSD_KR_NT) {
            const int r = bx * PSD_KR_NT + t;
            E x = K::zero();
            if (r < n) {
                if (i < a.ncols) x = K::cmul(Ue[(size_t)i * n + r], vv[t]);
                else x = psd_kr_real<Z>(K::abs2(vv[t]));
            }
            s[t] = x;
        }
        psd_kr_tree<E, K>(s);
        PSD_ONE dp[(size_t)bx * a.ldp + (i < a.ncols ? i : a.ldp - 1)] = s[0];
        PSD_SYNC();
    }
}

// ---- v -= U c with c = the in-order sum of the dot partials (pass 1: pA, sets h; pass 2: pB, adds to h), then the
// per-workgroup partial of ||v||^2 into w1 / w2.  Every workgroup sums the partials itself; workgroup 0 writes h.
template <bool Z>
PSD_KERNEL_B(PSD_KR_NT) psd_kr_axpy(psd_kr_args a, int pass) {
    if (psd_kr_stopped(a.st)) return;
    if (pass == 2 && !psd_kr_decide<Z>(a, false).reorth) return;
    typedef psd_kr_el<Z> K;
    typedef typename K::E E;
    PSD_LDS_DECL;
    E* s = (E*)psd_lds;
    E* cc = s + PSD_KR_NT;  // [ncols]
    E* ve = (E*)a.v;
    E* he = (E*)a.h;
    const E* Ue = (const E*)a.U;
    const E* dp = (const E*)(pass == 2 ? a.pB : a.pA);
    const int n = a.n, bx = PSD_BLOCK_X;
    PSD_PAR_FOR(i, a.ncols) {
        E c = K::zero();
        for (int b = 0; b < a.nblk; ++b) c = K::add(c, dp[(size_t)b * a.ldp + i]);
        cc[i] = c;
        if (bx == 0) he[i] = (pass == 2) ? K::add(he[i], c) : c;
    }
    PSD_SYNC();
    PSD_PAR_FOR(t, PSD_KR_NT) {
        const int r = bx * PSD_KR_NT + t;
        E x = K::zero();
        if (r < n) {
            E y = ve[r];
            for (int i = 0; i < a.ncols; ++i) y = K::sub(y, K::mul(Ue[(size_t)i * n + r], cc[i]));
            ve[r] = y;
            x = psd_kr_real<Z>(K::abs2(y));
        }
        s[t] = x;
    }
    psd_kr_tree<E, K>(s);
    double* w = pass == 2 ? a.w2 : a.w1;
    PSD_ONE w[bx] = K::re(s[0]);
}

// ---- the final decision: workgroup 0 records it (projected-factor column, state); every workgroup writes its rows of
// the new basis column v / h_jj unless the step stopped.
template <bool Z>
PSD_KERNEL_B(PSD_KR_NT) psd_kr_store(psd_kr_args a) {
    if (psd_kr_stopped(a.st)) return;
    typedef psd_kr_el<Z> K;
    typedef typename K::E E;
    const psd_kr_dec d = psd_kr_decide<Z>(a, true);
    const int n = a.n, bx = PSD_BLOCK_X;
    if (bx == 0) {
        E* He = (E*)a.Hcol;
        const E* he = (const E*)a.h;
        if (He) {
            PSD_PAR_FOR(i, a.ncols) He[i] = he[i];
            PSD_ONE He[a.ncols] = d.stop ? K::zero() : psd_kr_real<Z>(d.hjj);
        }
        PSD_ONE {
            if (d.reorth) a.st[PSD_KR_ST_NREORTH] += 1;
            if (d.stop) {
                a.st[PSD_KR_ST_LFAC] = a.lfac;
                a.st[PSD_KR_ST_KIND] = d.kind;
                a.st[PSD_KR_ST_STOP] = 1;
            }
        }
    }
    if (d.stop) return;
    const double rh = 1.0 / d.hjj;
    E* out = (E*)a.U + (size_t)a.ncols * n;
    const E* ve = (const E*)a.v;
    PSD_PAR_FOR(t, PSD_KR_NT) {
        const int r = bx * PSD_KR_NT + t;
        if (r < n) out[r] = K::scal(rh, ve[r]);
    }
}

// ---- start vectors: counter-based uniform [0, 1) numbers (splitmix64 of seed and draw index), one draw per call of the
// driver's generator, element i from counter i (re / im from 2i / 2i + 1)
PSD_HD uint64_t psd_kr_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
PSD_KERNEL_B(PSD_KR_NT) psd_kr_rand(double* v, int count, uint64_t seed, uint64_t draw) {
    const uint64_t key = psd_kr_mix(seed ^ psd_kr_mix(draw + 0x632BE59BD9B4E019ull));
    PSD_PAR_FOR(t, PSD_KR_NT) {
        const int i = PSD_BLOCK_X * PSD_KR_NT + t;
        if (i < count) v[i] = (double)(psd_kr_mix(key + (uint64_t)i) >> 11) * (1.0 / 9007199254740992.0);
    }
}

// ---- basis update V_l[:, a:a+m) <- V_l[:, a:a+m) Q_l for every factor l in one launch (grid: row tiles x p).  The
// workgroup stages its R x m tile in LDS first, so the product is written in place.  Q: [p][m][m], column-major.
template <bool Z>
PSD_KERNEL_B(PSD_KR_NT) psd_kr_basis(double* V, size_t vstride, const double* Q, int n, int a0, int m, int R) {
    typedef psd_kr_el<Z> K;
    typedef typename K::E E;
    PSD_LDS_DECL;
    E* tile = (E*)psd_lds;  // [m][R]
    const int l = PSD_BLOCK_Y;
    E* Ve = (E*)V + (size_t)l * vstride + (size_t)a0 * n;
    const E* Qe = (const E*)Q + (size_t)l * m * m;
    const int r0 = PSD_BLOCK_X * R;
    const int rows = (r0 + R <= n) ? R : n - r0;
    PSD_PAR_FOR(e, rows * m) {
        const int i = e / rows, r = e - i * rows;
        tile[(size_t)i * R + r] = Ve[(size_t)i * n + r0 + r];
    }
    PSD_SYNC();
    PSD_PAR_FOR(e, rows * m) {
        const int j = e / rows, r = e - j * rows;
        E y = K::zero();
        for (int i = 0; i < m; ++i) y = K::add(y, K::mul(tile[(size_t)i * R + r], Qe[(size_t)j * m + i]));
        Ve[(size_t)j * n + r0 + r] = y;
    }
}

// reset of the step flags (the re-orthogonalisation counter stays)
PSD_KERNEL_B(64) psd_kr_reset(int* st) {
    PSD_ONE {
        st[PSD_KR_ST_STOP] = 0;
        st[PSD_KR_ST_LFAC] = 0;
        st[PSD_KR_ST_KIND] = 0;
    }
}

// CSR operators (sparse factors): the matvec that writes v directly, and the structure check
#include "psd_csr.h"
