// Periodic Sylvester solves for many small periodic Schur forms, and what xTRSEN builds on them (the S and the SEP of an
// invariant periodic subspace), for the batches of psd_bord.h / psd_zbord.h.  The host driver is psd_bsylv_host.inl.
// The bodies of the solve take a row range of T11 and a column range of T22: the whole of X here, a tile of it in the
// single-problem walk of psd_sylv.h.
//
// A periodic Schur form of order n and period p in USER order, split at m (k = n - m): T_l = [T11_l T12_l; 0 T22_l].  With
// (a(l), b(l)) = (l + 1, l) for orientation 'L' and (l, l + 1) for 'R' (the factors of the residual Z_a T_l Z_b' - A_l), the
// periodic Sylvester operator on p stacked m x k blocks is
//     S(X)_l = T11_l X_b(l) - X_a(l) T22_l ,                    l = 1..p ,
// and its adjoint under the Frobenius inner product over the stacked blocks
//     S^H(Y)_j = T11_l^H Y_l - Y_l' T22_l'^H ,   b(l) = j, a(l') = j   ('L': l = j, l' = j - 1;  'R': l = j - 1, l' = j).
//
// psd_bsyl_solve<CPLX>: S(X) = C or S^H(X) = C for a group of problems, one wavefront per problem, C overwritten by X in
// global memory; T is only read.  Bartels-Stewart over the common block partition of the factors: block rows of T11
// bottom-up and block columns of T22 left to right (S^H: top-down, right to left).  Block (i, j) is the cyclic system
//     A_ii,l X_ij,b - X_ij,a B_jj,l = C_ij,l - sum_{r > i} A_ir,l X_rj,b + sum_{r < j} X_ir,a B_rj,l      over all l,
// a chain of p small Sylvester equations that the solvers of the reordering kernels take: psd_rord_psylsolve (Float64,
// blocks 1 or 2 wide, the partition read from the sub-diagonal of the quasi-triangular factor) and psd_ord_cycsolve
// (ComplexF64, scalars).  For S^H the chain runs over the equations in reverse order, which brings it to the same form.
//   Float64     the wavefront walks the blocks one after the other; the right-hand sides of a block are dealt to the lanes
//               (an entry of an equation per group of lanes, a slice of its sum per lane, added in lane order).
//   ComplexF64  the entries of an anti-diagonal of X are independent: one entry per lane, each lane with its own sums and
//               its own cyclic solve.
// LDS holds the small-block scratch alone (it grows with p, not with n).  Every sum has a fixed order and nothing is shared
// between workgroups: a problem's bits do not depend on the batch, on its place in it or on the grouping.
// A problem whose small solve is rejected (T11 and T22 share an eigenvalue of the product) or whose solution is not
// finite gets PSD_INFO_SINGULAR in info[q] and NaNs in X; the others complete.  There is no scale factor (xTRSYL's).
//
// psd_bsyl_norms: s[q][l] = 1 / sqrt(1 + ||X_l||_F^2), one wavefront per (problem, factor).
// psd_bsyl_est_step: the vector work of LAPACK's reverse-communication 1-norm estimator (xLACN2, real and complex variant)
// for || S^-1 ||_1 on the p m k stacked unknowns, per problem, between two solves; the vectors stay on the device.
#pragma once
#include "psd_rord.h"
#include "psd_zord.h"

#define PSD_BSYL_NMAX 128  // largest order of the batch entries (above it: the tiled single-problem walk of psd_sylv.h)
#define PSD_BSYL_ITMAX 5   // xLACN2's iteration limit

struct psd_bsyl_args {
    const double* T;   // [gc][p][n][n] column-major blocks, user order (CPLX: interleaved)
    double* X;         // [gc][p][xb] elements: block l of problem q is m[q] x (n - m[q]) column-major, ld m[q]
    const int* m;      // [gc]
    const int* act;    // [gc]: a problem with act[q] == 0 takes no part
    const int* ptrans; // [gc] per-problem form (1: S, 2: S^H, the estimator's kase), or null: `trans` for all
    int* info;         // [gc]: PSD_INFO_SINGULAR is left here; never cleared
    size_t xb;
    int n, p, qsub, left, trans, fromT;  // qsub: 0-based factor with the 2x2 blocks; fromT: C = -T12 is loaded first
};

// scratch of the Float64 path in doubles: per factor PSD_RORD_SCR + 52 (psd_rord_psylsolve), its 192, the partial sums
// (max(64, 4 p)), a flag word and the signature bytes
PSD_HD size_t psd_bsyl_lds_bytes(int p, bool cplx) {
    if (cplx) return sizeof(double) * 2 * 64 * (8 * (size_t)p + 1) + 16;
    const size_t red = 4 * (size_t)p > 64 ? 4 * (size_t)p : 64;
    return sizeof(double) * ((size_t)p * (PSD_RORD_SCR + 52) + 192 + red + 2) + (((size_t)p + 15) & ~(size_t)15);
}

// the factors and the unknowns of equation e (0-based), and the place of the equation in the solvers' chain
struct psd_bsyl_eq {
    int fa, fb, ua, ub;
};
PSD_D psd_bsyl_eq psd_bsyl_equation(int e, int p, bool left, bool trans) {
    const int nx = e + 1 < p ? e + 1 : 0, pv = e > 0 ? e - 1 : p - 1;
    psd_bsyl_eq q;
    if (!trans) {
        q.fa = q.fb = e;
        q.ua = left ? e : nx;
        q.ub = left ? nx : e;
    } else if (left) {
        q.fa = q.ua = e;
        q.fb = q.ub = pv;
    } else {
        q.fa = q.ua = pv;
        q.fb = q.ub = e;
    }
    return q;
}

// X_q = NaN (a problem that ended with PSD_INFO_SINGULAR)
template <bool CPLX>
PSD_D void psd_bsyl_poison(double* X, size_t xb, int p, int mk) {
    constexpr int E = CPLX ? 2 : 1;
    const double nan = NAN;
    for (int l = 0; l < p; ++l) {
        PSD_PAR_FOR(t, mk * E) { X[(size_t)l * xb * E + t] = nan; }
    }
}

// the product of the scalars a_l and of the scalars b_l are the same number: the cyclic scalar system is singular.  (Equal
// diagonals give equal bits.  A product that left the range says nothing.)
PSD_D bool psd_bsyl_finite(double v) { return v - v == 0.0; }
PSD_D bool psd_bsyl_same_product(double pa, double pb) { return pa == pb && psd_bsyl_finite(pa) && pa != 0.0; }

// The rows [r.i0, r.i1) of T11 and the columns [r.j0, r.j1) of T22 (local: column j of T22 is column m + j of T) of one
// problem: the whole of X for the batch kernel, a tile of it for the tiled walk of psd_sylv.h, whose update kernel has
// taken the sums over the tiles solved before into the right-hand side.  X has leading dimension m.
struct psd_bsyl_range {
    int i0, i1, j0, j1;
};

// false: the problem is singular (the caller leaves the code and the NaNs)
PSD_D bool psd_bsyl_real_range(const double* T, double* X, size_t xb, int n, int p, int m, int qsub, bool left, bool trans,
                               int fromT, const psd_bsyl_range rg) {
    PSD_LDS_DECL;
    const size_t nn = (size_t)n * n;
    const int mt = rg.i1 - rg.i0, kt = rg.j1 - rg.j0;
    double* scr = (double*)psd_lds;
    double* wk = scr + (size_t)p * PSD_RORD_SCR;
    double* ws = wk + (size_t)p * 52;
    double* red = ws + 192;
    const int nred = 4 * p > 64 ? 4 * p : 64;
    double* flag = red + nred;  // the block's verdict (and a word of padding)
    unsigned char* SL = (unsigned char*)(flag + 2);
    const double* Tq = T + (size_t)qsub * nn;
    if (fromT) {
        for (int l = 0; l < p; ++l) {
            PSD_PAR_FOR(t, mt * kt) {
                const int i = rg.i0 + t % mt, j = rg.j0 + t / mt;
                X[(size_t)l * xb + (size_t)j * m + i] = -T[(size_t)l * nn + (size_t)(m + j) * n + i];
            }
        }
    }
    PSD_PAR_FOR(l, p) { SL[l] = left ? 1 : 0; }
    PSD_SYNC();
    // block rows of T11: bottom-up (S^H: top-down); i0 is the first row of the block, p1 its width
    int inext = trans ? rg.i0 : rg.i1 - 1;
    while (trans ? inext < rg.i1 : inext >= rg.i0) {
        int i0, p1;
        if (trans) {
            i0 = inext;
            p1 = (i0 + 1 < rg.i1 && Tq[(size_t)i0 * n + i0 + 1] != 0.0) ? 2 : 1;
            inext = i0 + p1;
        } else {
            p1 = (inext > rg.i0 && Tq[(size_t)(inext - 1) * n + inext] != 0.0) ? 2 : 1;
            i0 = inext - p1 + 1;
            inext = i0 - 1;
        }
        // block columns of T22: left to right (S^H: right to left)
        int jnext = trans ? rg.j1 - 1 : rg.j0;
        while (trans ? jnext >= rg.j0 : jnext < rg.j1) {
            int j0, p2;
            if (trans) {
                p2 = (jnext > rg.j0 && Tq[(size_t)(m + jnext - 1) * n + m + jnext] != 0.0) ? 2 : 1;
                j0 = jnext - p2 + 1;
                jnext = j0 - 1;
            } else {
                j0 = jnext;
                p2 = (j0 + 1 < rg.j1 && Tq[(size_t)(m + j0) * n + m + j0 + 1] != 0.0) ? 2 : 1;
                jnext = j0 + p2;
            }
            const int pp = p1 * p2, items = p * pp;
            const int nparts = items >= 64 ? 1 : 64 / items;
            // the sums of the right-hand sides: over the solved rows below (above) in column j, then over the solved
            // columns to the left (right) in row i; a lane takes every nparts-th term, ascending
            const int la = trans ? i0 - rg.i0 : rg.i1 - (i0 + p1), lb = trans ? rg.j1 - (j0 + p2) : j0 - rg.j0;
            PSD_PAR_FOR(t, items * nparts) {
                const int it = t / nparts, part = t - it * nparts, e = it / pp, ent = it - e * pp;
                const int i = i0 + ent % p1, j = j0 + ent / p1;
                const psd_bsyl_eq eq = psd_bsyl_equation(e, p, left, trans);
                const double* A = T + (size_t)eq.fa * nn;
                const double* B = T + (size_t)eq.fb * nn;
                const double* Xa = X + (size_t)eq.ua * xb;
                const double* Xb = X + (size_t)eq.ub * xb;
                double s = 0.0;
                for (int u = part; u < la + lb; u += nparts) {
                    if (u < la) {
                        const int r = trans ? rg.i0 + u : i0 + p1 + u;
                        const double a = trans ? A[(size_t)i * n + r] : A[(size_t)r * n + i];
                        s -= a * Xa[(size_t)j * m + r];
                    } else {
                        const int r = trans ? j0 + p2 + (u - la) : rg.j0 + (u - la);
                        const double b = trans ? B[(size_t)(m + r) * n + m + j] : B[(size_t)(m + j) * n + m + r];
                        s += Xb[(size_t)r * m + i] * b;
                    }
                }
                red[t] = s;
            }
            PSD_SYNC();
            // the chain of the block: equation e at place kp, the diagonal blocks (S^H: transposed), minus the right side
            PSD_PAR_FOR(it, items) {
                const int e = it / pp, ent = it - e * pp, ii = ent % p1, jj = ent / p1;
                const int kp = trans ? p - 1 - e : e;
                double s = X[(size_t)e * xb + (size_t)(j0 + jj) * m + i0 + ii];
                for (int part = 0; part < nparts; ++part) s += red[it * nparts + part];
                double* sc = scr + (size_t)kp * PSD_RORD_SCR;
                sc[4 + jj * 2 + ii] = -s;
                if (ent == 0) {
                    const psd_bsyl_eq eq = psd_bsyl_equation(e, p, left, trans);
                    const double* A = T + (size_t)eq.fa * nn;
                    const double* B = T + (size_t)eq.fb * nn;
                    for (int c = 0; c < 2; ++c)
                        for (int r = 0; r < 2; ++r) {
                            const int ar = trans ? c : r, ac = trans ? r : c;
                            sc[c * 2 + r] = (r < p1 && c < p1) ? A[(size_t)(i0 + ac) * n + i0 + ar] : 0.0;
                            sc[8 + c * 2 + r] = (r < p2 && c < p2) ? B[(size_t)(m + j0 + ac) * n + m + j0 + ar] : 0.0;
                        }
                }
            }
            PSD_SYNC();
            bool ok = true;
            if (pp == 1) {
                double pa = 1.0, pb = 1.0;  // (in the order of the factors, whatever the chain's is)
                for (int l = 0; l < p; ++l) {
                    pa *= T[(size_t)l * nn + (size_t)i0 * n + i0];
                    pb *= T[(size_t)l * nn + (size_t)(m + j0) * n + m + j0];
                }
                ok = !psd_bsyl_same_product(pa, pb);
            }
            if (ok) ok = psd_rord_psylsolve(p, p1, p2, scr, wk, ws, SL);
            PSD_SYNC();
            PSD_ONE { flag[0] = ok ? 0.0 : 1.0; }
            PSD_SYNC();
            // x of place kp is the unknown next to A for 'L', next to B for 'R'
            PSD_PAR_FOR(it, items) {
                const int kp = it / pp, ent = it - kp * pp, ii = ent % p1, jj = ent / p1;
                const psd_bsyl_eq eq = psd_bsyl_equation(trans ? p - 1 - kp : kp, p, left, trans);
                const double v = scr[(size_t)kp * PSD_RORD_SCR + 12 + jj * 2 + ii];
                if (!psd_bsyl_finite(v)) flag[0] = 1.0;
                X[(size_t)(left ? eq.ua : eq.ub) * xb + (size_t)(j0 + jj) * m + i0 + ii] = v;
            }
            PSD_SYNC();
            if (flag[0] != 0.0) return false;
        }
    }
    return true;
}

PSD_D void psd_bsyl_solve_real(const psd_bsyl_args& g) {
    const int q = PSD_BLOCK_X, n = g.n, p = g.p;
    if (!g.act[q]) return;
    const int m = g.m[q], k = n - m;
    if (m <= 0 || k <= 0) return;
    const bool left = g.left != 0, trans = g.ptrans ? g.ptrans[q] == 2 : g.trans != 0;
    double* X = g.X + (size_t)q * p * g.xb;
    if (psd_bsyl_real_range(g.T + (size_t)q * p * n * n, X, g.xb, n, p, m, g.qsub, left, trans, g.fromT,
                            psd_bsyl_range{0, m, 0, k}))
        return;
    PSD_ONE { g.info[q] = PSD_INFO_SINGULAR; }
    psd_bsyl_poison<false>(X, g.xb, p, m * k);
}

PSD_D bool psd_bsyl_cplx_range(const double* Td, double* Xd, size_t xb, int n, int p, int m, bool left, bool trans, int fromT,
                               const psd_bsyl_range rg) {
    PSD_LDS_DECL;
    const size_t nn = (size_t)n * n;
    const int mt = rg.i1 - rg.i0, kt = rg.j1 - rg.j0;
    const psd_z* T = (const psd_z*)Td;
    psd_z* X = (psd_z*)Xd;
    const int lstride = 8 * p + 1;  // a lane's eight arrays of p (the odd stride spreads the lanes over the banks)
    psd_z* lanes = (psd_z*)psd_lds;
    double* flag = (double*)(lanes + (size_t)64 * lstride);
    if (fromT) {
        for (int l = 0; l < p; ++l) {
            PSD_PAR_FOR(t, mt * kt) {
                const int i = rg.i0 + t % mt, j = rg.j0 + t / mt;
                X[(size_t)l * xb + (size_t)j * m + i] = zneg(T[(size_t)l * nn + (size_t)(m + j) * n + i]);
            }
        }
    }
    PSD_ONE { flag[0] = 0.0; }
    PSD_SYNC();
    // anti-diagonal d: the entries with ri + cj = d, ri counted from the bottom row and cj from the left column (S^H:
    // from the top row and the right column)
    for (int d = 0; d <= mt + kt - 2; ++d) {
        const int rlo = d - (kt - 1) > 0 ? d - (kt - 1) : 0, rhi = d < mt - 1 ? d : mt - 1;
        PSD_PAR_FOR(t, rhi - rlo + 1) {
            const int ri = rlo + t, cj = d - ri;
            const int i = trans ? rg.i0 + ri : rg.i1 - 1 - ri, j = trans ? rg.j1 - 1 - cj : rg.j0 + cj;
            psd_z* w = lanes + (size_t)(t & 63) * lstride;
            psd_z *ca = w, *cb = w + p, *cc = w + 2 * p, *cx = w + 3 * p;
            psd_z pa = zmk(1.0, 0.0), pb = zmk(1.0, 0.0);  // (in the order of the factors, whatever the chain's is)
            for (int l = 0; l < p; ++l) {
                pa = zmul(pa, T[(size_t)l * nn + (size_t)i * n + i]);
                pb = zmul(pb, T[(size_t)l * nn + (size_t)(m + j) * n + m + j]);
            }
            for (int e = 0; e < p; ++e) {
                const psd_bsyl_eq eq = psd_bsyl_equation(e, p, left, trans);
                const psd_z* A = T + (size_t)eq.fa * nn;
                const psd_z* B = T + (size_t)eq.fb * nn;
                const psd_z* Xa = X + (size_t)eq.ua * xb;
                const psd_z* Xb = X + (size_t)eq.ub * xb;
                psd_z s = X[(size_t)e * xb + (size_t)j * m + i];
                if (!trans) {
                    for (int r = i + 1; r < rg.i1; ++r) s = zsub(s, zmul(A[(size_t)r * n + i], Xa[(size_t)j * m + r]));
                    for (int r = rg.j0; r < j; ++r) s = zadd(s, zmul(Xb[(size_t)r * m + i], B[(size_t)(m + j) * n + m + r]));
                } else {
                    for (int r = rg.i0; r < i; ++r) s = zsub(s, zmul(zconj(A[(size_t)i * n + r]), Xa[(size_t)j * m + r]));
                    for (int r = j + 1; r < rg.j1; ++r)
                        s = zadd(s, zmul(Xb[(size_t)r * m + i], zconj(B[(size_t)(m + r) * n + m + j])));
                }
                psd_z a = A[(size_t)i * n + i], b = B[(size_t)(m + j) * n + m + j];
                if (trans) {
                    a = zconj(a);
                    b = zconj(b);
                }
                // psd_ord_cycsolve takes (A, B, C) of A x_k - B x_{k+1} = -C:  'L' a x_k - x_{k+1} b = s;  'R'
                // a x_{k+1} - x_k b = s, that is (-b) x_k - (-a) x_{k+1} = s
                const int kp = trans ? p - 1 - e : e;
                ca[kp] = left ? a : zneg(b);
                cb[kp] = left ? b : zneg(a);
                cc[kp] = zneg(s);
            }
            bool ok = !(pa.re == pb.re && pa.im == pb.im && psd_bsyl_finite(pa.re) && psd_bsyl_finite(pa.im) && !ziszero(pa));
            if (ok) ok = psd_ord_cycsolve(p, ca, cb, cc, cx, w + 4 * p, w + 5 * p, w + 6 * p, w + 7 * p);
            for (int kp = 0; kp < p; ++kp) {
                const psd_bsyl_eq eq = psd_bsyl_equation(trans ? p - 1 - kp : kp, p, left, trans);
                const psd_z v = ok ? cx[kp] : zmk(NAN, NAN);
                if (!(psd_bsyl_finite(v.re) && psd_bsyl_finite(v.im))) flag[0] = 1.0;
                X[(size_t)(left ? eq.ua : eq.ub) * xb + (size_t)j * m + i] = v;
            }
        }
        PSD_SYNC();
        if (flag[0] != 0.0) return false;
    }
    return true;
}

PSD_D void psd_bsyl_solve_cplx(const psd_bsyl_args& g) {
    const int q = PSD_BLOCK_X, n = g.n, p = g.p;
    if (!g.act[q]) return;
    const int m = g.m[q], k = n - m;
    if (m <= 0 || k <= 0) return;
    const bool left = g.left != 0, trans = g.ptrans ? g.ptrans[q] == 2 : g.trans != 0;
    double* X = g.X + (size_t)q * p * g.xb * 2;
    if (psd_bsyl_cplx_range(g.T + (size_t)q * p * n * n * 2, X, g.xb, n, p, m, left, trans, g.fromT, psd_bsyl_range{0, m, 0, k}))
        return;
    PSD_ONE { g.info[q] = PSD_INFO_SINGULAR; }
    psd_bsyl_poison<true>(X, g.xb, p, m * k);
}

template <bool CPLX>
PSD_KERNEL_B(64) psd_bsyl_solve(psd_bsyl_args g) {
    if (CPLX) psd_bsyl_solve_cplx(g);
    else psd_bsyl_solve_real(g);
}

// bad[q] = 1 where the split m[q] cuts a 2x2 block of the quasi-triangular factor (Float64): grid ceil(nb / 64)
PSD_KERNEL_B(64) psd_bsyl_split(const double* T, const int* m, int* bad, int nb, int n, int p, int qsub) {
    PSD_PAR_FOR(t, 64) {
        const int q = PSD_BLOCK_X * 64 + t;
        if (q < nb) {
            const int mq = m[q];
            const double* Tq = T + ((size_t)q * p + qsub) * n * n;
            bad[q] = (mq > 0 && mq < n && Tq[(size_t)(mq - 1) * n + mq] != 0.0) ? 1 : 0;
        }
    }
}

struct psd_bsyl_norm_args {
    const double* X;  // as psd_bsyl_args
    const int* m;
    const int* act;
    double* s;        // [gc][p]
    size_t xb;
    int n, p;
};

#define PSD_BSYL_RED_LDS (2 * 64 * sizeof(double))

// s[q][l] = 1 / sqrt(1 + ||X_l||_F^2): grid gc * p, one wavefront each; a lane's stride over the entries ascending, then
// the halving tree.  The rows of inactive and trivial problems are the host's.
template <bool CPLX>
PSD_KERNEL_B(64) psd_bsyl_norms(psd_bsyl_norm_args g) {
    PSD_LDS_DECL;
    double* red = (double*)psd_lds;
    constexpr int E = CPLX ? 2 : 1;
    const int q = PSD_BLOCK_X / g.p, l = PSD_BLOCK_X - q * g.p;
    if (!g.act[q]) return;
    const int m = g.m[q], mk = m * (g.n - m);
    if (mk <= 0) return;
    const double* x = g.X + ((size_t)q * g.p + l) * g.xb * E;
    PSD_PAR_FOR(t, 64) {
        double s = 0.0;
        for (int i = t; i < mk * E; i += 64) s += x[i] * x[i];
        red[t] = s;
    }
    PSD_SYNC();
    for (int h = 32; h > 0; h >>= 1) {
        PSD_PAR_FOR(t, h) { red[t] += red[t + h]; }
        PSD_SYNC();
    }
    PSD_ONE { g.s[(size_t)q * g.p + l] = 1.0 / sqrt(1.0 + red[0]); }
}

// ---- the estimator ---------------------------------------------------------------------------------------------------
// xLACN2 in reverse communication, the state of a problem between two solves.  state: ISAVE(1), 0 before the first step;
// j: ISAVE(2), 0-based; iter: ISAVE(3); kase: what the next solve applies (1: S^-1, 2: S^-H), 0 when the problem is done.
struct psd_bsyl_est {
    int state, j, iter, kase;
    double est;
};

struct psd_bsyl_est_args {
    double* X;   // [gc][p][xb] elements: the estimator's vector x, stacked in user order, each block column-major
    double* SG;  // Float64: the sign vector ISGN, as X
    const int* m;
    const int* act;
    psd_bsyl_est* rec;  // [gc]
    int* kase;          // [gc]: rec[q].kase, where the solve reads it
    size_t xb;
    int n, p;
};

#define PSD_BSYL_EST_LDS (3 * 64 * sizeof(double))

template <bool CPLX>
PSD_D double psd_bsyl_abs(const double* x, size_t o) {
    return CPLX ? hypot(x[2 * o], x[2 * o + 1]) : fabs(x[o]);
}

// One step for every active problem: grid gc, one wavefront each.  The entry i of the stacked vector is element
// (i % mk) of block i / mk.  Sums: a lane's stride ascending, then the halving tree; the first largest entry: the same
// tree on (value, index), the smaller index winning a tie.
template <bool CPLX>
PSD_KERNEL_B(64) psd_bsyl_est_step(psd_bsyl_est_args g) {
    PSD_LDS_DECL;
    double* red = (double*)psd_lds;  // [64] sums / values, [64] indices, [64] flags
    constexpr int E = CPLX ? 2 : 1;
    const int q = PSD_BLOCK_X;
    if (!g.act[q]) return;
    const int m = g.m[q], mk = m * (g.n - m), N = g.p * mk;
    if (mk <= 0) return;
    double* X = g.X + (size_t)q * g.p * g.xb * E;
    double* SG = g.SG ? g.SG + (size_t)q * g.p * g.xb : nullptr;
    psd_bsyl_est r = g.rec[q];
    auto at = [&](int i) { return (size_t)(i / mk) * g.xb + (size_t)(i % mk); };
    auto tree = [&]() {
        PSD_SYNC();
        for (int h = 32; h > 0; h >>= 1) {
            PSD_PAR_FOR(t, h) { red[t] += red[t + h]; }
            PSD_SYNC();
        }
    };
    auto sum1 = [&]() {  // sum |x_i|
        PSD_PAR_FOR(t, 64) {
            double s = 0.0;
            for (int i = t; i < N; i += 64) s += psd_bsyl_abs<CPLX>(X, at(i));
            red[t] = s;
        }
        tree();
        const double s = red[0];
        PSD_SYNC();
        return s;
    };
    auto imax1 = [&]() {  // the first i with the largest |x_i|
        PSD_PAR_FOR(t, 64) {
            double v = -1.0;
            int ix = N;
            for (int i = t; i < N; i += 64) {
                const double a = psd_bsyl_abs<CPLX>(X, at(i));
                if (a > v) {
                    v = a;
                    ix = i;
                }
            }
            red[t] = v;
            red[64 + t] = (double)ix;
        }
        PSD_SYNC();
        for (int h = 32; h > 0; h >>= 1) {
            PSD_PAR_FOR(t, h) {
                const double v2 = red[t + h], i2 = red[64 + t + h];
                if (v2 > red[t] || (v2 == red[t] && i2 < red[64 + t])) {
                    red[t] = v2;
                    red[64 + t] = i2;
                }
            }
            PSD_SYNC();
        }
        const int ix = (int)red[64];
        PSD_SYNC();
        return ix < N ? ix : 0;
    };
    auto unit = [&](int j) {  // x = e_j
        PSD_PAR_FOR(i, N) {
            const size_t o = at(i);
            X[E * o] = i == j ? 1.0 : 0.0;
            if (CPLX) X[E * o + 1] = 0.0;
        }
    };
    // x_i = sign(x_i) (complex: x_i / |x_i|); Float64: returns whether the sign vector is the one of the last time, and
    // keeps the new one
    auto signs = [&](bool compare) {
        PSD_PAR_FOR(t, 64) { red[128 + t] = 0.0; }
        PSD_SYNC();
        PSD_PAR_FOR(t, 64) {
            for (int i = t; i < N; i += 64) {
                const size_t o = at(i);
                if (CPLX) {
                    const double a = hypot(X[2 * o], X[2 * o + 1]);
                    if (a > PSD_DBL_MIN) {
                        X[2 * o] /= a;
                        X[2 * o + 1] /= a;
                    } else {
                        X[2 * o] = 1.0;
                        X[2 * o + 1] = 0.0;
                    }
                } else {
                    const double sg = X[o] > 0.0 ? 1.0 : -1.0;
                    if (compare && SG[o] != sg) red[128 + t] = 1.0;
                    X[o] = sg;
                    SG[o] = sg;
                }
            }
        }
        PSD_SYNC();
        bool same = compare;
        for (int t = 0; t < 64; ++t)
            if (red[128 + t] != 0.0) same = false;
        PSD_SYNC();
        return same;
    };
    bool final_vector = false;
    if (r.state == 0) {
        PSD_PAR_FOR(i, N) {
            const size_t o = at(i);
            X[E * o] = 1.0 / (double)N;
            if (CPLX) X[E * o + 1] = 0.0;
        }
        r.state = 1;
        r.kase = 1;
    } else if (r.state == 1) {
        r.est = sum1();
        if (N == 1) {
            r.kase = 0;
        } else {
            (void)signs(false);
            r.state = 2;
            r.kase = 2;
        }
    } else if (r.state == 2) {
        r.j = imax1();
        r.iter = 2;
        unit(r.j);
        r.state = 3;
        r.kase = 1;
    } else if (r.state == 3) {
        const double estold = r.est;
        r.est = sum1();
        bool stop = !(r.est > estold);  // (a NaN ends the iteration too; the host sees it in est)
        if (!CPLX && !stop) {
            // (xLACN2 compares the signs first and stores the new vector only when it goes on; the comparison is all
            // that is needed of the old one when it stops)
            stop = signs(true);
        } else if (!stop) {
            (void)signs(false);
        }
        if (stop) {
            final_vector = true;
        } else {
            r.state = 4;
            r.kase = 2;
        }
    } else if (r.state == 4) {
        const int jlast = r.j;
        r.j = imax1();
        const double a = CPLX ? psd_bsyl_abs<CPLX>(X, at(jlast)) : X[at(jlast)];
        const double b = psd_bsyl_abs<CPLX>(X, at(r.j));
        if (a != b && r.iter < PSD_BSYL_ITMAX) {
            r.iter += 1;
            unit(r.j);
            r.state = 3;
            r.kase = 1;
        } else {
            final_vector = true;
        }
    } else if (r.state == 5) {
        const double temp = 2.0 * (sum1() / (double)(3 * (size_t)N));
        if (temp > r.est) r.est = temp;
        r.kase = 0;
    }
    if (final_vector) {  // x_i = (-1)^i (1 + i / (N - 1))
        PSD_PAR_FOR(i, N) {
            const size_t o = at(i);
            X[E * o] = ((i & 1) ? -1.0 : 1.0) * (1.0 + (double)i / (double)(N - 1));
            if (CPLX) X[E * o + 1] = 0.0;
        }
        r.state = 5;
        r.kase = 1;
    }
    PSD_SYNC();
    PSD_ONE {
        g.rec[q] = r;
        g.kase[q] = r.kase;
    }
}
