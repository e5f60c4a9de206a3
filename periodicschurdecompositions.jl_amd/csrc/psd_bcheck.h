// Batched device-side verifier: checkpsd(P, As; thresh, strict) — src/diagnostics.jl:190-263 — for MANY decompositions
// of one shape (n, p) in ONE launch.  The single form (psd_check.h) takes four launches per factor on 64 x 64 tiles and
// sends W = T_l Z_b' through HBM; here one 256-thread workgroup owns one pair (problem q, factor l) and leaves
//   acc[(q * p + l) * 4 + 0] = || tril(T_l, -1) ||_F^2   (tril(., -2) for the quasi-triangular factor of a real one)
//   acc[(q * p + l) * 4 + 1] = opnorm(A_l, 1)
//   acc[(q * p + l) * 4 + 2] = || Z_l Z_l' - I ||_F^2
//   acc[(q * p + l) * 4 + 3] = || Z_a T_l Z_b' - A_l ||_F^2,   (a, b) from the table ab (the host applies the rule of
//                                                              diagnostics.jl:249-253 once per call)
// The three products run on the matrix cores (v_mfma_f64_16x16x4_f64, the fragment maps of psd_ck_gemm) over
// ceil(n / 16) tiles per dimension, dealt to the four wavefronts: n = 8 is one tile, n = 64 sixteen (four per wavefront).
// Operands are streamed from global memory in K-steps of 16 through two staging buffers (every operand is staged as
// X(x, k0 + k) -> buf[k][x], contiguous in x; a conjugate transpose is a sign at the use); partial tiles are zero-padded
// there and masked in the epilogues.  W is written from the accumulators into LDS and read from there as the right
// operand of the second product; A_l is read once, in that product's epilogue.  Z_l is one of Z_a and Z_b, so the
// orthogonality product rides on the staging of the product that has it.  ComplexF64: four real products on
// de-interleaved planes.
//
// Every sum has a fixed order — registers of a lane, lanes of a wavefront (butterfly), wavefronts through LDS — and one
// thread stores the four numbers of the factor: no floating-point atomics, nothing shared between workgroups.  A
// factor's numbers therefore do not depend on nb, on the problem's place in the batch or on the grouping, bit for bit.
//
// LDS: (n16 + 32) rows of ld doubles per plane (W and the two staging buffers; n16 = 16 ceil(n / 16), ld = n16 padded
// so that consecutive k rows of a fragment fall into different bank halves) + 16 doubles: 60 KB for Float64 at n = 64,
// 120 KB for ComplexF64 (W alone: 40 / 80 KB), 4.6 KB at n = 8.
#pragma once
#include "psd_complex.h"
#ifdef PSD_HOSTSIM
#include <vector>
#endif

#define PSD_BCK_NMAX 64
#define PSD_BCK_NT 256
#define PSD_BCK_TK 16

struct psd_bck_args {
    const double* T;  // [g][p][n][n] column-major blocks in user order (complex: interleaved), read only
    const double* Z;
    const double* A;
    const int* ab;  // [p][2]: the factors a, b of the residual Z_a T_l Z_b' - A_l
    double* acc;    // [g * p][4]
    int n, p;
    int qsub;  // the quasi-triangular factor of a real decomposition (0-based; -1: none)
};

PSD_HD int psd_bck_n16(int n) { return (n + 15) / 16 * 16; }
PSD_HD int psd_bck_ld(int n16) { return (n16 % 32 == 16) ? n16 : n16 + 16; }
inline size_t psd_bck_lds_bytes(int n, bool cplx) {
    const int n16 = psd_bck_n16(n);
    return sizeof(double) * ((size_t)(cplx ? 2 : 1) * (n16 + 2 * PSD_BCK_TK) * psd_bck_ld(n16) + 16);
}

#ifndef PSD_HOSTSIM
typedef double psd_bck_d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double psd_bck_wave_sum(double v) {  // every lane receives the same bits
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// buf[k][x] = X(x, k0 + k), x < n16, k < 16 (zero beyond n); planes re | im
template <bool CPLX>
__device__ __forceinline__ void psd_bck_stage(double* buf, size_t plane, const double* X, int n, int n16, int ld, int k0) {
    for (int e = threadIdx.x; e < PSD_BCK_TK * n16; e += PSD_BCK_NT) {
        const int k = e / n16, x = e - k * n16;
        double re = 0.0, im = 0.0;
        if (x < n && k0 + k < n) {
            const size_t o = (size_t)(k0 + k) * n + x;
            if (CPLX) {
                re = X[2 * o];
                im = X[2 * o + 1];
            } else {
                re = X[o];
            }
        }
        buf[k * ld + x] = re;
        if (CPLX) buf[plane + k * ld + x] = im;
    }
}

// C += L op(R) over one K-step for the tiles of this wavefront: L[k][i], R[k][j] are rows of ld doubles (planes re | im at
// lplane / rplane); rs = -1: R is used conjugated
template <bool CPLX>
__device__ __forceinline__ void psd_bck_mma(psd_bck_d4 (&cr)[4], psd_bck_d4 (&ci)[4], const double* L, size_t lplane,
                                            const double* R, size_t rplane, double rs, int ld, int nt, int wave, int lane) {
    const int col = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int t = wave + 4 * s;
        if (t >= nt * nt) break;
        const int ti = t % nt, tj = t / nt;
#pragma unroll
        for (int kk = 0; kk < PSD_BCK_TK; kk += 4) {
            const int lo = (kk + kq) * ld + 16 * ti + col, ro = (kk + kq) * ld + 16 * tj + col;
            const double ar = L[lo], br = R[ro];
            cr[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, cr[s], 0, 0, 0);
            if (CPLX) {
                const double ai = L[lplane + lo], bi = rs * R[rplane + ro];
                cr[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, bi, cr[s], 0, 0, 0);
                ci[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ci[s], 0, 0, 0);
                ci[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ci[s], 0, 0, 0);
            }
        }
    }
}

template <bool CPLX>
__global__ void __launch_bounds__(PSD_BCK_NT) psd_bck_check(psd_bck_args g) {
    extern __shared__ __attribute__((aligned(16))) char psd_bck_lds[];
    constexpr int E = CPLX ? 2 : 1;
    const int n = g.n, p = g.p;
    const int n16 = psd_bck_n16(n), nt = n16 / 16, ld = psd_bck_ld(n16);
    const int f = blockIdx.x, l = f % p;
    const size_t nn = (size_t)n * n * E, base = (size_t)(f - l) * nn;  // the blocks of this factor's problem
    const int a = g.ab[2 * l], b = g.ab[2 * l + 1];
    const double* Tl = g.T + base + (size_t)l * nn;
    const double* Al = g.A + base + (size_t)l * nn;
    const double* Za = g.Z + base + (size_t)a * nn;
    const double* Zb = g.Z + base + (size_t)b * nn;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // planes: W [n16][ld] | Ls [16][ld] | Rs [16][ld], the imaginary planes behind all three
    double* Ws = (double*)psd_bck_lds;
    double* Ls = Ws + (size_t)n16 * ld;
    double* Rs = Ls + (size_t)PSD_BCK_TK * ld;
    const size_t plane = (size_t)(n16 + 2 * PSD_BCK_TK) * ld;
    double* red = Ws + E * plane;  // [4][4]

    // triangularity and 1-norm: a wavefront per column, a lane per row
    const int sub = (!CPLX && l == g.qsub) ? 1 : 0;  // diagnostics.jl:225-235
    double ts = 0.0, best = 0.0;
    for (int c = wave; c < n; c += 4) {
        double av = 0.0;
        if (lane < n) {
            const size_t o = (size_t)c * n + lane;
            if (CPLX) {
                const double tr = Tl[2 * o], ti = Tl[2 * o + 1];
                if (lane > c + sub) ts += tr * tr + ti * ti;
                av = hypot(Al[2 * o], Al[2 * o + 1]);
            } else {
                const double tr = Tl[o];
                if (lane > c + sub) ts += tr * tr;
                av = fabs(Al[o]);
            }
        }
        const double s = psd_bck_wave_sum(av);
        if (s > best) best = s;
    }
    ts = psd_bck_wave_sum(ts);

    psd_bck_d4 wr[4], wi[4], orr[4], oi[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        wr[s] = psd_bck_d4{0.0, 0.0, 0.0, 0.0};
        wi[s] = psd_bck_d4{0.0, 0.0, 0.0, 0.0};
        orr[s] = psd_bck_d4{0.0, 0.0, 0.0, 0.0};
        oi[s] = psd_bck_d4{0.0, 0.0, 0.0, 0.0};
    }
    const bool orth1 = (b == l);  // Z_l Z_l' rides on the first product (its right operand) or on the second (its left)
    // W = T_l Z_b'
    for (int k0 = 0; k0 < n16; k0 += PSD_BCK_TK) {
        psd_bck_stage<CPLX>(Ls, plane, Tl, n, n16, ld, k0);
        psd_bck_stage<CPLX>(Rs, plane, Zb, n, n16, ld, k0);
        __syncthreads();
        psd_bck_mma<CPLX>(wr, wi, Ls, plane, Rs, plane, -1.0, ld, nt, wave, lane);
        if (orth1) psd_bck_mma<CPLX>(orr, oi, Rs, plane, Rs, plane, -1.0, ld, nt, wave, lane);
        __syncthreads();
    }
    // C/D fragment: col = lane & 15, row = (lane >> 4) + 4 * reg.  The padding of W is exact zeros (zero-padded operands).
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int t = wave + 4 * s;
        if (t >= nt * nt) break;
        const int ti = t % nt, tj = t / nt;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = (16 * ti + (lane >> 4) + 4 * r) * ld + 16 * tj + (lane & 15);
            Ws[o] = wr[s][r];
            if (CPLX) Ws[plane + o] = wi[s][r];
            wr[s][r] = 0.0;
            wi[s][r] = 0.0;
        }
    }
    __syncthreads();
    // R = Z_a W
    for (int k0 = 0; k0 < n16; k0 += PSD_BCK_TK) {
        psd_bck_stage<CPLX>(Ls, plane, Za, n, n16, ld, k0);
        __syncthreads();
        psd_bck_mma<CPLX>(wr, wi, Ls, plane, Ws + (size_t)k0 * ld, plane, 1.0, ld, nt, wave, lane);
        if (!orth1) psd_bck_mma<CPLX>(orr, oi, Ls, plane, Ls, plane, -1.0, ld, nt, wave, lane);
        __syncthreads();
    }
    double so = 0.0, sr = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int t = wave + 4 * s;
        if (t >= nt * nt) break;
        const int ti = t % nt, tj = t / nt;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * ti + (lane >> 4) + 4 * r, j = 16 * tj + (lane & 15);
            if (i >= n || j >= n) continue;
            const size_t o = (size_t)j * n + i;
            double vr = wr[s][r], vi = CPLX ? wi[s][r] : 0.0;
            if (CPLX) {
                vr -= Al[2 * o];
                vi -= Al[2 * o + 1];
            } else {
                vr -= Al[o];
            }
            sr += vr * vr + vi * vi;
            const double ur = orr[s][r] - (i == j ? 1.0 : 0.0), ui = CPLX ? oi[s][r] : 0.0;
            so += ur * ur + ui * ui;
        }
    }
    so = psd_bck_wave_sum(so);
    sr = psd_bck_wave_sum(sr);
    if (lane == 0) {
        red[4 * wave + 0] = ts;
        red[4 * wave + 1] = best;
        red[4 * wave + 2] = so;
        red[4 * wave + 3] = sr;
    }
    __syncthreads();
    if (tid == 0) {
        double m = red[1];
        for (int w = 1; w < 4; ++w)
            if (red[4 * w + 1] > m) m = red[4 * w + 1];
        double* out = g.acc + 4 * (size_t)f;
        out[0] = ((red[0] + red[4]) + red[8]) + red[12];
        out[1] = m;
        out[2] = ((red[2] + red[6]) + red[10]) + red[14];
        out[3] = ((red[3] + red[7]) + red[11]) + red[15];
    }
}
#else
// test-tier stand-in for the matrix-core kernel (plain loops, same argument block): one call per launch, every
// (problem, factor) pair in turn; W is rounded to working precision, as on the device.
template <bool CPLX>
static void psd_bck_check_sim(const psd_bck_args& g, int nfac) {
    constexpr int E = CPLX ? 2 : 1;
    const int n = g.n, p = g.p;
    const size_t nn = (size_t)n * n * E;
    std::vector<double> W(nn);
    // C = X op(Y) (conj: Y' for the right operand), column-major, optionally minus D or the identity; returns ||.||_F^2
    auto prod = [&](const double* X, const double* Y, bool conjt, double* Cout, const double* D, bool eye) {
        double ss = 0.0;
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) {
                double vr = 0.0, vi = 0.0;
                for (int k = 0; k < n; ++k) {
                    const size_t ox = (size_t)k * n + i, oy = conjt ? (size_t)k * n + j : (size_t)j * n + k;
                    if (CPLX) {
                        const double xr = X[2 * ox], xi = X[2 * ox + 1];
                        const double yr = Y[2 * oy], yi = conjt ? -Y[2 * oy + 1] : Y[2 * oy + 1];
                        vr += xr * yr;
                        vr += -xi * yi;
                        vi += xr * yi;
                        vi += xi * yr;
                    } else {
                        vr += X[ox] * Y[oy];
                    }
                }
                const size_t o = (size_t)j * n + i;
                if (Cout) {
                    Cout[E * o] = vr;
                    if (CPLX) Cout[2 * o + 1] = vi;
                    continue;
                }
                if (D) {
                    vr -= D[E * o];
                    if (CPLX) vi -= D[2 * o + 1];
                } else if (eye && i == j) {
                    vr -= 1.0;
                }
                ss += vr * vr + vi * vi;
            }
        return ss;
    };
    for (int f = 0; f < nfac; ++f) {
        const int l = f % p;
        const size_t base = (size_t)(f - l) * nn;
        const int a = g.ab[2 * l], b = g.ab[2 * l + 1];
        const double* Tl = g.T + base + (size_t)l * nn;
        const double* Al = g.A + base + (size_t)l * nn;
        const double* Zl = g.Z + base + (size_t)l * nn;
        const int sub = (!CPLX && l == g.qsub) ? 1 : 0;
        double ts = 0.0, best = 0.0;
        for (int c = 0; c < n; ++c) {
            double s = 0.0;
            for (int r = 0; r < n; ++r) {
                const size_t o = (size_t)c * n + r;
                if (r > c + sub)
                    for (int e = 0; e < E; ++e) ts += Tl[E * o + e] * Tl[E * o + e];
                s += CPLX ? hypot(Al[2 * o], Al[2 * o + 1]) : fabs(Al[o]);
            }
            if (s > best) best = s;
        }
        double* out = g.acc + 4 * (size_t)f;
        out[0] = ts;
        out[1] = best;
        out[2] = prod(Zl, Zl, true, nullptr, nullptr, true);
        prod(Tl, g.Z + base + (size_t)b * nn, true, W.data(), nullptr, false);
        out[3] = prod(g.Z + base + (size_t)a * nn, W.data(), false, nullptr, Al, false);
    }
}
#endif
