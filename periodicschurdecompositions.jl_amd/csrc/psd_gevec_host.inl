// Host driver of geigvecs (psd_gevec.h): eigenvectors of a signed or singular periodic Schur decomposition by periodic
// back-substitution, the periodic form of xTGEVC.  Included after psd_evec_host.inl (psd_devbuf, Timer, the launch
// sequence it shares).
//
// Argument checks, the diagonals of the factors (read once: the row-block map, the scalars a_l of every column and the
// pair scalars), the completion of `select` to whole pairs, the map of the user's factors and signature onto the working
// (left) form, workspace, the launches on the context's main stream and the read-back of the counters.
#include <complex>

namespace {

// g: [p][n][3] complex: T_l(i, i), T_l(i + 1, i), T_l(i, i + 1), from host matrices (hT) or the device block (dT)
template <bool CPLX>
int gev_gather(psd_ctx* c, int n, int p, const double* dT, double* const* hT, std::vector<std::complex<double>>& g) {
    constexpr int E = CPLX ? 2 : 1;
    const size_t np3 = (size_t)p * n * 3;
    std::vector<double> raw(np3 * E);
    if (hT) {
        for (int l = 0; l < p; ++l)
            for (int i = 0; i < n; ++i) {
                const size_t o = ((size_t)l * n + i) * 3;
                const size_t at[3] = {(size_t)i * n + i, (size_t)i * n + i + 1, (size_t)(i + 1) * n + i};
                for (int q = 0; q < 3; ++q)
                    for (int e = 0; e < E; ++e) raw[(o + q) * E + e] = (q == 0 || i + 1 < n) ? hT[l][at[q] * E + e] : 0.0;
            }
    } else {
        psd_devbuf b;
        PSD_CHECK(b.alloc(sizeof(double) * raw.size()));
        const int nb = (int)(((size_t)p * n + 63) / 64);
        PSD_LAUNCH(psd_gev_gather, psd_dim3(nb), 64, 0, c->stream, dT, n, p, E, b.d());
        PSD_CHECK(psd_rt_d2h(raw.data(), b.d(), sizeof(double) * raw.size(), c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
    }
    g.resize(np3);
    for (size_t q = 0; q < np3; ++q) g[q] = std::complex<double>(raw[q * E], CPLX ? raw[q * E + 1] : 0.0);
    return 0;
}

// The scalars a_l (user order, au [p]) of the solve column whose own block is the b rows from k.  dg(l, i, q): T_l(i, i),
// T_l(i + 1, i), T_l(i, i + 1) for q = 0, 1, 2; si: schurindex - 1; wmap, sgn: the working form.  A 1x1 block: the
// diagonal entries; returns whether one of them is zero (a zero or infinite eigenvalue).  A pair: sqrt|det B_l|, times
// e^(i arg lambda) at schurindex (e^(-i arg lambda) if that factor is inverted: the signed product is lambda).
template <class DG>
bool gev_scalars(int p, int si, const uint8_t* S, const int* wmap, const int* sgn, int k, int b, DG dg,
                 std::complex<double>* au) {
    using cd = std::complex<double>;
    if (b == 1) {
        bool z = false;
        for (int l = 0; l < p; ++l) {
            au[l] = dg(l, k, 0);
            z = z || dg(l, k, 0) == 0.0;
        }
        return z;
    }
    auto blk = [&](int l, double B[2][2]) {
        B[0][0] = dg(l, k, 0).real();
        B[0][1] = dg(l, k, 2).real();
        B[1][0] = l == si ? dg(l, k, 1).real() : 0.0;
        B[1][1] = dg(l, k + 1, 0).real();
    };
    // lambda of the first member (positive imaginary part) from the working product, renormalised at each step
    double M[2][2] = {{1.0, 0.0}, {0.0, 1.0}};
    for (int w = 0; w < p; ++w) {
        double B[2][2], F[2][2], R[2][2];
        blk(wmap[w], B);
        if (sgn[w]) {
            memcpy(F, B, sizeof(F));
        } else {
            F[0][0] = B[1][1];
            F[0][1] = -B[0][1];
            F[1][0] = -B[1][0];
            F[1][1] = B[0][0];  // adj(B), made a positive multiple of B^-1 (the argument of lambda is all we need)
            const double d = B[0][0] * B[1][1] - B[0][1] * B[1][0];
            if (d < 0)
                for (auto& r : F)
                    for (auto& v : r) v = -v;
        }
        double mx = 0.0;
        for (int q = 0; q < 2; ++q)
            for (int r = 0; r < 2; ++r) {
                R[q][r] = F[q][0] * M[0][r] + F[q][1] * M[1][r];
                mx = fmax(mx, fabs(R[q][r]));
            }
        for (int q = 0; q < 2; ++q)
            for (int r = 0; r < 2; ++r) M[q][r] = mx > 0.0 ? R[q][r] / mx : R[q][r];
    }
    const double h = 0.5 * (M[0][0] + M[1][1]), det = M[0][0] * M[1][1] - M[0][1] * M[1][0];
    const double th = atan2(sqrt(fmax(det - h * h, 0.0)), h);
    for (int l = 0; l < p; ++l) {
        double B[2][2];
        blk(l, B);
        const double r = sqrt(fabs(B[0][0] * B[1][1] - B[0][1] * B[1][0]));
        au[l] = l == si ? std::polar(r, (S && !S[si]) ? -th : th) : cd(r, 0.0);
    }
    return false;
}

// dT, dZ: [p][n][n] device blocks in user order; hT: host copies of the factors, or nullptr (read from dT); S: NULL or
// the user's signature; select completed in place; dV as eigvecs_dev; aout: p x maxvec complex (ld p), or nullptr.
template <bool CPLX>
int geigvecs_dev(psd_ctx* c, int n, int p, const double* dT, double* const* hT, const double* dZ, const uint8_t* S,
                 char orient, int schurindex, uint8_t* select, int shifted, double* dV, int maxvec, double* aout,
                 psd_evec_stats* st) {
    using cd = std::complex<double>;
    constexpr int E = CPLX ? 2 : 1;
    const size_t nn = (size_t)n * n;
    const bool left = orient == 'L';
    const int si = schurindex - 1;
    std::vector<cd> gd;
    if (int rc = gev_gather<CPLX>(c, n, p, dT, hT, gd)) return rc;
    auto dg = [&](int l, int i, int q) { return gd[((size_t)l * n + i) * 3 + q]; };  // q: 0 diag, 1 sub, 2 super
    // row blocks: 2x2 where the sub-diagonal of the quasi-triangular factor is non-zero (real decompositions)
    std::vector<int> bsz(n, 1);
    if (!CPLX)
        for (int i = 0; i + 1 < n; ++i)
            if (bsz[i] == 1 && dg(si, i, 1) != 0.0) {
                bsz[i] = 2;
                bsz[i + 1] = 0;
            }
    std::vector<int> k0, m, ke, ocol, pair;
    int nvec = 0;
    for (int i = 0; i < n; i += bsz[i]) {
        const int b = bsz[i];
        if (b == 2 && (select[i] || select[i + 1])) select[i] = select[i + 1] = 1;
        if (!select[i]) continue;
        k0.push_back(i);
        m.push_back(b);
        ke.push_back(i + b);
        ocol.push_back(nvec);
        pair.push_back(b == 2);
        nvec += b;
    }
    const int ns = (int)k0.size();
    if (st) st->nvec = nvec;
    if (!dV) return 0;
    if (nvec > maxvec) return -13;
    if (ns == 0) return 0;
    const int nmat = shifted ? p : 1;
    // working form: W_j = T_{wmap[j]}; x_l = y_{vmap[l]}; the signature follows the factors
    std::vector<int> wmap(p), vmap(p), ident(p), sgn(p), bmap(p);
    for (int j = 0; j < p; ++j) {
        wmap[j] = left ? j : p - 1 - j;
        vmap[j] = left ? j : (p - j) % p;
        ident[j] = j;
    }
    for (int j = 0; j < p; ++j) {
        sgn[j] = S ? (S[wmap[j]] ? 1 : 0) : 1;
        bmap[j] = sgn[j] ? j : (j + 1) % p;  // an inverted factor's update reads X_{j+1}
    }
    const int six = left ? si : p - schurindex;
    // the scalars a_l (user order) of every solve column
    std::vector<cd> au((size_t)p * ns);
    int nzero = 0;
    for (int j = 0; j < ns; ++j)
        nzero += gev_scalars(p, si, S, wmap.data(), sgn.data(), k0[j], m[j], dg, au.data() + (size_t)j * p);
    if (aout)
        for (int j = 0; j < ns; ++j)
            for (int l = 0; l < p; ++l) {
                const cd v = au[(size_t)j * p + l];
                const size_t o = 2 * ((size_t)ocol[j] * p + l);
                aout[o] = v.real();
                aout[o + 1] = v.imag();
                if (pair[j]) {
                    aout[o + 2 * p] = v.real();
                    aout[o + 2 * p + 1] = -v.imag();
                }
            }
    std::vector<double> ac(2 * (size_t)p * ns);
    for (int w = 0; w < p; ++w)
        for (int j = 0; j < ns; ++j) {
            const cd v = au[(size_t)j * p + wmap[w]];
            ac[2 * ((size_t)w * ns + j)] = v.real();
            ac[2 * ((size_t)w * ns + j) + 1] = v.imag();
        }
    // workspace: X and R planes, counters, the small tables, the scalars
    const size_t xs = (size_t)p * n * ns, rs = (size_t)p * PSD_EV_RB * ns;
    psd_devbuf bX, bR, bS, bI, bA;
    PSD_CHECK(bX.alloc(sizeof(double) * 2 * xs));
    PSD_CHECK(bR.alloc(sizeof(double) * 2 * rs));
    PSD_CHECK(bS.alloc(sizeof(double) * 2 * ns));
    PSD_CHECK(bA.alloc(sizeof(double) * ac.size()));
    const size_t ni = (size_t)n + 5 * p + 8 * (size_t)ns;
    PSD_CHECK(bI.alloc(sizeof(int) * ni));
    std::vector<int> htab;
    htab.reserve(ni);
    for (auto* v : {&bsz, &wmap, &vmap, &ident, &sgn, &bmap, &k0, &m, &ke, &ocol, &pair})
        htab.insert(htab.end(), v->begin(), v->end());
    htab.resize(ni, 0);  // (the counters: 3 per column)
    int* di = (int*)bI.p;
    const int *d_bsz = di, *d_wmap = di + n, *d_vmap = d_wmap + p, *d_ident = d_vmap + p, *d_sgn = d_ident + p,
              *d_bmap = d_sgn + p, *d_k0 = d_bmap + p, *d_m = d_k0 + ns, *d_ke = d_m + ns, *d_ocol = d_ke + ns,
              *d_pair = d_ocol + ns;
    int* d_cnt = di + n + 5 * p + 5 * ns;
    PSD_CHECK(psd_rt_h2d(di, htab.data(), sizeof(int) * ni, c->stream));
    PSD_CHECK(psd_rt_h2d(bA.d(), ac.data(), sizeof(double) * ac.size(), c->stream));
    double *Xr = bX.d(), *Xi = Xr + xs, *Rr = bR.d(), *Ri = Rr + rs, *sr = bS.d(), *si_ = sr + ns;
    Timer tsolve, tback;
    tsolve.start(c->stream);
    PSD_CHECK(psd_rt_memset(Xr, 0, sizeof(double) * 2 * xs, c->stream));
    psd_gev_args ga;
    memset(&ga, 0, sizeof(ga));
    psd_ev_args& a = ga.e;
    a.T = dT; a.wmap = d_wmap; a.bsz = d_bsz; a.k0 = d_k0; a.m = d_m; a.kend = d_ke;
    a.Xr = Xr; a.Xi = Xi; a.Rr = Rr; a.Ri = Ri; a.cnt = d_cnt;
    a.n = n; a.p = p; a.ns = ns; a.six = six;
    ga.sgn = d_sgn; ga.ac = bA.d();
    psd_ev_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.A = dT; g.Br = Xr; g.Bi = Xi; g.amap = d_wmap; g.bmap = d_bmap; g.cmap = d_ident; g.kend = d_ke;
    g.Cr = Rr; g.Ci = Ri; g.astride = nn * E; g.bstride = (size_t)n * ns; g.cstride = (size_t)PSD_EV_RB * ns;
    g.lda = n; g.ldb = ns; g.ncol = ns; g.mode = 0; g.crows = PSD_EV_RB;
    for (int r1 = n; r1 > 0;) {
        int r0 = r1 > PSD_EV_CH ? r1 - PSD_EV_CH : 0;
        if (bsz[r0] == 0) ++r0;
        int jlo = 0;
        while (jlo < ns && k0[jlo] < r0) ++jlo;
        if (jlo < ns) {
            g.i0 = r0; g.M = r1 - r0; g.kbeg = r1; g.jlo = jlo;
#ifdef PSD_HOSTSIM
            psd_ev_gemm_sim<CPLX>(g, p);
#else
            hipLaunchKernelGGL(psd_ev_gemm<CPLX>, dim3(1, (ns - jlo + PSD_EV_TN - 1) / PSD_EV_TN, p), dim3(256), 0,
                               c->stream, g);
#endif
            a.r0 = r0; a.r1 = r1; a.jlo = jlo;
            if (CPLX)
                PSD_LAUNCH(psd_gev_solve_z, psd_dim3(ns - jlo), 64, PSD_GEV_LDS, c->stream, ga);
            else
                PSD_LAUNCH(psd_gev_solve_d, psd_dim3(ns - jlo), 64, PSD_GEV_LDS, c->stream, ga);
        }
        r1 = r0;
    }
    const double ms_solve = tsolve.stop(c->stream);
    // back-transform V_l = Z_l x_l as eigvecs_dev: V_1, its norms and phases, then the other factors
    tback.start(c->stream);
    g.A = dZ; g.amap = d_ident; g.bmap = d_vmap; g.cmap = d_ident; g.Cr = dV; g.Ci = nullptr;
    g.cstride = 2 * (size_t)n * nvec; g.ldc = n; g.i0 = 0; g.M = n; g.kbeg = 0; g.jlo = 0; g.mode = 1;
    g.ocol = d_ocol; g.pair = d_pair; g.sr = nullptr; g.si = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        const int nz = pass == 0 ? 1 : nmat - 1;
        if (nz == 0) break;
        if (pass == 1) {
            g.amap = d_ident + 1; g.bmap = d_vmap + 1; g.cmap = d_ident + 1; g.sr = sr; g.si = si_;
        }
#ifdef PSD_HOSTSIM
        psd_ev_gemm_sim<CPLX>(g, nz);
#else
        hipLaunchKernelGGL(psd_ev_gemm<CPLX>, dim3((n + PSD_EV_RB - 1) / PSD_EV_RB, (ns + PSD_EV_TN - 1) / PSD_EV_TN, nz),
                           dim3(256), 0, c->stream, g);
#endif
        if (pass == 0)
            PSD_LAUNCH(psd_ev_norm, psd_dim3((ns + 63) / 64), 64, 0, c->stream, dV, n, ns, d_ocol, d_pair,
                       (const int*)d_cnt, sr, si_);
    }
    const double ms_back = tback.stop(c->stream);
    std::vector<int> cnt(3 * (size_t)ns);
    PSD_CHECK(psd_rt_d2h(cnt.data(), d_cnt, sizeof(int) * 3 * ns, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    if (st) {
        for (int j = 0; j < ns; ++j) {
            st->nperturbed += cnt[3 * j];
            st->nrescaled += cnt[3 * j + 1] > 0;
        }
        st->nzero = nzero;
        st->ms_solve = ms_solve;
        st->ms_backtransform = ms_back;
        st->ms_kernels = ms_solve + ms_back;
    }
    return 0;
}

int geigvecs_checked(psd_ctx* c, int n, int p, const void* T, const void* Z, char orient, int schurindex,
                     const uint8_t* select, int nsel, psd_evec_stats* st) {
    if (!c) return -1;
    if (n < 1) return -2;
    if (p < 1) return -3;
    if (!T) return -4;
    if (!Z) return -5;
    if (orient != 'L' && orient != 'R') return -7;
    if (schurindex < 1 || schurindex > p) return -8;
    if (!select || nsel != n) return -9;
    if (st) memset(st, 0, sizeof(*st));
    return 0;
}

template <bool CPLX>
int geigvecs_host(psd_ctx* c, int n, int p, double* const* T, double* const* Z, const uint8_t* S, char orient,
                  int schurindex, uint8_t* select, int nsel, int shifted, double* const* V, int maxvec, double* aout,
                  psd_evec_stats* stats, int* info) {
    psd_evec_stats local;
    psd_evec_stats* st = stats ? stats : &local;
    if ((*info = geigvecs_checked(c, n, p, T, Z, orient, schurindex, select, nsel, st)) != 0) return *info;
    if (!V)
        return *info = geigvecs_dev<CPLX>(c, n, p, nullptr, T, nullptr, S, orient, schurindex, select, shifted,
                                          nullptr, maxvec, nullptr, st);
    constexpr int E = CPLX ? 2 : 1;
    const size_t nn = (size_t)n * n * E;
    std::vector<uint8_t> sel(select, select + n);  // (the size first: V must hold the completed selection)
    if ((*info = geigvecs_dev<CPLX>(c, n, p, nullptr, T, nullptr, S, orient, schurindex, sel.data(), shifted, nullptr,
                                    maxvec, nullptr, st)) != 0)
        return *info;
    const int nvec = st->nvec, nmat = shifted ? p : 1;
    if (nvec > maxvec) return *info = -13;
    psd_devbuf bT, bZ, bV;
    PSD_CHECK(bT.alloc(nn * p * sizeof(double)));
    PSD_CHECK(bZ.alloc(nn * p * sizeof(double)));
    PSD_CHECK(bV.alloc(2 * (size_t)n * (nvec > 0 ? nvec : 1) * nmat * sizeof(double)));
    for (int l = 0; l < p; ++l) {
        PSD_CHECK(psd_rt_h2d(bT.d() + l * nn, T[l], nn * 8, c->stream));
        PSD_CHECK(psd_rt_h2d(bZ.d() + l * nn, Z[l], nn * 8, c->stream));
    }
    if ((*info = geigvecs_dev<CPLX>(c, n, p, bT.d(), T, bZ.d(), S, orient, schurindex, select, shifted, bV.d(), maxvec,
                                    aout, st)) != 0)
        return *info;
    for (int l = 0; l < nmat; ++l)
        PSD_CHECK(psd_rt_d2h(V[l], bV.d() + 2 * (size_t)l * n * nvec, 2 * (size_t)n * nvec * 8, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    return *info = 0;
}

template <bool CPLX>
int geigvecs_devcall(psd_ctx* c, int n, int p, const double* dT, const double* dZ, const uint8_t* S, char orient,
                     int schurindex, uint8_t* select, int nsel, int shifted, double* dV, int maxvec, double* aout,
                     psd_evec_stats* stats, int* info) {
    int dummy;
    if (!info) info = &dummy;
    psd_evec_stats local;
    psd_evec_stats* st = stats ? stats : &local;
    if ((*info = geigvecs_checked(c, n, p, dT, dZ, orient, schurindex, select, nsel, st)) != 0) return *info;
    return *info = geigvecs_dev<CPLX>(c, n, p, dT, nullptr, dZ, S, orient, schurindex, select, shifted, dV, maxvec, aout,
                                      st);
}

}  // namespace

extern "C" {

int psd_d_geigvecs(psd_ctx* c, int n, int p, double* const* T, double* const* Z, const uint8_t* S, char orient,
                   int schurindex, uint8_t* select, int nsel, int shifted, double* const* V, int maxvec, double* a,
                   psd_evec_stats* stats, int* info) {
    int dummy;
    return geigvecs_host<false>(c, n, p, T, Z, S, orient, schurindex, select, nsel, shifted, V, maxvec, a, stats,
                                info ? info : &dummy);
}

int psd_z_geigvecs(psd_ctx* c, int n, int p, double* const* T, double* const* Z, const uint8_t* S, char orient,
                   int schurindex, uint8_t* select, int nsel, int shifted, double* const* V, int maxvec, double* a,
                   psd_evec_stats* stats, int* info) {
    int dummy;
    return geigvecs_host<true>(c, n, p, T, Z, S, orient, schurindex, select, nsel, shifted, V, maxvec, a, stats,
                               info ? info : &dummy);
}

int psd_d_geigvecs_dev(psd_ctx* c, int n, int p, const double* dT, const double* dZ, const uint8_t* S, char orient,
                       int schurindex, uint8_t* select, int nsel, int shifted, double* dV, int maxvec, double* a,
                       psd_evec_stats* stats, int* info) {
    return geigvecs_devcall<false>(c, n, p, dT, dZ, S, orient, schurindex, select, nsel, shifted, dV, maxvec, a, stats,
                                   info);
}

int psd_z_geigvecs_dev(psd_ctx* c, int n, int p, const double* dT, const double* dZ, const uint8_t* S, char orient,
                       int schurindex, uint8_t* select, int nsel, int shifted, double* dV, int maxvec, double* a,
                       psd_evec_stats* stats, int* info) {
    return geigvecs_devcall<true>(c, n, p, dT, dZ, S, orient, schurindex, select, nsel, shifted, dV, maxvec, a, stats,
                                  info);
}

}  // extern "C"
