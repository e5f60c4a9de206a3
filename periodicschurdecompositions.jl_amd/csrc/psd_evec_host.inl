// Host driver of eigvecs(ps, select; shifted) by periodic back-substitution (psd_evec.h), src/vectors.jl:25-138 without
// the reordering.  Included at the end of psd_engine.cpp (one translation unit), after psd_check_host.inl (psd_devbuf).
//
// Argument checks, the completion of `select` to whole conjugate pairs (vectors.jl:42-62), the row-block map of the
// quasi-triangular factor, the map of the user's factors onto the working (left) form, workspace, the launches on the
// context's main stream and the read-back of the counters.
#include <complex>

namespace {

// lambda^(1/p), the principal root the reference takes: (values[k] + 0im)^(1/p) (vectors.jl:67)
static std::complex<double> psd_ev_root(std::complex<double> lam, int p) {
    if (lam == 0.0) return 0.0;
    const double r = pow(std::abs(lam), 1.0 / p), th = atan2(lam.imag() + 0.0, lam.real()) / p;
    return std::complex<double>(r * cos(th), r * sin(th));
}

// dT, dZ: [p][n][n] device blocks in user order (E doubles per element); lam: host, the n eigenvalues; select: n flags,
// completed to pairs in place; dV: nmat blocks of n x nvec (interleaved complex, column-major); dV == nullptr: only the
// completion and stats->nvec (a size query).  hTsi: a host copy of the quasi-triangular factor, or nullptr (read from dT).
// conjroot: the form is the flip-adjoint of a caller's (the left vectors of the batch entries, psd_lbevec.h) and lam the
// conjugates of the caller's eigenvalues: the root is conj(psd_ev_root(conj lam)), the conjugate of the caller's root.
template <bool CPLX>
int eigvecs_dev(psd_ctx* c, int n, int p, const double* dT, const double* dZ, const std::complex<double>* lam,
                char orient, int schurindex, uint8_t* select, int shifted, double* dV, int maxvec, psd_evec_stats* st,
                const double* hTsi = nullptr, bool conjroot = false) {
    constexpr int E = CPLX ? 2 : 1;
    const size_t nn = (size_t)n * n;
    const bool left = orient == 'L';
    // row blocks: 2x2 where the sub-diagonal of the quasi-triangular factor is non-zero (real decompositions)
    std::vector<int> bsz(n, 1);
    if (!CPLX && n > 1 && hTsi) {
        for (int i = 0; i + 1 < n; ++i)
            if (bsz[i] == 1 && hTsi[(size_t)i * n + i + 1] != 0.0) {
                bsz[i] = 2;
                bsz[i + 1] = 0;
            }
    } else if (!CPLX && n > 1) {
        psd_devbuf bsub;
        PSD_CHECK(bsub.alloc(sizeof(double) * n));
        PSD_LAUNCH(psd_ev_subdiag, psd_dim3((n + 63) / 64), 64, 0, c->stream, dT + (size_t)(schurindex - 1) * nn, n,
                   bsub.d());
        std::vector<double> sub(n);
        PSD_CHECK(psd_rt_d2h(sub.data(), bsub.d(), sizeof(double) * (n - 1), c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        for (int i = 0; i + 1 < n; ++i)
            if (bsz[i] == 1 && sub[i] != 0.0) {
                bsz[i] = 2;
                bsz[i + 1] = 0;
            }
    }
    // solve columns, top to bottom; a pair is one solve column and two output columns
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
    if (nvec > maxvec) return -10;
    if (ns == 0) return 0;
    const int nmat = shifted ? p : 1;
    // working form (left orientation): W_j = T_j, y_j = x_j; right: W_j = T_{p-1-j}, x_l = y_{(p-l) mod p} (0-based)
    std::vector<int> wmap(p), vmap(p), ident(p);
    for (int j = 0; j < p; ++j) {
        wmap[j] = left ? j : p - 1 - j;
        vmap[j] = left ? j : (p - j) % p;
        ident[j] = j;
    }
    const int six = left ? schurindex - 1 : p - schurindex;
    std::vector<double> mu(2 * ns), lamc(2 * ns), ev(2 * (size_t)n);
    for (int j = 0; j < ns; ++j) {
        const std::complex<double> l = lam[k0[j]];
        const std::complex<double> u = conjroot ? std::conj(psd_ev_root(std::conj(l), p)) : psd_ev_root(l, p);
        lamc[2 * j] = l.real();
        lamc[2 * j + 1] = l.imag();
        mu[2 * j] = u.real();
        mu[2 * j + 1] = u.imag();
    }
    for (int i = 0; i < n; ++i) {
        ev[2 * i] = lam[i].real();
        ev[2 * i + 1] = lam[i].imag();
    }
    // workspace: X and R planes, counters, the small tables
    const size_t xs = (size_t)p * n * ns, rs = (size_t)p * PSD_EV_RB * ns;
    psd_devbuf bX, bR, bS, bI, bD;
    PSD_CHECK(bX.alloc(sizeof(double) * 2 * xs));
    PSD_CHECK(bR.alloc(sizeof(double) * 2 * rs));
    PSD_CHECK(bS.alloc(sizeof(double) * 2 * ns));
    const size_t ni = (size_t)n + 3 * p + 8 * (size_t)ns;
    PSD_CHECK(bI.alloc(sizeof(int) * ni));
    PSD_CHECK(bD.alloc(sizeof(double) * (4 * (size_t)ns + 2 * (size_t)n)));
    std::vector<int> htab;
    htab.reserve(ni);
    for (auto* v : {&bsz, &wmap, &vmap, &ident, &k0, &m, &ke, &ocol, &pair}) htab.insert(htab.end(), v->begin(), v->end());
    htab.resize(ni, 0);  // (the counters: 3 per column)
    int* di = (int*)bI.p;
    const int *d_bsz = di, *d_wmap = di + n, *d_vmap = d_wmap + p, *d_ident = d_vmap + p, *d_k0 = d_ident + p,
              *d_m = d_k0 + ns, *d_ke = d_m + ns, *d_ocol = d_ke + ns, *d_pair = d_ocol + ns;
    int* d_cnt = di + n + 3 * p + 5 * ns;
    std::vector<double> hd(mu);
    hd.insert(hd.end(), lamc.begin(), lamc.end());
    hd.insert(hd.end(), ev.begin(), ev.end());
    double* dd = bD.d();
    PSD_CHECK(psd_rt_h2d(di, htab.data(), sizeof(int) * ni, c->stream));
    PSD_CHECK(psd_rt_h2d(dd, hd.data(), sizeof(double) * hd.size(), c->stream));
    double *Xr = bX.d(), *Xi = Xr + xs, *Rr = bR.d(), *Ri = Rr + rs, *sr = bS.d(), *si = sr + ns;
    Timer tsolve, tback;
    tsolve.start(c->stream);
    PSD_CHECK(psd_rt_memset(Xr, 0, sizeof(double) * 2 * xs, c->stream));
    psd_ev_args a;
    a.T = dT; a.wmap = d_wmap; a.bsz = d_bsz; a.k0 = d_k0; a.m = d_m; a.kend = d_ke;
    a.mu = dd; a.lam = dd + 2 * ns; a.ev = dd + 4 * ns;
    a.Xr = Xr; a.Xi = Xi; a.Rr = Rr; a.Ri = Ri; a.cnt = d_cnt;
    a.n = n; a.p = p; a.ns = ns; a.six = six;
    psd_ev_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.A = dT; g.Br = Xr; g.Bi = Xi; g.amap = d_wmap; g.bmap = d_ident; g.cmap = d_ident; g.kend = d_ke;
    g.Cr = Rr; g.Ci = Ri; g.astride = nn * E; g.bstride = (size_t)n * ns; g.cstride = (size_t)PSD_EV_RB * ns;
    g.lda = n; g.ldb = ns; g.ncol = ns; g.mode = 0; g.crows = PSD_EV_RB;
    // chunks of at most PSD_EV_CH rows, bottom up, never splitting a 2x2 block
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
                PSD_LAUNCH(psd_ev_solve_z, psd_dim3(ns - jlo), 64, PSD_EV_LDS, c->stream, a);
            else
                PSD_LAUNCH(psd_ev_solve_d, psd_dim3(ns - jlo), 64, PSD_EV_LDS, c->stream, a);
        }
        r1 = r0;
    }
    const double ms_solve = tsolve.stop(c->stream);
    // back-transform V_l = Z_l x_l: V_1 first, its norms and phases, then the other factors with the column factors
    tback.start(c->stream);
    g.A = dZ; g.amap = d_ident; g.bmap = d_vmap; g.cmap = d_ident; g.Cr = dV; g.Ci = nullptr;
    g.cstride = 2 * (size_t)n * nvec; g.ldc = n; g.i0 = 0; g.M = n; g.kbeg = 0; g.jlo = 0; g.mode = 1;
    g.ocol = d_ocol; g.pair = d_pair; g.sr = nullptr; g.si = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        const int nz = pass == 0 ? 1 : nmat - 1;
        if (nz == 0) break;
        if (pass == 1) {
            g.amap = d_ident + 1; g.bmap = d_vmap + 1; g.cmap = d_ident + 1; g.sr = sr; g.si = si;
        }
#ifdef PSD_HOSTSIM
        psd_ev_gemm_sim<CPLX>(g, nz);
#else
        hipLaunchKernelGGL(psd_ev_gemm<CPLX>, dim3((n + PSD_EV_RB - 1) / PSD_EV_RB, (ns + PSD_EV_TN - 1) / PSD_EV_TN, nz),
                           dim3(256), 0, c->stream, g);
#endif
        if (pass == 0)
            PSD_LAUNCH(psd_ev_norm, psd_dim3((ns + 63) / 64), 64, 0, c->stream, dV, n, ns, d_ocol, d_pair,
                       (const int*)d_cnt, sr, si);
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
            st->nzero += cnt[3 * j + 2];
        }
        st->ms_solve = ms_solve;
        st->ms_backtransform = ms_back;
        st->ms_kernels = ms_solve + ms_back;
    }
    return 0;
}

template <bool CPLX>
int eigvecs_checked(psd_ctx* c, int n, int p, const void* T, const void* Z, const std::complex<double>* lam,
                    const uint8_t* S, char orient, int schurindex, uint8_t* select, int nsel, psd_evec_stats* st) {
    if (!c) return -1;
    if (n < 1) return -2;
    if (p < 1) return -3;
    if (!T) return -4;
    if (!Z) return -5;
    if (!lam) return -6;
    if (orient != 'L' && orient != 'R') return -7;
    if (schurindex < 1 || schurindex > p) return -8;
    if (!select || nsel != n) return -9;
    if (S)
        for (int l = 0; l < p; ++l)
            if (!S[l]) return PSD_INFO_NOTIMPL;
    if (st) memset(st, 0, sizeof(*st));
    return 0;
}

template <bool CPLX>
int eigvecs_host(psd_ctx* c, int n, int p, double* const* T, double* const* Z, const std::complex<double>* lam,
                 const uint8_t* S, char orient, int schurindex, uint8_t* select, int nsel, int shifted, double* const* V,
                 int maxvec, psd_evec_stats* stats, int* info) {
    psd_evec_stats local;
    psd_evec_stats* st = stats ? stats : &local;
    if ((*info = eigvecs_checked<CPLX>(c, n, p, T, Z, lam, S, orient, schurindex, select, nsel, st)) != 0) return *info;
    constexpr int E = CPLX ? 2 : 1;
    const size_t nn = (size_t)n * n * E;
    const double* hTsi = T[schurindex - 1];
    if (!V) return *info = eigvecs_dev<CPLX>(c, n, p, nullptr, nullptr, lam, orient, schurindex, select, shifted,
                                             nullptr, maxvec, st, hTsi);
    std::vector<uint8_t> sel(select, select + n);  // (the size first: V must hold the completed selection)
    if ((*info = eigvecs_dev<CPLX>(c, n, p, nullptr, nullptr, lam, orient, schurindex, sel.data(), shifted, nullptr,
                                   maxvec, st, hTsi)) != 0)
        return *info;
    const int nvec = st->nvec, nmat = shifted ? p : 1;
    if (nvec > maxvec) return *info = -10;
    psd_devbuf bT, bZ, bV;
    PSD_CHECK(bT.alloc(nn * p * sizeof(double)));
    PSD_CHECK(bZ.alloc(nn * p * sizeof(double)));
    PSD_CHECK(bV.alloc(2 * (size_t)n * (nvec > 0 ? nvec : 1) * nmat * sizeof(double)));
    for (int l = 0; l < p; ++l) {
        PSD_CHECK(psd_rt_h2d(bT.d() + l * nn, T[l], nn * 8, c->stream));
        PSD_CHECK(psd_rt_h2d(bZ.d() + l * nn, Z[l], nn * 8, c->stream));
    }
    if ((*info = eigvecs_dev<CPLX>(c, n, p, bT.d(), bZ.d(), lam, orient, schurindex, select, shifted, bV.d(), maxvec,
                                   st, hTsi)) != 0)
        return *info;
    for (int l = 0; l < nmat; ++l)
        PSD_CHECK(psd_rt_d2h(V[l], bV.d() + 2 * (size_t)l * n * nvec, 2 * (size_t)n * nvec * 8, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    return *info = 0;
}

// the eigenvalues as complex numbers: wr + i wi, or alpha / beta * 2^ascale (generalized.jl:40-42)
static std::vector<std::complex<double>> psd_ev_values(int n, const double* wr, const double* wi, const double* alpha,
                                                       const double* beta, const int32_t* ascale) {
    std::vector<std::complex<double>> v;
    if (n < 1) return v;
    v.resize(n);
    for (int i = 0; i < n; ++i) {
        if (wr)
            v[i] = std::complex<double>(wr[i], wi[i]);
        else
            v[i] = std::complex<double>(alpha[2 * i], alpha[2 * i + 1]) / beta[i] * ldexp(1.0, ascale ? ascale[i] : 0);
    }
    return v;
}

}  // namespace

extern "C" {

int psd_d_eigvecs(psd_ctx* c, int n, int p, double* const* T, double* const* Z, const double* wr, const double* wi,
                  const uint8_t* S, char orient, int schurindex, uint8_t* select, int nsel, int shifted,
                  double* const* V, int maxvec, psd_evec_stats* stats, int* info) {
    int dummy;
    if (!info) info = &dummy;
    const auto lam = (wr && wi) ? psd_ev_values(n, wr, wi, nullptr, nullptr, nullptr) : std::vector<std::complex<double>>();
    return eigvecs_host<false>(c, n, p, T, Z, lam.empty() ? nullptr : lam.data(), S, orient, schurindex, select, nsel,
                               shifted, V, maxvec, stats, info);
}

int psd_z_eigvecs(psd_ctx* c, int n, int p, double* const* T, double* const* Z, const double* alpha, const double* beta,
                  const int32_t* ascale, const uint8_t* S, char orient, int schurindex, uint8_t* select, int nsel,
                  int shifted, double* const* V, int maxvec, psd_evec_stats* stats, int* info) {
    int dummy;
    if (!info) info = &dummy;
    const auto lam = (alpha && beta) ? psd_ev_values(n, nullptr, nullptr, alpha, beta, ascale)
                                     : std::vector<std::complex<double>>();
    return eigvecs_host<true>(c, n, p, T, Z, lam.empty() ? nullptr : lam.data(), S, orient, schurindex, select, nsel,
                              shifted, V, maxvec, stats, info);
}

int psd_d_eigvecs_dev(psd_ctx* c, int n, int p, const double* dT, const double* dZ, const double* wr, const double* wi,
                      const uint8_t* S, char orient, int schurindex, uint8_t* select, int nsel, int shifted, double* dV,
                      int maxvec, psd_evec_stats* stats, int* info) {
    int dummy;
    if (!info) info = &dummy;
    psd_evec_stats local;
    psd_evec_stats* st = stats ? stats : &local;
    const auto lam = (wr && wi) ? psd_ev_values(n, wr, wi, nullptr, nullptr, nullptr) : std::vector<std::complex<double>>();
    const std::complex<double>* lp = lam.empty() ? nullptr : lam.data();
    if ((*info = eigvecs_checked<false>(c, n, p, dT, dZ, lp, S, orient, schurindex, select, nsel, st)) != 0) return *info;
    return *info = eigvecs_dev<false>(c, n, p, dT, dZ, lp, orient, schurindex, select, shifted, dV, maxvec, st);
}

int psd_z_eigvecs_dev(psd_ctx* c, int n, int p, const double* dT, const double* dZ, const double* alpha,
                      const double* beta, const int32_t* ascale, const uint8_t* S, char orient, int schurindex,
                      uint8_t* select, int nsel, int shifted, double* dV, int maxvec, psd_evec_stats* stats, int* info) {
    int dummy;
    if (!info) info = &dummy;
    psd_evec_stats local;
    psd_evec_stats* st = stats ? stats : &local;
    const auto lam = (alpha && beta) ? psd_ev_values(n, nullptr, nullptr, alpha, beta, ascale)
                                     : std::vector<std::complex<double>>();
    const std::complex<double>* lp = lam.empty() ? nullptr : lam.data();
    if ((*info = eigvecs_checked<true>(c, n, p, dT, dZ, lp, S, orient, schurindex, select, nsel, st)) != 0) return *info;
    return *info = eigvecs_dev<true>(c, n, p, dT, dZ, lp, orient, schurindex, select, shifted, dV, maxvec, st);
}

}  // extern "C"
