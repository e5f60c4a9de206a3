// Host driver of psd_z_eigvecs_batch / psd_z_eigvecs_batch_dev (psd_zbevec.h): eigenvectors by back-substitution for nb
// ComplexF64 periodic Schur decompositions of one shape, as psd_z_pschur_batch leaves them.  Included at the end of
// psd_engine.cpp behind psd_bevec_host.inl, whose argument checks, call description, statistics and group plumbing it
// shares (bevec_checked, bevec_call, bevec_finish; batch_group, batch_buffers, batch_upload, batch_download).
//
// A complex form is triangular in every factor, so nothing is read back before the solve: `select` is used as given and
// every selected row is one solve column.  Per group of problems: the tables are built on the host and uploaded once; then
// psd_zbev_solve, psd_zbev_backtransform for V_1, psd_bev_norm, psd_zbev_backtransform for the other factors — four
// launches with shifted and p > 1, three otherwise, whatever nb and n are — and one read-back of the counters.  Orders
// above the context's bev_nmax (PSD_BEV_NMAX) run eigvecs_dev<true> problem by problem on the slices of the batch buffers.

namespace {

// lam [gc][n]: the eigenvalues of the group, converted as psd_z_eigvecs converts them
std::vector<std::complex<double>> zbevec_values(int gc, int n, const double* alpha, const double* beta,
                                                const int32_t* ascale) {
    std::vector<std::complex<double>> lam;
    lam.reserve((size_t)gc * n);
    for (int q = 0; q < gc; ++q) {
        const auto v = psd_ev_values(n, nullptr, nullptr, alpha + 2 * (size_t)q * n, beta + (size_t)q * n,
                                     ascale ? ascale + (size_t)q * n : nullptr);
        lam.insert(lam.end(), v.begin(), v.end());
    }
    return lam;
}

// gc problems resident on the device (dT, dZ [gc][p][n][n] complex, dV [gc][nmat][maxvec][n] complex), their eigenvalues
// and selections; cnt3 [gc][3] receives the counters per problem
int zbevec_group(const bevec_call& k, int gc, const double* dT, const double* dZ, const std::complex<double>* lam,
                 const uint8_t* select, double* dV, int32_t* cnt3, psd_bevec_stats* st) {
    psd_ctx* c = k.c;
    const int n = k.n, p = k.p, nmat = k.shifted ? p : 1;
    const int IS = psd_bev_istride(n), IH = psd_bev_ihead(p), DS = psd_bev_dstride(n);
    std::vector<int> itab((size_t)IH + (size_t)gc * IS, 0), units;
    std::vector<double> dtab((size_t)gc * DS, 0.0);
    for (int j = 0; j < p; ++j) {  // working form (left orientation), as eigvecs_dev
        itab[j] = k.left ? j : p - 1 - j;
        itab[p + j] = k.left ? j : (p - j) % p;
    }
    int nsm = 0;
    for (int q = 0; q < gc; ++q) {
        int* tab = itab.data() + IH + (size_t)q * IS;
        double* dt = dtab.data() + (size_t)q * DS;
        const std::complex<double>* l = lam + (size_t)q * n;
        int ns = 0;
        for (int i = 0; i < n; ++i) {
            tab[i] = 1;  // (every row block is one row; the kernel does not look)
            dt[4 * n + 2 * i] = l[i].real();
            dt[4 * n + 2 * i + 1] = l[i].imag();
            if (!select[(size_t)q * n + i]) continue;
            const std::complex<double> u = psd_ev_root(l[i], p);
            tab[n + ns] = i;
            tab[2 * n + ns] = 1;
            tab[3 * n + ns] = i + 1;
            tab[4 * n + ns] = ns;
            tab[5 * n + ns] = 0;
            tab[6 * n + ns] = i + 1;
            dt[2 * ns] = u.real();
            dt[2 * ns + 1] = u.imag();
            dt[2 * n + 2 * ns] = l[i].real();
            dt[2 * n + 2 * ns + 1] = l[i].imag();
            units.push_back(q);
            units.push_back(ns);
            ++ns;
        }
        tab[7 * n] = ns;
        nsm = ns > nsm ? ns : nsm;
    }
    const int nunits = (int)(units.size() / 2);
    PSD_CHECK(psd_rt_memset(dV, 0, sizeof(double) * 2 * (size_t)gc * nmat * n * k.maxvec, c->stream));
    if (nunits == 0) {
        PSD_CHECK(psd_rt_sync(c->stream));
        return 0;
    }
    itab.insert(itab.end(), units.begin(), units.end());
    const size_t ncnt = 3 * (size_t)gc * n;
    psd_batchbuf bI, bD, bX, bR, bS, bC;
    PSD_CHECK(bI.alloc(sizeof(int) * itab.size()));
    PSD_CHECK(bD.alloc(sizeof(double) * dtab.size()));
    PSD_CHECK(bX.alloc(sizeof(double) * 2 * (size_t)gc * p * n * nsm));
    if (p > 64) PSD_CHECK(bR.alloc(sizeof(double) * 4 * (size_t)nunits * p));
    PSD_CHECK(bS.alloc(sizeof(double) * 2 * (size_t)gc * n));
    PSD_CHECK(bC.alloc(sizeof(int) * ncnt));
    PSD_CHECK(psd_rt_h2d(bI.ptr, itab.data(), sizeof(int) * itab.size(), c->stream));
    PSD_CHECK(psd_rt_h2d(bD.ptr, dtab.data(), sizeof(double) * dtab.size(), c->stream));
    PSD_CHECK(psd_rt_memset(bC.ptr, 0, sizeof(int) * ncnt, c->stream));
    Timer tsolve, tback;
    tsolve.start(c->stream);
    psd_bev_args a;
    a.T = dT; a.itab = (const int*)bI.ptr; a.dtab = bD.d(); a.X = bX.d(); a.R = bR.d(); a.cnt = (int*)bC.ptr;
    a.n = n; a.p = p; a.nsm = nsm; a.nunits = nunits; a.gc = gc; a.six = k.six;
    const int C = 64 / psd_bev_lw(p);
    PSD_LAUNCH(psd_zbev_solve, psd_dim3((nunits + C - 1) / C), 64, PSD_BEV_LDS, c->stream, a);
    st->nlaunch += 1;
    st->ms_solve += tsolve.stop(c->stream);
    // V_l = Z_l x_l: V_1 first, its norms and phases, then the other factors with the column factors
    tback.start(c->stream);
    psd_bev_bt_args g;
    g.Z = dZ; g.X = bX.d(); g.itab = (const int*)bI.ptr; g.S = nullptr; g.cnt = (const int*)bC.ptr; g.V = dV;
    g.n = n; g.p = p; g.nsm = nsm; g.nmat = nmat; g.maxvec = k.maxvec; g.z0 = 0; g.nz = 1;
    const int tiles = (int)(((size_t)nsm * n + PSD_BEV_NT - 1) / PSD_BEV_NT);
    PSD_LAUNCH(psd_zbev_backtransform, psd_dim3(gc, tiles), PSD_BEV_NT, 0, c->stream, g);
    PSD_LAUNCH(psd_bev_norm, psd_dim3((int)(((size_t)gc * n + PSD_BEV_NT - 1) / PSD_BEV_NT)), PSD_BEV_NT, 0, c->stream, dV,
               (const int*)bI.ptr, (const int*)bC.ptr, bS.d(), n, p, gc, nmat, k.maxvec);
    st->nlaunch += 2;
    if (nmat > 1) {
        g.S = bS.d(); g.z0 = 1; g.nz = nmat - 1;
        PSD_LAUNCH(psd_zbev_backtransform, psd_dim3(gc * (nmat - 1), tiles), PSD_BEV_NT, 0, c->stream, g);
        st->nlaunch += 1;
    }
    st->ms_backtransform += tback.stop(c->stream);
    std::vector<int> cnt(ncnt);
    PSD_CHECK(psd_rt_d2h(cnt.data(), bC.ptr, sizeof(int) * ncnt, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    for (int q = 0; q < gc; ++q)
        for (int j = 0; j < n; ++j) {
            const int* e = cnt.data() + 3 * ((size_t)q * n + j);
            cnt3[3 * q] += e[0];
            cnt3[3 * q + 1] += e[1] > 0;
            cnt3[3 * q + 2] += e[2];
        }
    return 0;
}

// above the cap: the single path on the slices of the batch buffers (its V blocks are n x nvec: through a staging block
// into the n x maxvec blocks of the batch)
int zbevec_single(const bevec_call& k, int gc, const double* dT, const double* dZ, const std::complex<double>* lam,
                  const uint8_t* select, const int* nvec, double* dV, int32_t* cnt3, psd_bevec_stats* st) {
    psd_ctx* c = k.c;
    const int n = k.n, p = k.p, nmat = k.shifted ? p : 1;
    const size_t nn2 = 2 * (size_t)n * n, vb = 2 * (size_t)n * k.maxvec;
    PSD_CHECK(psd_rt_memset(dV, 0, sizeof(double) * vb * nmat * gc, c->stream));
    psd_batchbuf stage;
    PSD_CHECK(stage.alloc(sizeof(double) * vb * nmat));
    for (int q = 0; q < gc; ++q) {
        if (nvec[q] == 0) continue;
        std::vector<uint8_t> sel(select + (size_t)q * n, select + (size_t)(q + 1) * n);
        psd_evec_stats es;
        memset(&es, 0, sizeof(es));
        const int rc = eigvecs_dev<true>(c, n, p, dT + (size_t)q * p * nn2, dZ + (size_t)q * p * nn2, lam + (size_t)q * n,
                                         k.orient, k.schurindex, sel.data(), k.shifted, stage.d(), nvec[q], &es);
        if (rc != 0) return rc;
        for (int l = 0; l < nmat; ++l)
            PSD_CHECK(psd_rt_d2d(dV + ((size_t)q * nmat + l) * vb, stage.d() + 2 * (size_t)l * n * nvec[q],
                                 sizeof(double) * 2 * n * nvec[q], c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        cnt3[3 * q] += es.nperturbed;
        cnt3[3 * q + 1] += es.nrescaled;
        cnt3[3 * q + 2] += es.nzero;
        st->ms_solve += es.ms_solve;
        st->ms_backtransform += es.ms_backtransform;
        st->nlaunch += 3 + 2 * ((n + PSD_EV_CH - 1) / PSD_EV_CH);  // (an upper bound: a launch pair per chunk)
    }
    return 0;
}

int zbevec_run(const bevec_call& k, int gc, const double* dT, const double* dZ, const double* alpha, const double* beta,
               const int32_t* ascale, const uint8_t* select, const int* nvec, double* dV, int32_t* cnt3,
               psd_bevec_stats* st) {
    st->ngroups += 1;
    const auto lam = zbevec_values(gc, k.n, alpha, beta, ascale);
    if (k.n > k.c->bev_nmax) return zbevec_single(k, gc, dT, dZ, lam.data(), select, nvec, dV, cnt3, st);
    return zbevec_group(k, gc, dT, dZ, lam.data(), select, dV, cnt3, st);
}

// nvec [nb]: the selected rows of every problem; returns the largest
int zbevec_count(int nb, int n, const uint8_t* select, int* nvec) {
    int mv = 0;
    for (int q = 0; q < nb; ++q) {
        int nv = 0;
        for (int i = 0; i < n; ++i) nv += select[(size_t)q * n + i] != 0;
        nvec[q] = nv;
        mv = nv > mv ? nv : mv;
    }
    return mv;
}

}  // namespace

extern "C" {

int psd_z_eigvecs_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, const double* dZ, const double* alpha,
                            const double* beta, const int32_t* ascale, char orient, int schurindex, const uint8_t* select,
                            int shifted, double* dV, int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats,
                            int* info) {
    int dummy;
    if (!info) info = &dummy;
    psd_bevec_stats local;
    psd_bevec_stats* st = stats ? stats : &local;
    memset(st, 0, sizeof(*st));
    if ((*info = bevec_checked(c, nb, n, p, dT, dZ, alpha, beta, orient, schurindex, select, nvec, st)) != 0 || nb == 0)
        return *info;
    const size_t nn2 = 2 * (size_t)n * n;
    const bool left = orient == 'L';
    const int mv = zbevec_count(nb, n, select, nvec);
    if (!dV) return *info = 0;
    if (mv > maxvec) return *info = -10;
    const int nmat = shifted ? p : 1;
    std::vector<int32_t> cnt3(3 * (size_t)nb, 0);
    if (mv > 0) {
        const bevec_call k{c, n, p, 0, schurindex, shifted, maxvec, left, orient};
        const int g = batch_group(c, nb, sizeof(double) * 2 * (size_t)p * n * mv);
        for (int q0 = 0; q0 < nb; q0 += g) {
            const int gc = nb - q0 < g ? nb - q0 : g;
            *info = zbevec_run(k, gc, dT + (size_t)q0 * p * nn2, dZ + (size_t)q0 * p * nn2, alpha + 2 * (size_t)q0 * n,
                               beta + (size_t)q0 * n, ascale ? ascale + (size_t)q0 * n : nullptr, select + (size_t)q0 * n,
                               nvec + q0, dV + 2 * (size_t)q0 * nmat * n * maxvec, cnt3.data() + 3 * (size_t)q0, st);
            if (*info != 0) return *info;
        }
    } else {
        PSD_CHECK(psd_rt_memset(dV, 0, sizeof(double) * 2 * (size_t)nb * nmat * n * maxvec, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
    }
    bevec_finish(nb, nvec, cnt3.data(), pcnt, st);
    return *info = 0;
}

int psd_z_eigvecs_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, const double* alpha,
                        const double* beta, const int32_t* ascale, char orient, int schurindex, const uint8_t* select,
                        int shifted, double* const* V, int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats,
                        int* info) {
    int dummy;
    if (!info) info = &dummy;
    psd_bevec_stats local;
    psd_bevec_stats* st = stats ? stats : &local;
    memset(st, 0, sizeof(*st));
    if ((*info = bevec_checked(c, nb, n, p, T, Z, alpha, beta, orient, schurindex, select, nvec, st)) != 0 || nb == 0)
        return *info;
    const size_t nn2 = 2 * (size_t)n * n;
    const bool left = orient == 'L';
    const int mv = zbevec_count(nb, n, select, nvec);
    if (!V) return *info = 0;
    if (mv > maxvec) return *info = -10;
    const int nmat = shifted ? p : 1;
    const size_t vb = 2 * (size_t)n * maxvec;
    std::vector<int32_t> cnt3(3 * (size_t)nb, 0);
    if (mv == 0 || maxvec == 0) {
        for (size_t e = 0; e < (size_t)nb * nmat; ++e) memset(V[e], 0, sizeof(double) * vb);
        bevec_finish(nb, nvec, cnt3.data(), pcnt, st);
        return *info = 0;
    }
    const bevec_call k{c, n, p, 0, schurindex, shifted, maxvec, left, orient};
    // (16 bytes per element of T, Z, V and of the X planes)
    int g = batch_group(c, nb, sizeof(double) * (2 * nn2 * p + vb * nmat + 2 * (size_t)p * n * mv));
    psd_batchbuf dbuf[2], dV;
    psd_hostbuf hst, hv;
    if ((*info = batch_buffers(g, nn2 * p, 2, dbuf, hst)) != 0) return *info;
    PSD_CHECK(dV.alloc(sizeof(double) * vb * nmat * g));
    if (!hv.alloc(sizeof(double) * vb * nmat * g)) return *info = PSD_INFO_RUNTIME + 3;
    for (int q0 = 0; q0 < nb; q0 += g) {
        const int gc = nb - q0 < g ? nb - q0 : g;
        if ((*info = batch_upload(c, T, q0, gc, p, nn2, hst.d(), dbuf[0].d())) != 0) return *info;
        if ((*info = batch_upload(c, Z, q0, gc, p, nn2, hst.d(), dbuf[1].d())) != 0) return *info;
        *info = zbevec_run(k, gc, dbuf[0].d(), dbuf[1].d(), alpha + 2 * (size_t)q0 * n, beta + (size_t)q0 * n,
                           ascale ? ascale + (size_t)q0 * n : nullptr, select + (size_t)q0 * n, nvec + q0, dV.d(),
                           cnt3.data() + 3 * (size_t)q0, st);
        if (*info != 0) return *info;
        if ((*info = batch_download(c, V, q0, gc, nmat, vb, hv.d(), dV.d())) != 0) return *info;
    }
    bevec_finish(nb, nvec, cnt3.data(), pcnt, st);
    return *info = 0;
}

}  // extern "C"
