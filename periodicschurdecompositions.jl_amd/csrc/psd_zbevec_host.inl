// Host driver of psd_z_eigvecs_batch / psd_z_eigvecs_batch_dev (psd_zbevec.h): eigenvectors by back-substitution for nb
// ComplexF64 periodic Schur decompositions of one shape, as psd_z_pschur_batch leaves them.  Included at the end of
// psd_engine.cpp behind psd_bevec_host.inl, whose argument checks, call description, statistics and group plumbing it
// shares (bevec_checked, bevec_call, bevec_launch, bevec_single, bevec_finish; batch_staged).
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

// The tables of gc complex problems from their selections: the integers (itab), the units, and with lam [gc][n] the doubles
// (dtab: roots and eigenvalues); the signed path (psd_zgbevec_host.inl) has no eigenvalues, passes lam = nullptr and leaves
// dtab empty.  Returns the largest number of solve columns of a problem.
int zbevec_tables(const bevec_call& k, int gc, const std::complex<double>* lam, const uint8_t* select,
                  std::vector<int>& itab, std::vector<double>& dtab, std::vector<int>& units) {
    const int n = k.n, p = k.p;
    const int IS = psd_bev_istride(n), IH = psd_bev_ihead(p), DS = psd_bev_dstride(n);
    itab.assign((size_t)IH + (size_t)gc * IS, 0);
    dtab.assign(lam ? (size_t)gc * DS : 0, 0.0);
    units.clear();
    for (int j = 0; j < p; ++j) {  // working form (left orientation), as eigvecs_dev
        itab[j] = k.left ? j : p - 1 - j;
        itab[p + j] = k.left ? j : (p - j) % p;
    }
    int nsm = 0;
    for (int q = 0; q < gc; ++q) {
        int* tab = itab.data() + IH + (size_t)q * IS;
        double* dt = lam ? dtab.data() + (size_t)q * DS : nullptr;
        const std::complex<double>* l = lam ? lam + (size_t)q * n : nullptr;
        int ns = 0;
        for (int i = 0; i < n; ++i) {
            tab[i] = 1;  // (every row block is one row; the kernel does not look)
            if (l) {
                dt[4 * n + 2 * i] = l[i].real();
                dt[4 * n + 2 * i + 1] = l[i].imag();
            }
            if (!select[(size_t)q * n + i]) continue;
            tab[n + ns] = i;
            tab[2 * n + ns] = 1;
            tab[3 * n + ns] = i + 1;
            tab[4 * n + ns] = ns;
            tab[5 * n + ns] = 0;
            tab[6 * n + ns] = i + 1;
            if (l) {
                const std::complex<double> u = psd_ev_root(l[i], p);
                dt[2 * ns] = u.real();
                dt[2 * ns + 1] = u.imag();
                dt[2 * n + 2 * ns] = l[i].real();
                dt[2 * n + 2 * ns + 1] = l[i].imag();
            }
            units.push_back(q);
            units.push_back(ns);
            ++ns;
        }
        tab[7 * n] = ns;
        nsm = ns > nsm ? ns : nsm;
    }
    return nsm;
}

// gc problems resident on the device (dT, dZ [gc][p][n][n] complex, dV [gc][nmat][maxvec][n] complex), their eigenvalues
// and selections; cnt3 [gc][3] receives the counters per problem
int zbevec_group(const bevec_call& k, int gc, const double* dT, const double* dZ, const std::complex<double>* lam,
                 const uint8_t* select, double* dV, int32_t* cnt3, psd_bevec_stats* st) {
    std::vector<int> itab, units;
    std::vector<double> dtab;
    const int nsm = zbevec_tables(k, gc, lam, select, itab, dtab, units);
    return bevec_launch<true>(k, gc, dT, dZ, itab, dtab, units, nsm, dV, cnt3, st);
}

int zbevec_run(const bevec_call& k, int gc, const double* dT, const double* dZ, const double* alpha, const double* beta,
               const int32_t* ascale, const uint8_t* select, const int* nvec, double* dV, int32_t* cnt3,
               psd_bevec_stats* st) {
    st->ngroups += 1;
    const auto lam = zbevec_values(gc, k.n, alpha, beta, ascale);
    if (k.n > k.c->bev_nmax) return bevec_single<true>(k, gc, dT, dZ, lam.data(), select, nvec, dV, cnt3, st);
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
    batch_call<psd_bevec_stats> entry(info, stats);
    psd_bevec_stats* st = entry.s;
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
        *info = bevec_dev_groups(c, nb, sizeof(double) * 2 * (size_t)p * n * mv, [&](int q0, int gc) {
            return zbevec_run(k, gc, dT + (size_t)q0 * p * nn2, dZ + (size_t)q0 * p * nn2, alpha + 2 * (size_t)q0 * n,
                              beta + (size_t)q0 * n, ascale ? ascale + (size_t)q0 * n : nullptr, select + (size_t)q0 * n,
                              nvec + q0, dV + 2 * (size_t)q0 * nmat * n * maxvec, cnt3.data() + 3 * (size_t)q0, st);
        });
        if (*info != 0) return *info;
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
    batch_call<psd_bevec_stats> entry(info, stats);
    psd_bevec_stats* st = entry.s;
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
    const batch_list L[] = {{T, p, nn2, BATCH_IN}, {Z, p, nn2, BATCH_IN}, {V, nmat, vb, BATCH_OUT}};
    auto body = [&](int q0, int gc, double* const* d) {
        return zbevec_run(k, gc, d[0], d[1], alpha + 2 * (size_t)q0 * n, beta + (size_t)q0 * n,
                          ascale ? ascale + (size_t)q0 * n : nullptr, select + (size_t)q0 * n, nvec + q0, d[2],
                          cnt3.data() + 3 * (size_t)q0, st);
    };
    const size_t per = sizeof(double) * (2 * nn2 * p + vb * nmat + 2 * (size_t)p * n * mv);
    *info = batch_staged(c, nb, per, L, nullptr, batch_no_extra, body);
    if (*info != 0) return *info;
    bevec_finish(nb, nvec, cnt3.data(), pcnt, st);
    return *info = 0;
}

}  // extern "C"
