// Host driver of psd_z_eigvecs_batch / psd_z_eigvecs_batch_dev (psd_zbevec.h): eigenvectors by back-substitution for nb
// ComplexF64 periodic Schur decompositions of one shape, as psd_z_pschur_batch leaves them.  Included at the end of
// psd_engine.cpp behind psd_bevec_host.inl, whose argument checks, call description, statistics and group plumbing it
// shares (bevec_checked, bevec_call, bevec_launch, bevec_single, bevec_entry_dev, bevec_entry_host).  zbevec_head is the
// head of the signed entries (psd_zgbevec_host.inl) too.
//
// A complex form is triangular in every factor, so nothing is read back before the solve: `select` is used as given and
// every selected row is one solve column.  Per group of problems: the tables are built on the host and uploaded once; then
// psd_zbev_solve, psd_zbev_backtransform for V_1, psd_bev_norm, psd_zbev_backtransform for the other factors — four
// launches with shifted and p > 1, three otherwise, whatever nb and n are — and one read-back of the counters.  Orders
// above the context's bev_nmax (PSD_BEV_NMAX) run eigvecs_dev<true> problem by problem on the slices of the batch buffers.
//
// psd_z_leigvecs_batch / psd_z_leigvecs_batch_dev (the LEFT eigenvectors, psd_lbevec.h): the same bodies with lside set,
// through lbevec_run of psd_bevec_host.inl; zbevec_run flips the eigenvalues and the selection of its group.

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
                const std::complex<double> u = bevec_root(k, l[i]);
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

// the problems [q0, q0 + gc) of a call: their blocks on the device and counters; alpha, beta, ascale, select, nvec: the
// rows of the whole call
int zbevec_run(const bevec_call& k, int q0, int gc, const double* dT, const double* dZ, const double* alpha,
               const double* beta, const int32_t* ascale, const uint8_t* select, const int* nvec, double* dV, int32_t* cnt3,
               psd_bevec_stats* st) {
    st->ngroups += 1;
    const size_t r0 = (size_t)q0 * k.n;
    auto lam = zbevec_values(gc, k.n, alpha + 2 * r0, beta + r0, ascale ? ascale + r0 : nullptr);
    select += r0;
    nvec += q0;
    std::vector<uint8_t> fsel;
    if (k.lconj) {  // a left call: the rows of the flipped form (psd_lbevec.h), eigenvalues conjugated
        fsel.resize((size_t)gc * k.n);
        for (int q = 0; q < gc; ++q) {
            std::reverse(lam.begin() + (size_t)q * k.n, lam.begin() + (size_t)(q + 1) * k.n);
            for (int i = 0; i < k.n; ++i) fsel[(size_t)q * k.n + k.n - 1 - i] = select[(size_t)q * k.n + i];
        }
        for (auto& l : lam) l = std::conj(l);
        select = fsel.data();
    }
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

// What the four complex entries start with: the codes, the counts, the size query (V null).  alpha, beta: the eigenvalue
// arguments of the unsigned entries (-6).  Returns true when the call is over (*info set).
bool zbevec_head(psd_ctx* c, int nb, int n, int p, const void* T, const void* Z, const double* alpha, const double* beta,
                 char orient, int schurindex, const uint8_t* select, const void* V, int maxvec, int* nvec,
                 psd_bevec_stats* st, int& mv, int* info) {
    if ((*info = bevec_checked(c, nb, n, p, T, Z, alpha, beta, orient, schurindex, select, nvec, st)) != 0 || nb == 0)
        return true;
    mv = zbevec_count(nb, n, select, nvec);
    if (!V) return true;
    if (mv > maxvec) {
        *info = -10;
        return true;
    }
    return false;
}

// The two complex entries behind their names.  lside: the left vectors (psd_lbevec.h): the solve runs on the flipped
// form, which has the opposite orientation and the same schurindex
int zbevec_dev(bool lside, psd_ctx* c, int nb, int n, int p, const double* dT, const double* dZ, const double* alpha,
               const double* beta, const int32_t* ascale, char orient, int schurindex, const uint8_t* select, int shifted,
               double* dV, int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info) {
    batch_call<psd_bevec_stats> entry(info, stats);
    psd_bevec_stats* st = entry.s;
    int mv = 0;
    if (zbevec_head(c, nb, n, p, dT, dZ, alpha, beta, orient, schurindex, select, dV, maxvec, nvec, st, mv, info)) return *info;
    const bool left = (orient == 'L') != lside;
    const bevec_call k{c, n, p, 0, schurindex, shifted, maxvec, left, left ? 'L' : 'R', lside};
    return *info = bevec_entry_dev(k, nb, 2 * (size_t)n * n, dT, dZ, dV, mv, nvec, pcnt, st,
                                   [&](int q0, int gc, const double* dTg, const double* dZg, double* dVg, int32_t* cnt3) {
        auto run = [&](const double* gT, const double* gZ) {
            return zbevec_run(k, q0, gc, gT, gZ, alpha, beta, ascale, select, nvec, dVg, cnt3, st);
        };
        return lside ? lbevec_run<true>(k, gc, dTg, dZg, dVg, nvec + q0, st, run) : run(dTg, dZg);
    });
}

int zbevec_host(bool lside, psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, const double* alpha,
                const double* beta, const int32_t* ascale, char orient, int schurindex, const uint8_t* select, int shifted,
                double* const* V, int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info) {
    batch_call<psd_bevec_stats> entry(info, stats);
    psd_bevec_stats* st = entry.s;
    int mv = 0;
    if (zbevec_head(c, nb, n, p, T, Z, alpha, beta, orient, schurindex, select, V, maxvec, nvec, st, mv, info)) return *info;
    const bool left = (orient == 'L') != lside;
    const bevec_call k{c, n, p, 0, schurindex, shifted, maxvec, left, left ? 'L' : 'R', lside};
    return *info = bevec_entry_host(k, nb, 2 * (size_t)n * n, T, Z, V, mv, nvec, pcnt, st,
                                    [&](int q0, int gc, const double* dTg, const double* dZg, double* dVg, int32_t* cnt3) {
        auto run = [&](const double* gT, const double* gZ) {
            return zbevec_run(k, q0, gc, gT, gZ, alpha, beta, ascale, select, nvec, dVg, cnt3, st);
        };
        return lside ? lbevec_run<true>(k, gc, dTg, dZg, dVg, nvec + q0, st, run) : run(dTg, dZg);
    });
}

}  // namespace

extern "C" {

int psd_z_eigvecs_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, const double* dZ, const double* alpha,
                            const double* beta, const int32_t* ascale, char orient, int schurindex, const uint8_t* select,
                            int shifted, double* dV, int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats,
                            int* info) {
    return zbevec_dev(false, c, nb, n, p, dT, dZ, alpha, beta, ascale, orient, schurindex, select, shifted, dV, maxvec, nvec,
                      pcnt, stats, info);
}

int psd_z_eigvecs_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, const double* alpha,
                        const double* beta, const int32_t* ascale, char orient, int schurindex, const uint8_t* select,
                        int shifted, double* const* V, int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats,
                        int* info) {
    return zbevec_host(false, c, nb, n, p, T, Z, alpha, beta, ascale, orient, schurindex, select, shifted, V, maxvec, nvec,
                       pcnt, stats, info);
}

int psd_z_leigvecs_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, const double* dZ, const double* alpha,
                             const double* beta, const int32_t* ascale, char orient, int schurindex, const uint8_t* select,
                             int shifted, double* dV, int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats,
                             int* info) {
    return zbevec_dev(true, c, nb, n, p, dT, dZ, alpha, beta, ascale, orient, schurindex, select, shifted, dV, maxvec, nvec,
                      pcnt, stats, info);
}

int psd_z_leigvecs_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, const double* alpha,
                         const double* beta, const int32_t* ascale, char orient, int schurindex, const uint8_t* select,
                         int shifted, double* const* V, int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats,
                         int* info) {
    return zbevec_host(true, c, nb, n, p, T, Z, alpha, beta, ascale, orient, schurindex, select, shifted, V, maxvec, nvec,
                       pcnt, stats, info);
}

}  // extern "C"
