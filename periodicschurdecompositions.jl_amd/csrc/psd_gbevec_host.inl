// Host driver of psd_d_geigvecs_batch / psd_d_geigvecs_batch_dev (psd_gbevec.h): geigvecs — eigenvectors by homogeneous
// back-substitution, zero and infinite eigenvalues included — for nb signed Float64 periodic Schur decompositions of one
// shape and one signature, as psd_d_gpschur_batch / psd_d_gordschur_batch leave them.  Included at the end of
// psd_engine.cpp behind psd_zgbevec_host.inl, whose pieces it shares: bevec_checked, bevec_blocks, bevec_call, bevec_itab,
// bevec_launch (with the senses of the working factors), bevec_single_loop, bevec_entry_dev, bevec_entry_host,
// zgbevec_sgn; the scalars of a solve column are gev_scalars of the single driver (psd_gevec_host.inl).
//
// Before the solve the host needs T_l(i, i), T_l(i + 1, i) and T_l(i, i + 1) of every factor of every problem: they
// define the 2x2 row blocks (the sub-diagonal of the quasi-triangular factor), the completion of `select` to whole pairs,
// the scalars a_l of every solve column (uploaded with the group's tables) and the count of zero scalars.  The host entry
// reads them from the caller's matrices; the device entry with ONE psd_gev_gather launch (its p the nb * p factors of
// the batch) and one read-back for the whole call.  Launches of a call up to the context's bev_nmax (PSD_BEV_NMAX), per
// group of problems, whatever nb and n are:
//   psd_gbev_solve, psd_bev_backtransform for V_1, psd_bev_norm, psd_bev_backtransform for the other factors:
//   four with shifted and p > 1, three otherwise;
//   the device entry: the gather, one more for the whole call;
//   none when nothing is selected.
// One read-back of the counters per group.  Orders above bev_nmax run geigvecs_dev<false> problem by problem on the slices
// of the batch buffers.

namespace {

struct gbevec_call {
    bevec_call k;
    const uint8_t* S;  // the user's signature (the single path takes it as given)
    std::vector<int> sgn;
};

// what the gathered entries give: the row blocks, the scalars of every solve column in working order
// ([nb][n][p] complex, the tables' dtab) and the columns with a zero scalar per problem
struct gbevec_plan {
    std::vector<int> bsz, nz;
    std::vector<double> ac;
};

int gbevec_checked(psd_ctx* c, int nb, int n, int p, const void* T, const void* Z, char orient, int schurindex,
                   const uint8_t* select, int* nvec, psd_bevec_stats* st) {
    const double none = 0.0;  // (there are no eigenvalue arguments: -6 is not used)
    return bevec_checked(c, nb, n, p, T, Z, &none, &none, orient, schurindex, select, nvec, st);
}

// gd: [nb * p][n][3], T_m(i, i), T_m(i + 1, i), T_m(i, i + 1) of factor m of the batch (psd_gev_gather's layout), or
// nullptr when nothing is selected.  Completes select, fills nvec and, with V, the plan and a ([nb][maxvec][p] complex or
// nullptr).  Returns true when the call is over (*info set); mv: the most columns of a problem.
bool gbevec_head(const gbevec_call& g, int nb, const double* gd, uint8_t* select, const void* V, double* a, int* nvec,
                 gbevec_plan& pl, int& mv, int* info) {
    using cd = std::complex<double>;
    const bevec_call& k = g.k;
    const int n = k.n, p = k.p, si = k.schurindex - 1;
    auto at = [&](int q, int l, int i, int w) { return gd[(((size_t)q * p + l) * n + i) * 3 + w]; };
    std::vector<double> sub;
    if (gd) {
        sub.resize((size_t)nb * n);
        for (int q = 0; q < nb; ++q)
            for (int i = 0; i < n; ++i) sub[(size_t)q * n + i] = at(q, si, i, 1);
    }
    bevec_blocks(nb, n, gd ? sub.data() : nullptr, select, pl.bsz, nvec);
    mv = 0;
    for (int q = 0; q < nb; ++q) mv = nvec[q] > mv ? nvec[q] : mv;
    *info = 0;
    if (!V) return true;
    if (mv > k.maxvec) {
        *info = -10;
        return true;
    }
    if (a) memset(a, 0, sizeof(double) * 2 * (size_t)nb * k.maxvec * p);
    pl.nz.assign(nb, 0);
    pl.ac.assign(mv > 0 ? 2 * (size_t)nb * n * p : 0, 0.0);
    if (mv == 0) return false;
    std::vector<int> wmap(p);
    for (int j = 0; j < p; ++j) wmap[j] = k.left ? j : p - 1 - j;
    std::vector<cd> au(p);
    for (int q = 0; q < nb; ++q) {
        const int* b = pl.bsz.data() + (size_t)q * n;
        int ns = 0, col = 0;
        for (int i = 0; i < n; i += b[i]) {
            if (!select[(size_t)q * n + i]) continue;
            pl.nz[q] += gev_scalars(p, si, g.S, wmap.data(), g.sgn.data(), i, b[i],
                                    [&](int l, int r, int w) { return cd(at(q, l, r, w), 0.0); }, au.data());
            for (int w = 0; w < p; ++w) {
                double* o = pl.ac.data() + 2 * (((size_t)q * n + ns) * p + w);
                o[0] = au[wmap[w]].real();
                o[1] = au[wmap[w]].imag();
            }
            if (a)
                for (int l = 0; l < p; ++l) {  // (a pair: the partner's scalars are the conjugates)
                    double* o = a + 2 * (((size_t)q * k.maxvec + col) * p + l);
                    o[0] = au[l].real();
                    o[1] = au[l].imag();
                    if (b[i] == 2) {
                        o[2 * p] = au[l].real();
                        o[2 * p + 1] = -au[l].imag();
                    }
                }
            ++ns;
            col += b[i];
        }
    }
    return false;
}

// the problems [q0, q0 + gc) of a call resident on the device (dT, dZ [gc][p][n][n], dV [gc][nmat][maxvec][n] complex);
// hT: the host matrices of the call (nb * p pointers) or nullptr; select, nvec: the rows of the whole call; cnt3 [gc][3]
// receives the counters per problem
int gbevec_run(const gbevec_call& g, const gbevec_plan& pl, int q0, int gc, const double* dT, const double* dZ,
               double* const* hT, const uint8_t* select, const int* nvec, double* dV, int32_t* cnt3, psd_bevec_stats* st) {
    const bevec_call& k = g.k;
    const int n = k.n, p = k.p;
    st->ngroups += 1;
    select += (size_t)q0 * n;
    nvec += q0;
    if (n > k.c->bev_nmax) {
        const size_t bd = (size_t)n * n;
        return bevec_single_loop(k, gc, select, nvec, dV, cnt3, st, [&](int q, uint8_t* sel, double* dVq, psd_evec_stats* es) {
            if (!hT) st->nlaunch += 1;  // (the entries of the problem again: psd_gev_gather)
            return geigvecs_dev<false>(k.c, n, p, dT + (size_t)q * p * bd, hT ? hT + (size_t)(q0 + q) * p : nullptr,
                                       dZ + (size_t)q * p * bd, g.S, k.orient, k.schurindex, sel, k.shifted, dVq, nvec[q],
                                       nullptr, es);
        });
    }
    std::vector<int> itab, units;
    const int nsm = bevec_itab(k, gc, select, pl.bsz.data() + (size_t)q0 * n, itab, units, [](int, int, int) {});
    const size_t per = 2 * (size_t)n * p;
    const std::vector<double> dtab(pl.ac.begin() + (size_t)q0 * per, pl.ac.begin() + (size_t)(q0 + gc) * per);
    if (const int rc = bevec_launch<false>(k, gc, dT, dZ, itab, dtab, units, nsm, dV, cnt3, st, g.sgn.data())) return rc;
    for (int q = 0; q < gc; ++q) cnt3[3 * q + 2] += pl.nz[q0 + q];
    return 0;
}

}  // namespace

extern "C" {

int psd_d_geigvecs_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, const double* dZ, const uint8_t* S,
                             char orient, int schurindex, uint8_t* select, int shifted, double* dV, int maxvec,
                             double* a, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info) {
    batch_call<psd_bevec_stats> entry(info, stats);
    psd_bevec_stats* st = entry.s;
    if ((*info = gbevec_checked(c, nb, n, p, dT, dZ, orient, schurindex, select, nvec, st)) != 0 || nb == 0) return *info;
    const size_t tot = (size_t)nb * p * n;
    bool any = false;
    for (size_t e = 0; e < (size_t)nb * n && !any; ++e) any = select[e] != 0;
    std::vector<double> gd;
    if (any) {  // one kernel and one read-back for the row blocks and the scalars of the whole batch
        psd_batchbuf bg;
        PSD_CHECK(bg.alloc(sizeof(double) * 3 * tot));
        PSD_LAUNCH(psd_gev_gather, psd_dim3((int)((tot + 63) / 64)), 64, 0, c->stream, dT, n, nb * p, 1, bg.d());
        st->nlaunch += 1;
        gd.resize(3 * tot);
        PSD_CHECK(psd_rt_d2h(gd.data(), bg.d(), sizeof(double) * 3 * tot, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
    }
    const bool left = orient == 'L';
    const gbevec_call g{{c, n, p, left ? schurindex - 1 : p - schurindex, schurindex, shifted, maxvec, left, orient}, S,
                        zgbevec_sgn(p, S, left)};
    gbevec_plan pl;
    int mv = 0;
    if (gbevec_head(g, nb, any ? gd.data() : nullptr, select, dV, a, nvec, pl, mv, info)) return *info;
    return *info = bevec_entry_dev(g.k, nb, (size_t)n * n, dT, dZ, dV, mv, nvec, pcnt, st,
                                   [&](int q0, int gc, const double* dTg, const double* dZg, double* dVg, int32_t* cnt3) {
        return gbevec_run(g, pl, q0, gc, dTg, dZg, nullptr, select, nvec, dVg, cnt3, st);
    });
}

int psd_d_geigvecs_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, const uint8_t* S,
                         char orient, int schurindex, uint8_t* select, int shifted, double* const* V, int maxvec,
                         double* a, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info) {
    batch_call<psd_bevec_stats> entry(info, stats);
    psd_bevec_stats* st = entry.s;
    if ((*info = gbevec_checked(c, nb, n, p, T, Z, orient, schurindex, select, nvec, st)) != 0 || nb == 0) return *info;
    std::vector<double> gd(3 * (size_t)nb * p * n, 0.0);  // (the factors are on the host: no kernel)
    for (size_t m = 0; m < (size_t)nb * p; ++m)
        for (int i = 0; i < n; ++i) {
            double* o = gd.data() + (m * n + i) * 3;
            o[0] = T[m][(size_t)i * n + i];
            if (i + 1 < n) {
                o[1] = T[m][(size_t)i * n + i + 1];
                o[2] = T[m][(size_t)(i + 1) * n + i];
            }
        }
    const bool left = orient == 'L';
    const gbevec_call g{{c, n, p, left ? schurindex - 1 : p - schurindex, schurindex, shifted, maxvec, left, orient}, S,
                        zgbevec_sgn(p, S, left)};
    gbevec_plan pl;
    int mv = 0;
    if (gbevec_head(g, nb, gd.data(), select, V, a, nvec, pl, mv, info)) return *info;
    return *info = bevec_entry_host(g.k, nb, (size_t)n * n, T, Z, V, mv, nvec, pcnt, st,
                                    [&](int q0, int gc, const double* dTg, const double* dZg, double* dVg, int32_t* cnt3) {
        return gbevec_run(g, pl, q0, gc, dTg, dZg, T, select, nvec, dVg, cnt3, st);
    });
}

}  // extern "C"
