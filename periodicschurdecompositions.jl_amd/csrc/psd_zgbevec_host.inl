// Host driver of psd_z_geigvecs_batch / psd_z_geigvecs_batch_dev (psd_zgbevec.h): geigvecs — eigenvectors by homogeneous
// back-substitution, zero and infinite eigenvalues included — for nb signed ComplexF64 periodic Schur decompositions of
// one shape and one signature, as psd_z_gpschur_batch / psd_z_gordschur_batch leave them.  Included at the end of
// psd_engine.cpp behind psd_zbevec_host.inl, whose pieces it shares: bevec_checked, bevec_call, bevec_launch (with the
// senses of the working factors), bevec_single_loop, bevec_entry_dev, bevec_entry_host, zbevec_head, zbevec_tables.
//
// Nothing is read back before the solve: `select` is used as given, every selected row is one solve column, and the
// kernel takes the scalars a_l from the diagonals of the factors.  Launches of a call up to the context's bev_nmax
// (PSD_BEV_NMAX), per group of problems, whatever nb and n are:
//   psd_zgbev_solve, psd_zbev_backtransform for V_1, psd_bev_norm, psd_zbev_backtransform for the other factors:
//   four with shifted and p > 1, three otherwise;
//   the device entry with a != NULL: one more for the whole call, psd_zgbev_diag (the host entry reads the diagonals from
//   the caller's matrices);
//   none when nothing is selected.
// One read-back of the counters per group, one of the diagonals per call.  Orders above bev_nmax run geigvecs_dev<true>
// problem by problem on the slices of the batch buffers.

namespace {

// the senses of the working factors (left orientation), as geigvecs_dev maps the user's signature
std::vector<int> zgbevec_sgn(int p, const uint8_t* S, bool left) {
    std::vector<int> sgn(p);
    for (int j = 0; j < p; ++j) sgn[j] = S ? (S[left ? j : p - 1 - j] ? 1 : 0) : 1;
    return sgn;
}

struct zgbevec_call {
    bevec_call k;
    const uint8_t* S;  // the user's signature (the single path takes it as given)
    std::vector<int> sgn;
};

// gc problems resident on the device (dT, dZ [gc][p][n][n] complex, dV [gc][nmat][maxvec][n] complex) and their
// selections; hT: their host matrices (gc * p pointers) or nullptr; cnt3 [gc][3] receives the counters per problem
int zgbevec_run(const zgbevec_call& g, int gc, const double* dT, const double* dZ, double* const* hT,
                const uint8_t* select, const int* nvec, double* dV, int32_t* cnt3, psd_bevec_stats* st) {
    const bevec_call& k = g.k;
    const int n = k.n, p = k.p;
    st->ngroups += 1;
    if (n > k.c->bev_nmax) {
        const size_t bd = 2 * (size_t)n * n;
        return bevec_single_loop(k, gc, select, nvec, dV, cnt3, st, [&](int q, uint8_t* sel, double* dVq, psd_evec_stats* es) {
            if (!hT) st->nlaunch += 1;  // (the diagonals of the problem: psd_gev_gather)
            return geigvecs_dev<true>(k.c, n, p, dT + (size_t)q * p * bd, hT ? hT + (size_t)q * p : nullptr,
                                      dZ + (size_t)q * p * bd, g.S, k.orient, k.schurindex, sel, k.shifted, dVq, nvec[q],
                                      nullptr, es);
        });
    }
    std::vector<int> itab, units;
    std::vector<double> dtab;
    const int nsm = zbevec_tables(k, gc, nullptr, select, itab, dtab, units);
    return bevec_launch<true>(k, gc, dT, dZ, itab, dtab, units, nsm, dV, cnt3, st, g.sgn.data());
}

// a [nb][maxvec][p] complex from the diagonals of the factors: diag(q, l, i) = T_l(i, i) of problem q (re, im).  The
// columns at and beyond the selected rows of a problem stay zero.
template <class Diag>
void zgbevec_scalars(int nb, int n, int p, int maxvec, const uint8_t* select, Diag diag, double* a) {
    memset(a, 0, sizeof(double) * 2 * (size_t)nb * maxvec * p);
    for (int q = 0; q < nb; ++q) {
        int col = 0;
        for (int i = 0; i < n; ++i) {
            if (!select[(size_t)q * n + i]) continue;
            for (int l = 0; l < p; ++l) {
                const double* d = diag(q, l, i);
                double* o = a + 2 * (((size_t)q * maxvec + col) * p + l);
                o[0] = d[0];
                o[1] = d[1];
            }
            ++col;
        }
    }
}

// the same from the factors on the device: one gather (psd_zgbev_diag) and one read-back for the whole batch; no launch
// when nothing is selected (mv == 0)
int zgbevec_scalars_dev(psd_ctx* c, int nb, int n, int p, const double* dT, int maxvec, int mv, const uint8_t* select,
                        double* a, psd_bevec_stats* st) {
    const size_t tot = (size_t)nb * p * n;
    std::vector<double> diag(mv > 0 ? 2 * tot : 0);
    if (mv > 0) {
        psd_batchbuf bdiag;
        PSD_CHECK(bdiag.alloc(sizeof(double) * 2 * tot));
        PSD_LAUNCH(psd_zgbev_diag, psd_dim3((int)((tot + PSD_BEV_NT - 1) / PSD_BEV_NT)), PSD_BEV_NT, 0, c->stream, dT, n,
                   (size_t)nb * p, bdiag.d());
        st->nlaunch += 1;
        PSD_CHECK(psd_rt_d2h(diag.data(), bdiag.d(), sizeof(double) * 2 * tot, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
    }
    zgbevec_scalars(nb, n, p, maxvec, select, [&](int q, int l, int i) { return diag.data() + 2 * (((size_t)q * p + l) * n + i); },
                    a);
    return 0;
}

}  // namespace

extern "C" {

int psd_z_geigvecs_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, const double* dZ, const uint8_t* S,
                             char orient, int schurindex, const uint8_t* select, int shifted, double* dV, int maxvec,
                             double* a, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info) {
    batch_call<psd_bevec_stats> entry(info, stats);
    psd_bevec_stats* st = entry.s;
    const double none = 0.0;  // (there are no eigenvalue arguments: -6 is not used)
    int mv = 0;
    if (zbevec_head(c, nb, n, p, dT, dZ, &none, &none, orient, schurindex, select, dV, maxvec, nvec, st, mv, info)) return *info;
    if (a && (*info = zgbevec_scalars_dev(c, nb, n, p, dT, maxvec, mv, select, a, st)) != 0) return *info;
    const bool left = orient == 'L';
    const zgbevec_call g{{c, n, p, 0, schurindex, shifted, maxvec, left, orient}, S, zgbevec_sgn(p, S, left)};
    return *info = bevec_entry_dev(g.k, nb, 2 * (size_t)n * n, dT, dZ, dV, mv, nvec, pcnt, st,
                                   [&](int q0, int gc, const double* dTg, const double* dZg, double* dVg, int32_t* cnt3) {
        return zgbevec_run(g, gc, dTg, dZg, nullptr, select + (size_t)q0 * n, nvec + q0, dVg, cnt3, st);
    });
}

int psd_z_geigvecs_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, const uint8_t* S,
                         char orient, int schurindex, const uint8_t* select, int shifted, double* const* V, int maxvec,
                         double* a, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info) {
    batch_call<psd_bevec_stats> entry(info, stats);
    psd_bevec_stats* st = entry.s;
    const double none = 0.0;
    int mv = 0;
    if (zbevec_head(c, nb, n, p, T, Z, &none, &none, orient, schurindex, select, V, maxvec, nvec, st, mv, info)) return *info;
    if (a)  // (the factors are on the host: no kernel)
        zgbevec_scalars(nb, n, p, maxvec, select,
                        [&](int q, int l, int i) { return T[(size_t)q * p + l] + 2 * ((size_t)i * n + i); }, a);
    const bool left = orient == 'L';
    const zgbevec_call g{{c, n, p, 0, schurindex, shifted, maxvec, left, orient}, S, zgbevec_sgn(p, S, left)};
    return *info = bevec_entry_host(g.k, nb, 2 * (size_t)n * n, T, Z, V, mv, nvec, pcnt, st,
                                    [&](int q0, int gc, const double* dTg, const double* dZg, double* dVg, int32_t* cnt3) {
        return zgbevec_run(g, gc, dTg, dZg, T + (size_t)q0 * p, select + (size_t)q0 * n, nvec + q0, dVg, cnt3, st);
    });
}

}  // extern "C"
