// Host driver of psd_?_checkpsd_batch / psd_?_checkpsd_batch_dev (psd_bcheck.h): checkpsd(P, As; thresh, strict) for nb
// decompositions of one shape, one signature, one orientation.  Included at the end of psd_engine.cpp behind
// psd_check_host.inl (checkpsd_dev, checkpsd_verdict), psd_batch_host.inl (psd_batchbuf, batch_group, batch_staged) and
// psd_bevec_host.inl (bevec_dev_groups).
//
// Per group of problems: ONE launch of psd_bck_check, a workgroup per (problem, factor), and one read-back of four
// numbers per factor; the verdicts are formed on the host by the function the single path uses.  Orders above
// PSD_BCK_NMAX run checkpsd_dev problem by problem on the slices of the batch buffers.  The factors are only read.

namespace {

struct bcheck_call {
    psd_ctx* c;
    int n, p, schurindex, strict;
    char orient;
    double thresh;
    const uint8_t* S;
    const int* dab;  // device [p][2]: the factors a, b of every residual (diagnostics.jl:249-253)
};

// gc problems resident on the device (dT, dZ, dA [gc][p][n][n] in user order); err, orth, tri [gc][p] and ok [gc] are the
// rows of these problems (orth, tri, ok may be null)
template <bool CPLX>
int bcheck_run(const bcheck_call& k, int gc, const double* dT, const double* dZ, const double* dA, double* err, double* orth,
               double* tri, int32_t* ok, psd_bcheck_stats* st) {
    psd_ctx* c = k.c;
    const int n = k.n, p = k.p;
    st->ngroups += 1;
    Timer tk;
    tk.start(c->stream);
    if (n > c->bck_nmax) {  // the single path on the slices of the batch
        const size_t pb = (size_t)(CPLX ? 2 : 1) * n * n * p;
        for (int q = 0; q < gc; ++q) {
            int good = 0;
            const int rc = checkpsd_dev<CPLX>(c, n, p, dT + q * pb, dZ + q * pb, dA + q * pb, k.S, k.orient, k.schurindex,
                                              nullptr, k.thresh, k.strict, err + (size_t)q * p, orth ? orth + (size_t)q * p : nullptr,
                                              tri ? tri + (size_t)q * p : nullptr, &good);
            if (rc != 0) return rc;
            if (ok) ok[q] = good;
            st->nfail += good ? 0 : 1;
            st->nlaunch += 4 * p;
        }
        st->ms_kernels += tk.stop(c->stream);
        return 0;
    }
    const size_t nacc = 4 * (size_t)gc * p;
    psd_batchbuf bacc;
    PSD_CHECK(bacc.alloc(sizeof(double) * nacc));
    psd_bck_args g;
    g.T = dT; g.Z = dZ; g.A = dA; g.ab = k.dab; g.acc = bacc.d();
    g.n = n; g.p = p; g.qsub = CPLX ? -1 : k.schurindex - 1;
#ifdef PSD_HOSTSIM
    psd_bck_check_sim<CPLX>(g, gc * p);
#else
    const size_t lds = psd_bck_lds_bytes(n, CPLX);
    PSD_CHECK(c->lds_limit(reinterpret_cast<const void*>(psd_bck_check<CPLX>), lds));
    hipLaunchKernelGGL(psd_bck_check<CPLX>, dim3(gc * p), dim3(PSD_BCK_NT), lds, c->stream, g);
#endif
    st->nlaunch += 1;
    std::vector<double> acc(nacc);
    PSD_CHECK(psd_rt_d2h(acc.data(), bacc.d(), sizeof(double) * nacc, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    st->ms_kernels += tk.stop(c->stream);
    for (int q = 0; q < gc; ++q) {
        bool good = true;
        for (int l = 0; l < p; ++l) {
            const double* a = acc.data() + 4 * ((size_t)q * p + l);
            const double t = sqrt(a[0]), o = sqrt(a[2]);
            if (!checkpsd_verdict(n, o, sqrt(a[3]), t, a[1], k.thresh, k.strict, err + (size_t)q * p + l)) good = false;
            if (orth) orth[(size_t)q * p + l] = o;
            if (tri) tri[(size_t)q * p + l] = t;
        }
        if (ok) ok[q] = good ? 1 : 0;
        st->nfail += good ? 0 : 1;
    }
    return 0;
}

int bcheck_checked(const psd_ctx* c, int nb, int n, int p, const void* T, const void* Z, const void* A, char orient,
                   int schurindex, const double* err) {
    if (!c) return -1;
    if (nb < 0) return -2;
    if (n < 1) return -3;
    if (p < 1) return -4;
    if (nb == 0) return 0;
    if (!T || !Z || !A) return -5;
    if (orient != 'R' && orient != 'L') return -8;
    if (schurindex < 1 || schurindex > p) return -9;
    if (!err) return -13;
    if (c->shard_world > 1) return PSD_INFO_NOTIMPL;  // (a period-sharded context keeps a slice of Z: single problems only)
    return 0;
}

// the table of the residuals' factors on the device
int bcheck_table(psd_ctx* c, int p, const uint8_t* S, char orient, psd_batchbuf& dab) {
    std::vector<int> ab(2 * (size_t)p);
    const bool left = orient == 'L';
    for (int l = 0; l < p; ++l) {
        const int l1 = (l + 1) % p;
        const bool sl = S ? (S[l] != 0) : true;
        ab[2 * l] = (sl != left) ? l : l1;  // diagnostics.jl:249-253
        ab[2 * l + 1] = (sl != left) ? l1 : l;
    }
    PSD_CHECK(dab.alloc(sizeof(int) * ab.size()));
    PSD_CHECK(psd_rt_h2d(dab.ptr, ab.data(), sizeof(int) * ab.size(), c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));  // (ab leaves scope)
    return 0;
}

template <bool CPLX>
int bcheck_entry_dev(psd_ctx* c, int nb, int n, int p, const double* dT, const double* dZ, const double* dA, const uint8_t* S,
                     char orient, int schurindex, double thresh, int strict, double* err, double* orth, double* tri,
                     int32_t* ok, psd_bcheck_stats* stats, int* info) {
    batch_call<psd_bcheck_stats> entry(info, stats);
    psd_bcheck_stats* st = entry.s;
    if ((*info = bcheck_checked(c, nb, n, p, dT, dZ, dA, orient, schurindex, err)) != 0 || nb == 0) return *info;
    psd_batchbuf dab;
    if ((*info = bcheck_table(c, p, S, orient, dab)) != 0) return *info;
    const bcheck_call k{c, n, p, schurindex, strict, orient, thresh, S, (const int*)dab.ptr};
    const size_t pb = (size_t)(CPLX ? 2 : 1) * n * n * p;
    st->nb = nb;
    return *info = bevec_dev_groups(c, nb, sizeof(double) * 4 * p, [&](int q0, int gc) {
        const size_t r = (size_t)q0 * p;
        return bcheck_run<CPLX>(k, gc, dT + q0 * pb, dZ + q0 * pb, dA + q0 * pb, err + r, orth ? orth + r : nullptr,
                                tri ? tri + r : nullptr, ok ? ok + q0 : nullptr, st);
    });
}

template <bool CPLX>
int bcheck_entry_host(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, double* const* A, const uint8_t* S,
                      char orient, int schurindex, double thresh, int strict, double* err, double* orth, double* tri,
                      int32_t* ok, psd_bcheck_stats* stats, int* info) {
    batch_call<psd_bcheck_stats> entry(info, stats);
    psd_bcheck_stats* st = entry.s;
    if ((*info = bcheck_checked(c, nb, n, p, T, Z, A, orient, schurindex, err)) != 0 || nb == 0) return *info;
    psd_batchbuf dab;
    if ((*info = bcheck_table(c, p, S, orient, dab)) != 0) return *info;
    const bcheck_call k{c, n, p, schurindex, strict, orient, thresh, S, (const int*)dab.ptr};
    const size_t bd = (size_t)(CPLX ? 2 : 1) * n * n;
    const batch_list L[] = {{T, p, bd, BATCH_IN}, {Z, p, bd, BATCH_IN}, {A, p, bd, BATCH_IN}};
    psd_stats copies;  // (batch_staged leaves the time of the copies in a psd_stats)
    memset(&copies, 0, sizeof(copies));
    st->nb = nb;
    *info = batch_staged(c, nb, sizeof(double) * (3 * bd + 4) * p, L, &copies, batch_no_extra,
                         [&](int q0, int gc, double* const* d) {
        const size_t r = (size_t)q0 * p;
        return bcheck_run<CPLX>(k, gc, d[0], d[1], d[2], err + r, orth ? orth + r : nullptr, tri ? tri + r : nullptr,
                                ok ? ok + q0 : nullptr, st);
    });
    st->ms_copy = copies.ms_copy;
    return *info;
}

}  // namespace

extern "C" {

int psd_d_checkpsd_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, double* const* A,
                         const uint8_t* S, char orient, int schurindex, double thresh, int strict, double* err, double* orth,
                         double* tri, int32_t* ok, psd_bcheck_stats* stats, int* info) {
    return bcheck_entry_host<false>(c, nb, n, p, T, Z, A, S, orient, schurindex, thresh, strict, err, orth, tri, ok, stats, info);
}

int psd_z_checkpsd_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, double* const* A,
                         const uint8_t* S, char orient, int schurindex, double thresh, int strict, double* err, double* orth,
                         double* tri, int32_t* ok, psd_bcheck_stats* stats, int* info) {
    return bcheck_entry_host<true>(c, nb, n, p, T, Z, A, S, orient, schurindex, thresh, strict, err, orth, tri, ok, stats, info);
}

int psd_d_checkpsd_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, const double* dZ, const double* dA,
                             const uint8_t* S, char orient, int schurindex, double thresh, int strict, double* err,
                             double* orth, double* tri, int32_t* ok, psd_bcheck_stats* stats, int* info) {
    return bcheck_entry_dev<false>(c, nb, n, p, dT, dZ, dA, S, orient, schurindex, thresh, strict, err, orth, tri, ok, stats,
                                   info);
}

int psd_z_checkpsd_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, const double* dZ, const double* dA,
                             const uint8_t* S, char orient, int schurindex, double thresh, int strict, double* err,
                             double* orth, double* tri, int32_t* ok, psd_bcheck_stats* stats, int* info) {
    return bcheck_entry_dev<true>(c, nb, n, p, dT, dZ, dA, S, orient, schurindex, thresh, strict, err, orth, tri, ok, stats,
                                  info);
}

}  // extern "C"
