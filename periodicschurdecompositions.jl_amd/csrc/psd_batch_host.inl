// Host drivers of the batched entries psd_d_phessenberg_batch / psd_d_pschur_batch / psd_d_pschur_batch_dev: nb general
// (unreduced) periodic problems of one shape (n, p) in one call — Floquet multipliers along a continuation branch, the
// orbits of a multiple-shooting sweep: order 8 ... 64, period 4 ... 100, hundreds to thousands of instances.
//
//   reduction    psd_bhess: one workgroup per problem, the whole batch in one launch (psd_bhess.h); above PSD_BH_NMAX the
//                multi-workgroup forms of hessenberg_dev / formq_dev, problem by problem on the slices of the batch buffer
//   Q formation  psd_bformq: one workgroup per (problem, factor); psd_btriu
//   iteration    iterate_dev(..., nprob, bws, pinfo) in chunks of at most PSD_SLOTS / 2 problems side by side on the slot
//                scheduler, as psd_d_pschur_hess_batch runs them
//   'L'          psd_breverse_blocks over the whole batch: one launch before the reduction, at most two behind the iteration
//
// Device buffers of a call are owned by psd_batchbuf objects (re-allocatable, unlike psd_devbuf): every way out frees them.

namespace {

struct psd_batchbuf {
    void* ptr = nullptr;
    psd_batchbuf() {}
    psd_batchbuf(const psd_batchbuf&) = delete;
    psd_batchbuf& operator=(const psd_batchbuf&) = delete;
    ~psd_batchbuf() { release(); }
    int alloc(size_t bytes) {
        release();
        const int rc = psd_rt_malloc(&ptr, bytes);
        if (rc != 0) ptr = nullptr;
        return rc;
    }
    void release() {
        if (ptr) psd_rt_free(ptr);
        ptr = nullptr;
    }
    double* d() const { return (double*)ptr; }
};
struct psd_hostbuf {
    void* ptr = nullptr;
    psd_hostbuf() {}
    psd_hostbuf(const psd_hostbuf&) = delete;
    psd_hostbuf& operator=(const psd_hostbuf&) = delete;
    ~psd_hostbuf() { free(ptr); }
    bool alloc(size_t bytes) {
        free(ptr);
        ptr = malloc(bytes ? bytes : 16);
        return ptr != nullptr;
    }
    double* d() const { return (double*)ptr; }
};

constexpr int PSD_BATCH_CHUNK = PSD_SLOTS / 2;  // problems side by side in one iterate_dev call

int batch_info_code(int pinfo) {
    return (pinfo == PSD_LIST_OVERFLOW) ? (PSD_INFO_RUNTIME + 77) : ((pinfo != 0) ? (PSD_INFO_NOCONV + pinfo) : 0);
}
bool batch_fatal(int rc) { return rc < 0 || rc >= PSD_INFO_NOTIMPL; }

// PSD.jl:213-259 for nb problems: dH [nb][p][n][n] internal order, dtau [nb][p][n]
int bhessenberg_dev(psd_ctx* c, int nb, int n, int p, double* dH, double* dtau) {
    const size_t nn = (size_t)n * n;
    PSD_CHECK(psd_rt_memset(dtau, 0, sizeof(double) * (size_t)nb * p * n, c->stream));
    if (n < 2) return 0;
    if (n <= c->bh_nmax) {
        PSD_LAUNCH(psd_bhess, psd_dim3(nb), PSD_HESS_NT, psd_bhess_lds_bytes(n), c->stream, dH, dtau, n, p);
        return 0;
    }
    for (int q = 0; q < nb; ++q) {
        const int rc = hessenberg_dev(c, n, p, dH + (size_t)q * p * nn, dtau + (size_t)q * p * n);
        if (rc != 0) return rc;
    }
    return 0;
}

// Q_j of every problem (dQ may be null: the factors alone), then the clean-up of the reflector storage
int bformq_dev(psd_ctx* c, int nb, int n, int p, double* dH, const double* dtau, double* dQ) {
    const size_t nn = (size_t)n * n;
    if (dQ) {
        if (n <= c->bh_nmax) {
            PSD_LAUNCH(psd_bformq, psd_dim3(nb * p), PSD_HESS_NT, PSD_HESS_NT * sizeof(double), c->stream,
                       (const double*)dH, dtau, dQ, n, p);
        } else {
            for (int q = 0; q < nb; ++q) {
                const int rc = formq_dev(c, n, p, dH + (size_t)q * p * nn, dtau + (size_t)q * p * n, dQ + (size_t)q * p * nn);
                if (rc != 0) return rc;
            }
        }
    }
    if (n >= 2) PSD_LAUNCH(psd_btriu, psd_dim3(nb * p), PSD_HESS_NT, 0, c->stream, dH, n, p);
    return 0;
}

void batch_add_stats(psd_stats* s, const psd_stats& a) {
    s->niter += a.niter;
    if (a.maxits > s->maxits) s->maxits = a.maxits;
    s->nsweeps += a.nsweeps;
    s->nrqpass += a.nrqpass;
    s->ndefl1 += a.ndefl1;
    s->ndefl2 += a.ndefl2;
    s->nwindows += a.nwindows;
    s->nlaunch_step += a.nlaunch_step;
    s->window = a.window;
    s->reserved += a.reserved;
    s->ms_hess += a.ms_hess;
    s->ms_formq += a.ms_formq;
    s->ms_iter += a.ms_iter;
    s->ms_total += a.ms_total;
    s->ms_copy += a.ms_copy;
    s->bytes_hess += a.bytes_hess;
    s->bytes_formq += a.bytes_formq;
}

// The whole path for nb problems resident on the device: dA / dZ [nb][p][n][n] in user order.  wr / wi (host, nb * n),
// infos (host, nb).  s receives the counters and times of this call.  Returns the first non-zero per-problem code, or a
// call-wide (argument / runtime) code.
int pschur_batch_core(psd_ctx* c, int nb, int n, int p, double* dA, bool left, int wantT, int wantZ, int maxitfac, double* dZ,
                      double* wr, double* wi, int* infos, psd_stats* s) {
    memset(s, 0, sizeof(*s));
    if (c->shard_world > 1) return PSD_INFO_NOTIMPL;  // (a period-sharded context keeps a slice of Z: single problems only)
    const size_t nn = (size_t)n * n;
    const int chunk = nb < PSD_BATCH_CHUNK ? nb : PSD_BATCH_CHUNK;
    const int mlog = 2 * maxitfac * n * chunk + n * chunk + 16;
    int rc = c->reserve(n, p, false, mlog);
    if (rc != 0) return rc;
    const size_t sbmax = (size_t)chunk * (n + 8);
    const size_t bws_doubles = 8 * sbmax + (size_t)chunk * (p + 8);
    psd_batchbuf dtau, bws;
    psd_hostbuf hw;
    PSD_CHECK(dtau.alloc(sizeof(double) * (size_t)nb * p * n));
    PSD_CHECK(bws.alloc(sizeof(double) * (bws_doubles > 2 * (size_t)nb ? bws_doubles : 2 * (size_t)nb)));
    if (!hw.alloc(sizeof(double) * 2 * (sbmax > (size_t)nb ? sbmax : (size_t)nb))) return PSD_INFO_RUNTIME + 3;
    Timer tall, tph;
    tall.start(c->stream);
    // PSD.jl:127-131: 'L' works on the reversed sequence
    if (left && p > 1) PSD_LAUNCH(psd_breverse_blocks, psd_dim3(nb * (p / 2)), PSD_HESS_NT, 0, c->stream, dA, nn, p, 0, p);
    tph.start(c->stream);
    if ((rc = bhessenberg_dev(c, nb, n, p, dA, dtau.d())) != 0) return rc;
    s->ms_hess = tph.stop(c->stream);
    tph.start(c->stream);
    if ((rc = bformq_dev(c, nb, n, p, dA, dtau.d(), wantZ ? dZ : nullptr)) != 0) return rc;
    s->ms_formq = tph.stop(c->stream);
    tph.start(c->stream);
    int callinfo = 0;
    if (n == 1) {  // PSD.jl:333-352
        PSD_LAUNCH(psd_bscalar_product, psd_dim3((nb + 63) / 64), 64, 0, c->stream, (const double*)dA, p, nb, bws.d(),
                   bws.d() + nb);
        PSD_CHECK(psd_rt_d2h(hw.d(), bws.d(), sizeof(double) * 2 * (size_t)nb, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        for (int q = 0; q < nb; ++q) {
            wr[q] = hw.d()[q];
            wi[q] = hw.d()[nb + q];
            infos[q] = 0;
        }
    } else {
        for (int q0 = 0; q0 < nb; q0 += PSD_BATCH_CHUNK) {
            const int nbc = (nb - q0 < PSD_BATCH_CHUNK) ? (nb - q0) : PSD_BATCH_CHUNK;
            const size_t sb = (size_t)nbc * (n + 8);
            PSD_CHECK(psd_rt_memset(bws.d(), 0, sizeof(double) * (8 * sb + (size_t)nbc * (p + 8)), c->stream));
            psd_rstate st;
            psd_stats cs;
            memset(&cs, 0, sizeof(cs));
            std::vector<int> pinfo(nbc, 0);
            rc = iterate_dev(c, n, p, dA + (size_t)q0 * p * nn, wantZ ? dZ + (size_t)q0 * p * nn : nullptr, wantT, wantZ,
                             maxitfac, &st, &cs, mlog, nbc, bws.d(), pinfo.data());
            if (rc != 0) return rc;
            stats_from_state(&cs, st);
            batch_add_stats(s, cs);
            PSD_CHECK(psd_rt_d2h(hw.d(), bws.d() + 6 * sb, sizeof(double) * 2 * sb, c->stream));  // wr | wi
            PSD_CHECK(psd_rt_sync(c->stream));
            for (int q = 0; q < nbc; ++q) {
                memcpy(wr + (size_t)(q0 + q) * n, hw.d() + (size_t)q * (n + 8), sizeof(double) * n);
                memcpy(wi + (size_t)(q0 + q) * n, hw.d() + sb + (size_t)q * (n + 8), sizeof(double) * n);
                infos[q0 + q] = batch_info_code(pinfo[q]);
            }
            if (callinfo == 0 && st.info != 0) callinfo = batch_info_code(st.info);
        }
    }
    s->ms_iter = tph.stop(c->stream);
    // PSD.jl:1078-1092: undo the reversal; Z_1 stays, Z_2..Z_p reverse
    if (left && p > 1) {
        PSD_LAUNCH(psd_breverse_blocks, psd_dim3(nb * (p / 2)), PSD_HESS_NT, 0, c->stream, dA, nn, p, 0, p);
        if (wantZ && p > 2)
            PSD_LAUNCH(psd_breverse_blocks, psd_dim3(nb * ((p - 1) / 2)), PSD_HESS_NT, 0, c->stream, dZ, nn, p, 1, p - 1);
    }
    s->ms_total = tall.stop(c->stream);
    s->bytes_hess = nb * 2.0 * 8.0 * p * (5.0 / 6.0) * (double)n * n * n;
    s->bytes_formq = wantZ ? nb * 2.0 * 8.0 * p * (double)n * n * n / 3.0 : 0.0;
    PSD_CHECK(psd_rt_last_error());
    int worst = 0;
    for (int q = 0; q < nb && worst == 0; ++q) worst = infos[q];
    return worst != 0 ? worst : callinfo;
}

// How many problems of `per` device bytes a host entry takes to the device at once: what fits half of the free device
// memory; PSD_BATCH_GROUP in the environment at psd_create lowers it (the tests reach the group loop with it)
int batch_group(const psd_ctx* c, int nb, size_t per) {
    size_t g = (size_t)nb;
#ifndef PSD_HOSTSIM
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && per > 0) {
        const size_t fit = fr / 2 / per;
        if (fit < g) g = fit;
    }
#else
    (void)per;
#endif
    if (c->batch_group >= 1 && (size_t)c->batch_group < g) g = (size_t)c->batch_group;
    return g < 1 ? 1 : (int)g;
}

// Device and staging buffers for groups of g problems; when an allocation fails, g is halved until the buffers fit
int batch_buffers(int& g, size_t per_doubles, int nbufs, psd_batchbuf* dev, psd_hostbuf& host) {
    for (;;) {
        int rc = 0;
        for (int k = 0; k < nbufs && rc == 0; ++k) rc = dev[k].alloc(sizeof(double) * per_doubles * g);
        if (rc == 0 && !host.alloc(sizeof(double) * per_doubles * g)) rc = 3;
        if (rc == 0) return 0;
        for (int k = 0; k < nbufs; ++k) dev[k].release();
        (void)psd_rt_last_error();  // (the failed allocation is handled here)
        if (g == 1) return PSD_INFO_RUNTIME + (rc & 0xffff);
        g = (g + 1) / 2;
    }
}

// the factors of problems [q0, q0 + g) between the caller's matrices and one device buffer, through one staging buffer;
// slot (0-based, as ord_slots returns it; null: the identity): the caller's factor slot[j] of a problem is its device block j
int batch_upload(psd_ctx* c, double* const* M, int q0, int g, int p, size_t nn, double* host, double* dev,
                 const int* slot = nullptr) {
    for (size_t q = 0; q < (size_t)g; ++q)
        for (int j = 0; j < p; ++j)
            memcpy(host + (q * p + j) * nn, M[(q0 + q) * p + (slot ? slot[j] : j)], nn * sizeof(double));
    PSD_CHECK(psd_rt_h2d(dev, host, sizeof(double) * nn * p * g, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));  // (the staging buffer is reused)
    return 0;
}
int batch_download(psd_ctx* c, double* const* M, int q0, int g, int p, size_t nn, double* host, const double* dev,
                   const int* slot = nullptr) {
    PSD_CHECK(psd_rt_d2h(host, dev, sizeof(double) * nn * p * g, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    for (size_t q = 0; q < (size_t)g; ++q)
        for (int j = 0; j < p; ++j)
            memcpy(M[(q0 + q) * p + (slot ? slot[j] : j)], host + (q * p + j) * nn, nn * sizeof(double));
    return 0;
}

}  // namespace

extern "C" {

int psd_d_phessenberg_batch(psd_ctx* c, int nb, int n, int p, double* const* A, double* tau, psd_stats* stats, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c) return *info = -1;
    if (nb < 1) return *info = -2;
    if ((*info = check_dims(n, p)) != 0) return *info = *info - 1;
    if (!A) return *info = -5;
    if (!tau) return *info = -6;
    if ((*info = c->reserve(n, p, false, 16)) != 0) return *info;
    const size_t nn = (size_t)n * n;
    int g = batch_group(c, nb, sizeof(double) * (nn + n) * p);
    psd_batchbuf dH, dtau;
    psd_hostbuf hst;
    if ((*info = batch_buffers(g, nn * p, 1, &dH, hst)) != 0) return *info;
    PSD_CHECK(dtau.alloc(sizeof(double) * (size_t)g * p * n));
    psd_stats local;
    memset(&local, 0, sizeof(local));
    psd_stats* s = stats ? stats : &local;
    Timer tc, tk;
    for (int q0 = 0; q0 < nb; q0 += g) {
        const int gc = (nb - q0 < g) ? (nb - q0) : g;
        tc.start(c->stream);
        if ((*info = batch_upload(c, A, q0, gc, p, nn, hst.d(), dH.d())) != 0) return *info;
        s->ms_copy += tc.stop(c->stream);
        tk.start(c->stream);
        if ((*info = bhessenberg_dev(c, gc, n, p, dH.d(), dtau.d())) != 0) return *info;
        s->ms_hess += tk.stop(c->stream);
        tc.start(c->stream);
        if ((*info = batch_download(c, A, q0, gc, p, nn, hst.d(), dH.d())) != 0) return *info;
        PSD_CHECK(psd_rt_d2h(tau + (size_t)q0 * p * n, dtau.d(), sizeof(double) * (size_t)gc * p * n, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        s->ms_copy += tc.stop(c->stream);
    }
    PSD_CHECK(psd_rt_last_error());
    s->ms_total = s->ms_hess;
    s->bytes_hess = nb * 2.0 * 8.0 * p * (5.0 / 6.0) * (double)n * n * n;
    return *info = 0;
}

int psd_d_pschur_batch_dev(psd_ctx* c, int nb, int n, int p, double* dA, char orient, int wantT, int wantZ, int maxitfac,
                           double* dZ, double* wr, double* wi, int* infos, int* schurindex, psd_stats* stats, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c) return *info = -1;
    if (nb < 1) return *info = -2;
    if ((*info = check_dims(n, p)) != 0) return *info = *info - 1;
    if (!dA) return *info = -5;
    if (orient != 'R' && orient != 'L') return *info = -6;  // PSD.jl:175-177
    if (maxitfac < 1) return *info = -9;
    if (wantZ && !dZ) return *info = -10;
    if (!wr || !wi) return *info = -11;
    psd_stats local;
    psd_stats* s = stats ? stats : &local;
    std::vector<int> linfo(infos ? 0 : nb, 0);
    const int rc = pschur_batch_core(c, nb, n, p, dA, orient == 'L', wantT, wantZ, maxitfac, dZ, wr, wi,
                                     infos ? infos : linfo.data(), s);
    if (schurindex) *schurindex = (orient == 'L') ? p : 1;
    return *info = rc;
}

int psd_d_pschur_batch(psd_ctx* c, int nb, int n, int p, double* const* A, char orient, int wantT, int wantZ, int maxitfac,
                       double* const* Z, double* wr, double* wi, int* infos, int* schurindex, psd_stats* stats, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c) return *info = -1;
    if (nb < 1) return *info = -2;
    if ((*info = check_dims(n, p)) != 0) return *info = *info - 1;
    if (!A) return *info = -5;
    if (orient != 'R' && orient != 'L') return *info = -6;
    if (maxitfac < 1) return *info = -9;
    if (wantZ && !Z) return *info = -10;
    if (!wr || !wi) return *info = -11;
    const size_t nn = (size_t)n * n;
    int g = batch_group(c, nb, sizeof(double) * ((wantZ ? 2 : 1) * nn + n) * p);
    psd_batchbuf dbuf[2];
    psd_hostbuf hst;
    if ((*info = batch_buffers(g, nn * p, wantZ ? 2 : 1, dbuf, hst)) != 0) return *info;
    psd_stats local;
    memset(&local, 0, sizeof(local));
    psd_stats* s = stats ? stats : &local;
    std::vector<int> linfo(infos ? 0 : nb, 0);
    int* pinfos = infos ? infos : linfo.data();
    Timer tc;
    int worst = 0;
    for (int q0 = 0; q0 < nb; q0 += g) {
        const int gc = (nb - q0 < g) ? (nb - q0) : g;
        psd_stats gs;
        tc.start(c->stream);
        if ((*info = batch_upload(c, A, q0, gc, p, nn, hst.d(), dbuf[0].d())) != 0) return *info;
        double ms_copy = tc.stop(c->stream);
        const int rc = pschur_batch_core(c, gc, n, p, dbuf[0].d(), orient == 'L', wantT, wantZ, maxitfac, dbuf[1].d(),
                                         wr + (size_t)q0 * n, wi + (size_t)q0 * n, pinfos + q0, &gs);
        if (batch_fatal(rc)) return *info = rc;
        if (rc != 0 && worst == 0) worst = rc;
        tc.start(c->stream);
        if ((*info = batch_download(c, A, q0, gc, p, nn, hst.d(), dbuf[0].d())) != 0) return *info;
        if (wantZ && (*info = batch_download(c, Z, q0, gc, p, nn, hst.d(), dbuf[1].d())) != 0) return *info;
        ms_copy += tc.stop(c->stream);
        batch_add_stats(s, gs);
        s->ms_copy += ms_copy;
    }
    if (schurindex) *schurindex = (orient == 'L') ? p : 1;
    return *info = worst;
}

}  // extern "C"
