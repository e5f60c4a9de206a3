// Host drivers of the batched entries psd_d_phessenberg_batch / psd_d_pschur_batch / psd_d_pschur_batch_dev /
// psd_d_pschur_hess_batch: nb periodic problems of one shape (n, p) in one call — Floquet multipliers along a continuation
// branch, the orbits of a multiple-shooting sweep: order 8 ... 64, period 4 ... 100, hundreds to thousands of instances.
//
//   reduction    psd_bhess: one workgroup per problem, the whole batch in one launch (psd_bhess.h); above PSD_BH_NMAX the
//                multi-workgroup forms of hessenberg_dev / formq_dev, problem by problem on the slices of the batch buffer
//   Q formation  psd_bformq: one workgroup per (problem, factor); psd_btriu
//   iteration    iterate_dev(..., nprob, bws, pinfo) in chunks of at most PSD_SLOTS / 2 problems side by side on the slot
//                scheduler
//   'L'          psd_breverse_blocks over the whole batch: one launch before the reduction, at most two behind the iteration
//
// The first part of this file is what every batch family shares (the complex, signed, ordschur and eigvecs drivers come
// in behind it): the buffers, the head of an entry, the per-problem codes, the statistics sums, the group sizing and the
// staged group loop.  Device buffers of a call are owned by psd_batchbuf objects (re-allocatable, unlike psd_devbuf):
// every way out frees them.

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

// The head of a batch entry: info may be null, the caller's stats are zeroed (s: them, or a local stand-in), and
// head() gives the codes every pschur / phessenberg entry starts with.  S: psd_stats or psd_bevec_stats.
template <class S>
struct batch_call {
    int info_sink = 0;
    S local;
    S* s;
    std::vector<int> linfo;
    batch_call(int*& info, S* stats) : s(stats ? stats : &local) {
        if (!info) info = &info_sink;
        memset(s, 0, sizeof(S));
    }
    int head(const psd_ctx* c, int nb, int n, int p) const {
        if (!c) return -1;
        if (nb < 1) return -2;
        const int rc = check_dims(n, p);
        return rc != 0 ? rc - 1 : 0;  // (-3: n, -4: p)
    }
    // where the per-problem codes of nb problems go: the caller's array, or a stand-in
    int* infos(int* user, int nb) {
        linfo.assign(user ? 0 : nb, 0);
        return user ? user : linfo.data();
    }
};

// the code of one problem from what its kernel left (the real iteration never leaves PSD_ZB_TICKCAP)
int batch_info_code(int pinfo) {
    if (pinfo == PSD_LIST_OVERFLOW) return PSD_INFO_RUNTIME + 77;
    if (pinfo == PSD_ZB_TICKCAP) return PSD_INFO_RUNTIME + 0xfffe;
    return (pinfo != 0) ? (PSD_INFO_NOCONV + pinfo) : 0;
}
bool batch_fatal(int rc) { return rc < 0 || rc >= PSD_INFO_NOTIMPL; }
int psd_rt_code(int e) { return e != 0 ? PSD_INFO_RUNTIME + (e & 0xffff) : 0; }  // (what PSD_CHECK returns for e)
int batch_first_code(const int* infos, int nb) {
    for (int q = 0; q < nb; ++q)
        if (infos[q] != 0) return infos[q];
    return 0;
}

// the counters of one problem's single-call run (a), added to the call's
void batch_add_counts(psd_stats* s, const psd_stats& a, bool nlog = true) {
    s->niter += a.niter;
    s->nsweeps += a.nsweeps;
    s->nrqpass += a.nrqpass;
    s->ndefl1 += a.ndefl1;
    s->ndefl2 += a.ndefl2;
    s->reserved += a.reserved;
    s->nwindows += a.nwindows;
    s->nlaunch_step += a.nlaunch_step;
    if (nlog) s->nlog += a.nlog;
}
// what one group (a: the stats of a *_batch_core run) adds to the call's; the real entries do not pass nlog on
void batch_add_stats(psd_stats* s, const psd_stats& a, bool nlog) {
    batch_add_counts(s, a, nlog);
    if (a.maxits > s->maxits) s->maxits = a.maxits;
    s->window = a.window;
    s->ms_hess += a.ms_hess;
    s->ms_formq += a.ms_formq;
    s->ms_iter += a.ms_iter;
    s->ms_total += a.ms_total;
    s->ms_copy += a.ms_copy;
    s->bytes_hess += a.bytes_hess;
    s->bytes_formq += a.bytes_formq;
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

// try_alloc(g) allocates what groups of g problems need; while it fails, g is halved.  Returns try_alloc's code at g = 1.
template <class F>
int batch_alloc_halving(int& g, F try_alloc) {
    for (;;) {
        const int rc = try_alloc(g);
        if (rc == 0) return 0;
        (void)psd_rt_last_error();  // (the failed allocation is handled here)
        if (g == 1) return rc;
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

// One list of host matrices of a staged call: M holds `blocks` pointers per problem, problem-major, each to `doubles`
// doubles.  M == null: the call has no such list (no buffer, and the body sees a null device pointer).
enum { BATCH_IN = 1, BATCH_OUT = 2 };
struct batch_list {
    double* const* M;
    int blocks;
    size_t doubles;
    int dir;                    // BATCH_IN: uploaded before the body; BATCH_OUT: downloaded behind it
    const int* slot = nullptr;  // as batch_upload
};

// The staged group loop of every host entry.  Groups of at most batch_group(c, nb, per) problems; one device buffer per
// list, one staging buffer, and whatever alloc(g) adds for a group of g (0, or the code that ends the call at g = 1), all
// inside one halving loop.  Per group: the BATCH_IN lists go up in order, body(q0, gc, dev) runs on the device pointers
// of the lists (a non-zero code ends the call), the BATCH_OUT lists come down in order.  s (may be null) receives the
// time of the copies in ms_copy and nothing else.
template <size_t NL, class Alloc, class Body>
int batch_staged(psd_ctx* c, int nb, size_t per, const batch_list (&L)[NL], psd_stats* s, Alloc alloc, Body body) {
    int g = batch_group(c, nb, per);
    psd_batchbuf dbuf[NL];
    psd_hostbuf host;
    int rc = batch_alloc_halving(g, [&](int gg) {
        size_t stage = 0;
        int e = 0;
        for (size_t k = 0; k < NL && e == 0; ++k) {
            if (!L[k].M) continue;
            const size_t bytes = sizeof(double) * L[k].doubles * L[k].blocks * gg;
            e = dbuf[k].alloc(bytes);
            if (bytes > stage) stage = bytes;
        }
        if (e == 0 && !host.alloc(stage)) e = 3;
        if (e == 0) return alloc(gg);
        for (size_t k = 0; k < NL; ++k) dbuf[k].release();
        return psd_rt_code(e);
    });
    if (rc != 0) return rc;
    double* dev[NL];
    for (size_t k = 0; k < NL; ++k) dev[k] = dbuf[k].d();
    Timer tc;
    for (int q0 = 0; q0 < nb; q0 += g) {
        const int gc = (nb - q0 < g) ? (nb - q0) : g;
        if (s) tc.start(c->stream);
        for (size_t k = 0; k < NL; ++k)
            if (L[k].M && (L[k].dir & BATCH_IN) &&
                (rc = batch_upload(c, L[k].M, q0, gc, L[k].blocks, L[k].doubles, host.d(), dev[k], L[k].slot)) != 0)
                return rc;
        if (s) s->ms_copy += tc.stop(c->stream);
        if ((rc = body(q0, gc, (double* const*)dev)) != 0) return rc;
        if (s) tc.start(c->stream);
        for (size_t k = 0; k < NL; ++k)
            if (L[k].M && (L[k].dir & BATCH_OUT) &&
                (rc = batch_download(c, L[k].M, q0, gc, L[k].blocks, L[k].doubles, host.d(), dev[k], L[k].slot)) != 0)
                return rc;
        if (s) s->ms_copy += tc.stop(c->stream);
    }
    return 0;
}
const auto batch_no_extra = [](int) { return 0; };  // (an entry whose groups need the list buffers alone)

// PSD.jl:127-131, 1078-1092: 'L' works on the reversed sequence.  The nb * p blocks of dA (bd doubles each) are reversed
// problem by problem, run() works on them, and the reversal is undone: in dA, and in dZ (may be null) for Z_2 .. Z_p — Z_1
// stays.  A non-zero code of run() is returned at once.
template <class Run>
int batch_reversed(psd_ctx* c, bool left, int nb, int p, size_t bd, double* dA, double* dZ, Run run) {
    const bool rev = left && p > 1;
    if (rev) PSD_LAUNCH(psd_breverse_blocks, psd_dim3(nb * (p / 2)), PSD_HESS_NT, 0, c->stream, dA, bd, p, 0, p);
    const int rc = run();
    if (rc != 0) return rc;
    if (rev) {
        PSD_LAUNCH(psd_breverse_blocks, psd_dim3(nb * (p / 2)), PSD_HESS_NT, 0, c->stream, dA, bd, p, 0, p);
        if (dZ && p > 2) PSD_LAUNCH(psd_breverse_blocks, psd_dim3(nb * ((p - 1) / 2)), PSD_HESS_NT, 0, c->stream, dZ, bd, p, 1, p - 1);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// the real family

constexpr int PSD_BATCH_CHUNK = PSD_SLOTS / 2;  // problems side by side in one iterate_dev call

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

// band arrays of iterate_dev for nbc problems side by side (bws), and the staging of their eigenvalues (hw)
size_t bchunk_ws_doubles(int nbc, int n, int p) { return 8 * (size_t)nbc * (n + 8) + (size_t)nbc * (p + 8); }

// nbc <= PSD_BATCH_CHUNK Hessenberg-triangular problems (n >= 2) side by side through one iterate_dev call: dH / dZ
// [nbc][p][n][n] internal order, bws / hw as bchunk_ws_doubles says.  wr / wi (host, nbc * n); pinfo (nbc) receives what
// the kernel left per problem, cs the statistics of the run.  Returns a call-wide code, otherwise the code of a run that
// ended as a whole (the scheduler's lists overflowed), in *runinfo.
int biterate_chunk(psd_ctx* c, int nbc, int n, int p, double* dH, double* dZ, int wantT, int wantZ, int maxitfac, int mlog,
                   double* bws, double* hw, double* wr, double* wi, int* pinfo, psd_stats* cs, int* runinfo) {
    const size_t sb = (size_t)nbc * (n + 8);
    PSD_CHECK(psd_rt_memset(bws, 0, sizeof(double) * bchunk_ws_doubles(nbc, n, p), c->stream));
    psd_rstate st;
    memset(cs, 0, sizeof(*cs));
    for (int q = 0; q < nbc; ++q) pinfo[q] = 0;
    const int rc = iterate_dev(c, n, p, dH, dZ, wantT, wantZ, maxitfac, &st, cs, mlog, nbc, bws, pinfo);
    if (rc != 0) return rc;
    stats_from_state(cs, st);
    PSD_CHECK(psd_rt_d2h(hw, bws + 6 * sb, sizeof(double) * 2 * sb, c->stream));  // wr | wi
    PSD_CHECK(psd_rt_sync(c->stream));
    for (int q = 0; q < nbc; ++q) {
        memcpy(wr + (size_t)q * n, hw + (size_t)q * (n + 8), sizeof(double) * n);
        memcpy(wi + (size_t)q * n, hw + sb + (size_t)q * (n + 8), sizeof(double) * n);
    }
    *runinfo = batch_info_code(st.info);
    return 0;
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
    const size_t bws_doubles = bchunk_ws_doubles(chunk, n, p);
    psd_batchbuf dtau, bws;
    psd_hostbuf hw;
    PSD_CHECK(dtau.alloc(sizeof(double) * (size_t)nb * p * n));
    PSD_CHECK(bws.alloc(sizeof(double) * (bws_doubles > 2 * (size_t)nb ? bws_doubles : 2 * (size_t)nb)));
    if (!hw.alloc(sizeof(double) * 2 * (sbmax > (size_t)nb ? sbmax : (size_t)nb))) return PSD_INFO_RUNTIME + 3;
    Timer tall, tph;
    int callinfo = 0;
    tall.start(c->stream);
    rc = batch_reversed(c, left, nb, p, nn, dA, wantZ ? dZ : nullptr, [&]() {
        tph.start(c->stream);
        if (int e = bhessenberg_dev(c, nb, n, p, dA, dtau.d())) return e;
        s->ms_hess = tph.stop(c->stream);
        tph.start(c->stream);
        if (int e = bformq_dev(c, nb, n, p, dA, dtau.d(), wantZ ? dZ : nullptr)) return e;
        s->ms_formq = tph.stop(c->stream);
        tph.start(c->stream);
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
                psd_stats cs;
                int runinfo = 0;
                if (int e = biterate_chunk(c, nbc, n, p, dA + (size_t)q0 * p * nn, wantZ ? dZ + (size_t)q0 * p * nn : nullptr,
                                           wantT, wantZ, maxitfac, mlog, bws.d(), hw.d(), wr + (size_t)q0 * n,
                                           wi + (size_t)q0 * n, infos + q0, &cs, &runinfo))
                    return e;
                batch_add_stats(s, cs, false);
                for (int q = q0; q < q0 + nbc; ++q) infos[q] = batch_info_code(infos[q]);
                if (callinfo == 0) callinfo = runinfo;
            }
        }
        s->ms_iter = tph.stop(c->stream);
        return 0;
    });
    if (rc != 0) return rc;
    s->ms_total = tall.stop(c->stream);
    s->bytes_hess = nb * 2.0 * 8.0 * p * (5.0 / 6.0) * (double)n * n * n;
    s->bytes_formq = wantZ ? nb * 2.0 * 8.0 * p * (double)n * n * n / 3.0 : 0.0;
    PSD_CHECK(psd_rt_last_error());
    const int worst = batch_first_code(infos, nb);
    return worst != 0 ? worst : callinfo;
}

}  // namespace

extern "C" {

int psd_d_phessenberg_batch(psd_ctx* c, int nb, int n, int p, double* const* A, double* tau, psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    if ((*info = k.head(c, nb, n, p)) != 0) return *info;
    if (!A) return *info = -5;
    if (!tau) return *info = -6;
    if ((*info = c->reserve(n, p, false, 16)) != 0) return *info;
    const size_t nn = (size_t)n * n;
    const batch_list L[] = {{A, p, nn, BATCH_IN | BATCH_OUT}};
    psd_batchbuf dtau;
    Timer tk;
    auto extra = [&](int g) { return psd_rt_code(dtau.alloc(sizeof(double) * (size_t)g * p * n)); };
    auto body = [&](int q0, int gc, double* const* d) {
        tk.start(c->stream);
        if (int e = bhessenberg_dev(c, gc, n, p, d[0], dtau.d())) return e;
        k.s->ms_hess += tk.stop(c->stream);
        tk.start(c->stream);
        PSD_CHECK(psd_rt_d2h(tau + (size_t)q0 * p * n, dtau.d(), sizeof(double) * (size_t)gc * p * n, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        k.s->ms_copy += tk.stop(c->stream);
        return 0;
    };
    *info = batch_staged(c, nb, sizeof(double) * (nn + n) * p, L, k.s, extra, body);
    if (*info != 0) return *info;
    PSD_CHECK(psd_rt_last_error());
    k.s->ms_total = k.s->ms_hess;
    k.s->bytes_hess = nb * 2.0 * 8.0 * p * (5.0 / 6.0) * (double)n * n * n;
    return *info = 0;
}

int psd_d_pschur_batch_dev(psd_ctx* c, int nb, int n, int p, double* dA, char orient, int wantT, int wantZ, int maxitfac,
                           double* dZ, double* wr, double* wi, int* infos, int* schurindex, psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    if ((*info = k.head(c, nb, n, p)) != 0) return *info;
    if (!dA) return *info = -5;
    if (orient != 'R' && orient != 'L') return *info = -6;  // PSD.jl:175-177
    if (maxitfac < 1) return *info = -9;
    if (wantZ && !dZ) return *info = -10;
    if (!wr || !wi) return *info = -11;
    const int rc = pschur_batch_core(c, nb, n, p, dA, orient == 'L', wantT, wantZ, maxitfac, dZ, wr, wi, k.infos(infos, nb), k.s);
    if (schurindex) *schurindex = (orient == 'L') ? p : 1;
    return *info = rc;
}

int psd_d_pschur_batch(psd_ctx* c, int nb, int n, int p, double* const* A, char orient, int wantT, int wantZ, int maxitfac,
                       double* const* Z, double* wr, double* wi, int* infos, int* schurindex, psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    if ((*info = k.head(c, nb, n, p)) != 0) return *info;
    if (!A) return *info = -5;
    if (orient != 'R' && orient != 'L') return *info = -6;
    if (maxitfac < 1) return *info = -9;
    if (wantZ && !Z) return *info = -10;
    if (!wr || !wi) return *info = -11;
    const size_t nn = (size_t)n * n;
    const batch_list L[] = {{A, p, nn, BATCH_IN | BATCH_OUT}, {wantZ ? Z : nullptr, p, nn, BATCH_OUT}};
    int* pinfos = k.infos(infos, nb);
    int worst = 0;
    auto body = [&](int q0, int gc, double* const* d) {
        psd_stats gs;
        const int rc = pschur_batch_core(c, gc, n, p, d[0], orient == 'L', wantT, wantZ, maxitfac, d[1], wr + (size_t)q0 * n,
                                         wi + (size_t)q0 * n, pinfos + q0, &gs);
        // real rule: the core returns per-problem codes too; only a fatal one ends the group loop, the first of the
        // others is remembered and the loop goes on
        if (batch_fatal(rc)) return rc;
        if (rc != 0 && worst == 0) worst = rc;
        batch_add_stats(k.s, gs, false);
        return 0;
    };
    *info = batch_staged(c, nb, sizeof(double) * ((wantZ ? 2 : 1) * nn + n) * p, L, k.s, batch_no_extra, body);
    if (*info != 0) return *info;
    if (schurindex) *schurindex = (orient == 'L') ? p : 1;
    return *info = worst;
}

// Batch of small Hessenberg-triangular problems in ONE call (the projected problems of the
// Krylov driver, krylov.jl:575-592,800-829, are <= 40 x 40 — one such problem per launch chain is the worst case for a
// launch-bound design).  The slot scheduler of the real iteration (psd_rq_step_mb) runs the problems side by side: each
// starts as one range with its own leader, its own factors, band arrays, eigenvalues and sweep budget; splits and
// trains take further slots as in a single problem.
int psd_d_pschur_hess_batch(psd_ctx* c, int nb, int n, int p, double* const* H, double* const* Q, int wantT, int wantZ,
                            int maxitfac, double* wr, double* wi, int* infos, psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    if (c && nb > PSD_BATCH_CHUNK) return *info = -2;  // (what one iterate_dev call takes; ahead of n and p, as nb < 1 is)
    if ((*info = k.head(c, nb, n, p)) != 0) return *info;
    if (!H) return *info = -5;
    if (wantZ && !Q) return *info = -6;
    if (maxitfac < 1) return *info = -9;
    if (!wr || !wi) return *info = -10;
    const int mlog = 2 * maxitfac * n * nb + n * nb + 16;
    if ((*info = c->reserve(n, p, false, mlog)) != 0) return *info;
    const size_t nn = (size_t)n * n;
    const batch_list L[] = {{H, p, nn, BATCH_IN | BATCH_OUT}, {wantZ ? Q : nullptr, p, nn, BATCH_IN | BATCH_OUT}};
    psd_batchbuf bws;
    psd_hostbuf hw;
    std::vector<int> pinfo(nb, 0);
    int callinfo = 0;
    Timer tk;
    auto extra = [&](int g) {
        PSD_CHECK(bws.alloc(sizeof(double) * bchunk_ws_doubles(g, n, p)));
        return hw.alloc(sizeof(double) * 2 * (size_t)g * (n + 8)) ? 0 : PSD_INFO_RUNTIME + 3;
    };
    auto body = [&](int q0, int gc, double* const* d) {
        const size_t sb = (size_t)gc * (n + 8);
        tk.start(c->stream);
        if (n == 1) {  // PSD.jl:333-352
            PSD_CHECK(psd_rt_memset(bws.d(), 0, sizeof(double) * bchunk_ws_doubles(gc, n, p), c->stream));
            for (int q = 0; q < gc; ++q)
                PSD_LAUNCH(psd_scalar_product, psd_dim3(1), 64, 0, c->stream, (const double*)(d[0] + (size_t)q * p), p,
                           bws.d() + 6 * sb + (size_t)q * (n + 8), bws.d() + 7 * sb + (size_t)q * (n + 8));
            PSD_CHECK(psd_rt_d2h(hw.d(), bws.d() + 6 * sb, sizeof(double) * 2 * sb, c->stream));
            PSD_CHECK(psd_rt_sync(c->stream));
            for (int q = 0; q < gc; ++q) {
                wr[q0 + q] = hw.d()[(size_t)q * (n + 8)];
                wi[q0 + q] = hw.d()[sb + (size_t)q * (n + 8)];
            }
        } else {
            psd_stats cs;
            int runinfo = 0;
            if (int e = biterate_chunk(c, gc, n, p, d[0], d[1], wantT, wantZ, maxitfac, mlog, bws.d(), hw.d(),
                                       wr + (size_t)q0 * n, wi + (size_t)q0 * n, pinfo.data() + q0, &cs, &runinfo))
                return e;
            batch_add_stats(k.s, cs, true);
            // (the chase kernel's profile is that of the last group)
            k.s->step_kernel_ms_avg = cs.step_kernel_ms_avg;
            k.s->step_kernel_samples = cs.step_kernel_samples;
            memcpy(k.s->step_cycles, cs.step_cycles, sizeof(cs.step_cycles));
            if (callinfo == 0) callinfo = runinfo;
        }
        k.s->ms_iter += tk.stop(c->stream);
        return 0;
    };
    *info = batch_staged(c, nb, sizeof(double) * ((wantZ ? 2 : 1) * nn * p + bchunk_ws_doubles(1, n, p)), L, k.s, extra, body);
    k.s->ms_total = k.s->ms_iter;
    if (*info != 0) return *info;
    for (int q = 0; q < nb; ++q) pinfo[q] = batch_info_code(pinfo[q]);
    if (infos) memcpy(infos, pinfo.data(), sizeof(int) * (size_t)nb);
    const int worst = batch_first_code(pinfo.data(), nb);
    return *info = worst != 0 ? worst : callinfo;
}

}  // extern "C"
