// Host drivers of psd_d_gordschur_batch / psd_d_gordschur_batch_dev (psd_gbord.h): ordschur!(P, select) for nb Float64
// generalized periodic Schur forms of one shape and one signature, as psd_d_gpschur_batch leaves them.  Included at the
// end of psd_engine.cpp behind psd_zgbord_host.inl: the checks are its zgbord_checked, the entry bodies, the fallback loop
// and the code collection those of psd_bord_host.inl, the window rule, the fallback rule and the LDS size those of
// bord_real.
//
// Per group of problems: the selections and the signature go up once, then psd_gbord — every problem's whole reordering
// in one launch —, psd_gbord_values and psd_gbord_cleanup, and one read-back of the per-problem states, codes and scaled
// eigenvalues.  Orders above PSD_BORD_NMAX, and periods whose narrowest window does not fit the LDS, run rordschur_dev
// with the signature problem by problem on the slices of the batch buffers — every problem, also one with a purely real
// spectrum, which the single entry psd_d_gordschur would promote to the complex kernel.  A null or all-true signature
// stays on these kernels, as in psd_d_gpschur_batch and the pairs path of psd_d_gordschur: the result is always in the
// scaled form.

namespace {

struct gbord_real {
    static constexpr int ed = 1;  // doubles of a matrix element

    static bool fallback(const psd_ctx* c, int n, int p) { return bord_real::fallback(c, n, p); }

    // device workspace of one problem besides its factors: that of bord_real, the scaled eigenvalues and (once) the
    // signature
    static size_t ws_bytes(int n, int p) {
        return bord_real::ws_bytes(n, p) + (sizeof(psd_z) + sizeof(double) + sizeof(int)) * (size_t)n + (size_t)p;
    }
    struct ws_t {
        bord_real::ws_t r;
        psd_batchbuf alpha, beta, ascale, S;
        int alloc(int g, int n, int p) {
            if (int e = r.alloc(g, n, p)) return e;
            PSD_CHECK(alpha.alloc(sizeof(psd_z) * (size_t)g * n));
            PSD_CHECK(beta.alloc(sizeof(double) * (size_t)g * n));
            PSD_CHECK(ascale.alloc(sizeof(int) * (size_t)g * n));
            PSD_CHECK(S.alloc((size_t)p + 16));
            return 0;
        }
    };

    // gc problems resident on the device in the internal order (dH, dZ [gc][p][n][n]) and their rows k (k.S: the
    // signature in that order).  The eigenvalue rows of a problem whose code is non-zero are not written.
    static int group(const bord_call& k, int gc, double* dH, double* dZ, ws_t& ws) {
        psd_ctx* c = k.c;
        const int n = k.n, p = k.p;
        const size_t nn = (size_t)n * n;
        if (fallback(c, n, p)) {
            if (int e = c->reserve(n, p, false, 16)) return e;
            return bord_single_loop(k, gc, [&](int q, psd_stats* ps) {
                const bord_vals v = k.v.at(q, n);
                int pinfo = 0;
                // (the eigenvalues come down only behind a run that ended with code 0)
                return rordschur_dev(c, n, p, dH + (size_t)q * p * nn, k.wantZ ? dZ + (size_t)q * p * nn : nullptr,
                                     k.select + (size_t)q * n, k.wantZ, nullptr, nullptr, ps, &pinfo, k.S, v.a, v.b, v.sc);
            });
        }
        const int W = bord_real::window(c, n, p);
        const size_t lds = rord_lds_bytes(p, W);
        PSD_CHECK(c->lds_limit(reinterpret_cast<const void*>(psd_gbord), lds));
        PSD_CHECK(psd_rt_h2d(ws.r.sel.ptr, k.select, (size_t)gc * n, c->stream));
        PSD_CHECK(psd_rt_h2d(ws.S.ptr, k.S, (size_t)p, c->stream));
        psd_gbord_args a;
        a.b.H = dH;
        a.b.Z = k.wantZ ? dZ : nullptr;
        a.b.st = (psd_rostate*)ws.r.st.ptr;
        a.b.desc = (psd_apply_desc*)ws.r.desc.ptr;
        a.b.tq = (psd_tq*)ws.r.tq.ptr;
        a.b.cnt = (int*)ws.r.cnt.ptr;
        a.b.select = (const unsigned char*)ws.r.sel.ptr;
        a.b.wr = ws.r.wr.d();
        a.b.wi = ws.r.wi.d();
        a.b.xscr = ws.r.xscr.d();
        a.b.infos = (int*)ws.r.infos.ptr;
        a.b.n = n; a.b.p = p; a.b.wantZ = k.wantZ; a.b.W = W;
        a.b.maxwin = 2 * n * (n + 2) + 1024;  // (a block moves up by a row or more per window, and at most n blocks move)
        a.S = (const unsigned char*)ws.S.ptr;
        a.alpha = (psd_z*)ws.alpha.ptr;
        a.beta = ws.beta.d();
        a.ascale = (int*)ws.ascale.ptr;
        Timer t;
        t.start(c->stream);
        PSD_LAUNCH(psd_gbord, psd_dim3(gc), PSD_STEP_NT, lds, c->stream, a);
        PSD_LAUNCH(psd_gbord_values, psd_dim3((n + 63) / 64, gc), 64, 0, c->stream, a);
        PSD_LAUNCH(psd_gbord_cleanup, psd_dim3(n, gc), 64, 0, c->stream, a);
        const double ms = t.stop(c->stream);
        const size_t gn = (size_t)gc * n;
        std::vector<psd_rostate> hst(gc);
        std::vector<psd_z> ha(gn);
        std::vector<double> hb(gn);
        std::vector<int> hsc(gn);
        PSD_CHECK(psd_rt_d2h(hst.data(), ws.r.st.ptr, sizeof(psd_rostate) * (size_t)gc, c->stream));
        PSD_CHECK(psd_rt_d2h(ha.data(), ws.alpha.ptr, sizeof(psd_z) * gn, c->stream));
        PSD_CHECK(psd_rt_d2h(hb.data(), ws.beta.ptr, sizeof(double) * gn, c->stream));
        PSD_CHECK(psd_rt_d2h(hsc.data(), ws.ascale.ptr, sizeof(int) * gn, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        PSD_CHECK(psd_rt_last_error());
        return bord_collect(k, hst, PSD_LIST_OVERFLOW, PSD_INFO_RUNTIME + 77, W, ms, [&](size_t q) {
            const bord_vals v = k.v.at(q, n);
            memcpy(v.a, ha.data() + q * n, sizeof(psd_z) * n);
            memcpy(v.b, hb.data() + q * n, sizeof(double) * n);
            for (int j = 0; j < n; ++j) v.sc[j] = hsc[q * n + j];
        });
    }
};

}  // namespace

extern "C" {

int psd_d_gordschur_batch_dev(psd_ctx* c, int nb, int n, int p, void* dT, void* dZ, const uint8_t* S, char orient,
                              int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta,
                              int32_t* ascale, int* infos, int* nswaps, psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    signed_order o;
    if ((*info = zgbord_checked(c, nb, n, p, dT, dZ, S, orient, schurindex, select, wantZ, alpha, beta, ascale, o)) != 0 ||
        nb == 0)
        return *info;
    const bord_call call{c, n, p, wantZ, o.S.data(), select, {alpha, beta, ascale}, k.infos(infos, nb), nswaps, k.s};
    return *info = bord_entry_dev<gbord_real>(call, nb, dT, dZ, o.sA, o.sZ);
}

int psd_d_gordschur_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, const uint8_t* S, char orient,
                          int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta, int32_t* ascale,
                          int* infos, int* nswaps, psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    signed_order o;
    if ((*info = zgbord_checked(c, nb, n, p, T, Z, S, orient, schurindex, select, wantZ, alpha, beta, ascale, o)) != 0 ||
        nb == 0)
        return *info;
    const bord_call call{c, n, p, wantZ, o.S.data(), select, {alpha, beta, ascale}, k.infos(infos, nb), nswaps, k.s};
    return *info = bord_entry_host<gbord_real>(call, nb, T, Z, o.sA, o.sZ);
}

}  // extern "C"
