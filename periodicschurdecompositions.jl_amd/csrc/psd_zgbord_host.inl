// Host drivers of psd_z_gordschur_batch / psd_z_gordschur_batch_dev (psd_zgbord.h): ordschur!(P, select) for nb ComplexF64
// generalized periodic Schur forms of one shape and one signature, as psd_z_gpschur_batch leaves them.  Included at the
// end of psd_engine.cpp behind psd_zbord_host.inl, whose argument checks, group loop and device permutations it shares.
//
// Per group of problems: the selections go up once, then psd_zgbord — every problem's whole reordering in one launch —
// and psd_zgbord_values, and one read-back of the per-problem states, codes and scaled eigenvalues.  Orders above
// PSD_BORD_NMAX, and periods whose narrowest window does not fit the LDS, run zgordschur_dev problem by problem on the
// slices of the batch buffers.  A null or all-true signature is the call of psd_z_ordschur_batch[_dev].
//
// Measured for this path: the sweep of tools/ordschur_batch_timing.py --signed (nb = 256, alternating S, n = 8 ... 64,
// p = 4 and 16) against the loop of single psd_z_gordschur calls — the batched call is ahead at every swept shape, 38 to
// 101 x in wall time (profiles/batch/README.md).  Orders 65 ... 128 have not been swept; the cap is the shared
// PSD_BORD_NMAX.

namespace {

// Window of the batched kernel: zgordschur_dev's choice, narrowed to the smallest candidate that still holds the whole
// problem when one does (zbord_window); 0: none fits.  PSD_BORD_W narrows it further.
int zgbord_window(const psd_ctx* c, int n, int p) {
    int W = choose_window_lds({32, 24, 20, 16, 12, 10, 8, 6, 4}, [&](int w) { return zgord_lds_bytes(p, w); }, n);
    if (W != 0 && c->bord_w >= PSD_ZGBORD_WMIN && c->bord_w < W) W = c->bord_w;
    return W;
}

size_t zgbord_lds_bytes(int p, int W) {
    const size_t a = zgord_lds_bytes(p, W), b = psd_zgbqz_apply_lds_bytes();
    return a > b ? a : b;
}

// device workspace of one problem besides its factors
size_t zgbord_ws_bytes(int n, int p) {
    return sizeof(psd_ostate) + sizeof(psd_gapply_desc) + sizeof(psd_ztr) * (size_t)p * PSD_GTR_CAP + sizeof(int) * (size_t)(p + 1) +
           (size_t)n + (sizeof(psd_z) + sizeof(double) + sizeof(int)) * (size_t)n;
}

// (S: the signature of the call in the internal order, p flags)
struct zgbord_ws {
    psd_batchbuf st, desc, tr, cnt, sel, alpha, beta, ascale, infos, S;
    int alloc(int g, int n, int p) {
        PSD_CHECK(st.alloc(sizeof(psd_ostate) * (size_t)g));
        PSD_CHECK(desc.alloc(sizeof(psd_gapply_desc) * (size_t)g));
        PSD_CHECK(tr.alloc(sizeof(psd_ztr) * (size_t)g * p * PSD_GTR_CAP));
        PSD_CHECK(cnt.alloc(sizeof(int) * (size_t)g * p));
        PSD_CHECK(sel.alloc((size_t)g * n));
        PSD_CHECK(alpha.alloc(sizeof(psd_z) * (size_t)g * n));
        PSD_CHECK(beta.alloc(sizeof(double) * (size_t)g * n));
        PSD_CHECK(ascale.alloc(sizeof(int) * (size_t)g * n));
        PSD_CHECK(infos.alloc(sizeof(int) * (size_t)g));
        PSD_CHECK(S.alloc((size_t)p + 16));
        return 0;
    }
};

bool zgbord_fallback(const psd_ctx* c, int n, int p) { return n > c->bord_nmax || zgbord_window(c, n, p) == 0; }

// gc problems resident on the device in the internal order (dH, dZ [gc][p][n][n]); S: the internal signature (host, p
// flags); select, alpha (pairs), beta, ascale, infos, nswaps: the host rows of these problems.  The rows of a problem
// whose code is non-zero are not written.  Adds to s.
int zgbord_group(psd_ctx* c, int gc, int n, int p, psd_z* dH, psd_z* dZ, const uint8_t* S, const uint8_t* select, int wantZ,
                 double* alpha, double* beta, int32_t* ascale, int* infos, int* nswaps, psd_stats* s, zgbord_ws& ws) {
    const size_t nn = (size_t)n * n;
    if (zgbord_fallback(c, n, p)) {
        int rc = c->zreserve(n, p, false, 16);
        if (rc == 0) rc = c->zgreserve(n, p);
        if (rc != 0) return rc;
        for (int q = 0; q < gc; ++q) {
            psd_stats ps;
            memset(&ps, 0, sizeof(ps));
            int pinfo = 0;
            // (the eigenvalues come down only behind a run that ended with code 0)
            rc = zgordschur_dev(c, n, p, dH + (size_t)q * p * nn, wantZ ? dZ + (size_t)q * p * nn : nullptr, S,
                                select + (size_t)q * n, wantZ, alpha + 2 * (size_t)q * n, beta + (size_t)q * n,
                                ascale + (size_t)q * n, &ps, &pinfo);
            if (batch_fatal(rc)) return rc;
            infos[q] = rc;
            if (nswaps) nswaps[q] = ps.nsweeps;
            s->nsweeps += ps.nsweeps;
            s->nwindows += ps.nwindows;
            s->nlaunch_step += ps.nlaunch_step;
            s->window = ps.window;
            s->ms_iter += ps.ms_iter;
            s->ms_total += ps.ms_total;
        }
        return 0;
    }
    const int W = zgbord_window(c, n, p);
    const size_t lds = zgbord_lds_bytes(p, W);
    PSD_CHECK(c->lds_limit(reinterpret_cast<const void*>(psd_zgbord), lds));
    PSD_CHECK(psd_rt_h2d(ws.sel.ptr, select, (size_t)gc * n, c->stream));
    PSD_CHECK(psd_rt_h2d(ws.S.ptr, S, (size_t)p, c->stream));
    psd_zgbord_args a;
    a.H = dH;
    a.Z = wantZ ? dZ : nullptr;
    a.S = (const unsigned char*)ws.S.ptr;
    a.st = (psd_ostate*)ws.st.ptr;
    a.desc = (psd_gapply_desc*)ws.desc.ptr;
    a.tr = (psd_ztr*)ws.tr.ptr;
    a.cnt = (int*)ws.cnt.ptr;
    a.select = (const unsigned char*)ws.sel.ptr;
    a.alpha = (psd_z*)ws.alpha.ptr;
    a.beta = ws.beta.d();
    a.ascale = (int*)ws.ascale.ptr;
    a.infos = (int*)ws.infos.ptr;
    a.n = n; a.p = p; a.wantZ = wantZ; a.W = W;
    a.maxwin = n * (n + 2) + 1024;  // (a selected eigenvalue moves up by a row or more per window, and at most n of them move)
    Timer t;
    t.start(c->stream);
    PSD_LAUNCH(psd_zgbord, psd_dim3(gc), PSD_STEP_NT, lds, c->stream, a);
    PSD_LAUNCH(psd_zgbord_values, psd_dim3((n + 63) / 64, gc), 64, 0, c->stream, a);
    const double ms = t.stop(c->stream);
    const size_t gn = (size_t)gc * n;
    std::vector<psd_ostate> hst(gc);
    std::vector<psd_z> ha(gn);
    std::vector<double> hb(gn);
    std::vector<int> hsc(gn);
    PSD_CHECK(psd_rt_d2h(hst.data(), ws.st.ptr, sizeof(psd_ostate) * (size_t)gc, c->stream));
    PSD_CHECK(psd_rt_d2h(ha.data(), ws.alpha.ptr, sizeof(psd_z) * gn, c->stream));
    PSD_CHECK(psd_rt_d2h(hb.data(), ws.beta.ptr, sizeof(double) * gn, c->stream));
    PSD_CHECK(psd_rt_d2h(hsc.data(), ws.ascale.ptr, sizeof(int) * gn, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    for (int q = 0; q < gc; ++q) {
        if (hst[q].info == PSD_ZGBORD_WINCAP) return PSD_INFO_RUNTIME + 0xfffd;  // (a run that does not end)
        infos[q] = hst[q].info;  // 0, 2000 + row (IllConditionedException), 3000 (SingularException)
        if (nswaps) nswaps[q] = hst[q].nswaps;
        if (hst[q].info == 0) {
            memcpy(alpha + 2 * (size_t)q * n, ha.data() + (size_t)q * n, sizeof(psd_z) * n);
            memcpy(beta + (size_t)q * n, hb.data() + (size_t)q * n, sizeof(double) * n);
            for (int j = 0; j < n; ++j) ascale[(size_t)q * n + j] = hsc[(size_t)q * n + j];
        }
        s->nsweeps += hst[q].nswaps;
        s->nwindows += hst[q].nwindows;
    }
    s->nlaunch_step += 1;
    s->window = W;
    s->ms_iter += ms;
    s->ms_total += ms;
    return 0;
}

// the argument codes of psd_z_ordschur_batch (zbord_checked) and the working order of the signed call; -10: the entry
// of S that lands first in that order is false (generalized.jl:182)
int zgbord_checked(psd_ctx* c, int nb, int n, int p, const void* T, const void* Z, const uint8_t* S, char orient,
                   int schurindex, const uint8_t* select, int wantZ, const double* alpha, const double* beta,
                   const int32_t* ascale, signed_order& o) {
    std::vector<int> slotA, slotZ;
    if (int e = zbord_checked(c, nb, n, p, T, Z, orient, schurindex, select, wantZ, alpha, beta, ascale, slotA, slotZ)) return e;
    if (nb == 0) return 0;
    return signed_slots(orient, schurindex, p, S, o) != 0 ? -10 : 0;
}

}  // namespace

extern "C" {

int psd_z_gordschur_batch_dev(psd_ctx* c, int nb, int n, int p, void* dT, void* dZ, const uint8_t* S, char orient,
                              int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta,
                              int32_t* ascale, int* infos, int* nswaps, psd_stats* stats, int* info) {
    if (zgb_all_true(S, p))  // (the all-true kernel, as psd_z_gpschur_batch_dev keeps it)
        return psd_z_ordschur_batch_dev(c, nb, n, p, dT, dZ, orient, schurindex, select, wantZ, alpha, beta, ascale, infos,
                                        nswaps, stats, info);
    batch_call<psd_stats> k(info, stats);
    signed_order o;
    if ((*info = zgbord_checked(c, nb, n, p, dT, dZ, S, orient, schurindex, select, wantZ, alpha, beta, ascale, o)) != 0 ||
        nb == 0)
        return *info;
    const size_t nn = (size_t)n * n;
    int* pinfos = k.infos(infos, nb);
    psd_z* H = (psd_z*)dT;
    psd_z* Z = wantZ ? (psd_z*)dZ : nullptr;
    zgbord_ws ws;
    auto group = [&](int q0, int gc) {
        return zgbord_group(c, gc, n, p, H + (size_t)q0 * p * nn, Z ? Z + (size_t)q0 * p * nn : nullptr, o.S.data(),
                            select + (size_t)q0 * n, wantZ, alpha + 2 * (size_t)q0 * n, beta + (size_t)q0 * n,
                            ascale + (size_t)q0 * n, pinfos + q0, nswaps ? nswaps + q0 : nullptr, k.s, ws);
    };
    return *info = bord_dev_run(c, nb, n, p, 2 * nn, (double*)H, (double*)Z, o.sA, o.sZ, zgbord_fallback(c, n, p),
                                zgbord_ws_bytes(n, p), ws, pinfos, group);
}

int psd_z_gordschur_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, const uint8_t* S, char orient,
                          int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta, int32_t* ascale,
                          int* infos, int* nswaps, psd_stats* stats, int* info) {
    if (zgb_all_true(S, p))
        return psd_z_ordschur_batch(c, nb, n, p, T, Z, orient, schurindex, select, wantZ, alpha, beta, ascale, infos, nswaps,
                                    stats, info);
    batch_call<psd_stats> k(info, stats);
    signed_order o;
    if ((*info = zgbord_checked(c, nb, n, p, T, Z, S, orient, schurindex, select, wantZ, alpha, beta, ascale, o)) != 0 ||
        nb == 0)
        return *info;
    const size_t nn2 = 2 * (size_t)n * n;  // doubles of one factor
    // user slot <-> internal slot on the way through the staging buffer, as psd_z_gordschur copies
    const batch_list L[] = {{T, p, nn2, BATCH_IN | BATCH_OUT, o.sA.data()},
                            {wantZ ? Z : nullptr, p, nn2, BATCH_IN | BATCH_OUT, o.sZ.data()}};
    int* pinfos = k.infos(infos, nb);
    zgbord_ws ws;
    auto extra = [&](int g) { return zgbord_fallback(c, n, p) ? 0 : ws.alloc(g, n, p); };
    auto body = [&](int q0, int gc, double* const* d) {
        return zgbord_group(c, gc, n, p, (psd_z*)d[0], (psd_z*)d[1], o.S.data(), select + (size_t)q0 * n, wantZ,
                            alpha + 2 * (size_t)q0 * n, beta + (size_t)q0 * n, ascale + (size_t)q0 * n, pinfos + q0,
                            nswaps ? nswaps + q0 : nullptr, k.s, ws);
    };
    *info = batch_staged(c, nb, sizeof(double) * (wantZ ? 2 : 1) * nn2 * p + zgbord_ws_bytes(n, p), L, k.s, extra, body);
    if (*info != 0) return *info;
    return *info = batch_first_code(pinfos, nb);
}

}  // extern "C"
