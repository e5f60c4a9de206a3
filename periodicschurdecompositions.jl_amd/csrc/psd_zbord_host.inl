// Host drivers of psd_z_ordschur_batch / psd_z_ordschur_batch_dev (psd_zbord.h): ordschur!(P, select) for nb ComplexF64
// periodic Schur forms of one shape, as psd_z_pschur_batch leaves them.  Included at the end of psd_engine.cpp behind
// psd_bord_host.inl, whose argument checks, slot permutations and group loop it shares (a complex matrix travels as
// 2 n^2 doubles).
//
// Per group of problems: the selections go up once, then psd_zbord — every problem's whole reordering in one launch —
// and psd_zbord_values, and one read-back of the per-problem states, codes and scaled eigenvalues.  Orders above
// PSD_BORD_NMAX, and periods whose narrowest window does not fit the LDS, run zordschur_dev problem by problem on the
// slices of the batch buffers.

namespace {

// Window of the batched kernel: zordschur_dev's choice, narrowed to the smallest candidate that still holds the whole
// problem when one does (the windows stay the same ones — a window never reaches above row 1 — and less LDS per
// workgroup lets more problems share a CU); 0: none fits.  PSD_BORD_W narrows it further.
int zbord_window(const psd_ctx* c, int n, int p) {
    int W = choose_window_lds({32, 24, 20, 16, 12, 10, 8, 6, 4}, [&](int w) { return ord_lds_bytes(p, w); }, n);
    if (W != 0 && c->bord_w >= PSD_ZBORD_WMIN && c->bord_w < W) W = c->bord_w;
    return W;
}

size_t zbord_lds_bytes(int p, int W) {
    const size_t a = ord_lds_bytes(p, W), b = psd_zbqz_apply_lds_bytes(W);
    return a > b ? a : b;
}

// device workspace of one problem besides its factors
size_t zbord_ws_bytes(int n, int p) {
    return sizeof(psd_ostate) + sizeof(psd_zapply_desc) + sizeof(psd_ztr) * (size_t)p * PSD_ZTR_CAP + sizeof(int) * (size_t)(p + 1) +
           (size_t)n + (sizeof(psd_z) + sizeof(double) + sizeof(int)) * (size_t)n;
}

struct zbord_ws {
    psd_batchbuf st, desc, tr, cnt, sel, alpha, beta, ascale, infos;
    int alloc(int g, int n, int p) {
        PSD_CHECK(st.alloc(sizeof(psd_ostate) * (size_t)g));
        PSD_CHECK(desc.alloc(sizeof(psd_zapply_desc) * (size_t)g));
        PSD_CHECK(tr.alloc(sizeof(psd_ztr) * (size_t)g * p * PSD_ZTR_CAP));
        PSD_CHECK(cnt.alloc(sizeof(int) * (size_t)g * p));
        PSD_CHECK(sel.alloc((size_t)g * n));
        PSD_CHECK(alpha.alloc(sizeof(psd_z) * (size_t)g * n));
        PSD_CHECK(beta.alloc(sizeof(double) * (size_t)g * n));
        PSD_CHECK(ascale.alloc(sizeof(int) * (size_t)g * n));
        PSD_CHECK(infos.alloc(sizeof(int) * (size_t)g));
        return 0;
    }
};

bool zbord_fallback(const psd_ctx* c, int n, int p) { return n > c->bord_nmax || zbord_window(c, n, p) == 0; }

// gc problems resident on the device in the internal order (dH, dZ [gc][p][n][n]); select, alpha (pairs), beta, ascale,
// infos, nswaps: the host rows of these problems.  The rows of a problem whose code is non-zero are not written.  Adds
// to s.
int zbord_group(psd_ctx* c, int gc, int n, int p, psd_z* dH, psd_z* dZ, const uint8_t* select, int wantZ, double* alpha,
                double* beta, int32_t* ascale, int* infos, int* nswaps, psd_stats* s, zbord_ws& ws) {
    const size_t nn = (size_t)n * n;
    if (zbord_fallback(c, n, p)) {
        int rc = c->zreserve(n, p, false, 16);
        if (rc != 0) return rc;
        for (int q = 0; q < gc; ++q) {
            psd_stats ps;
            memset(&ps, 0, sizeof(ps));
            int pinfo = 0;
            // (the eigenvalues come down only behind a run that ended with code 0)
            rc = zordschur_dev(c, n, p, dH + (size_t)q * p * nn, wantZ ? dZ + (size_t)q * p * nn : nullptr,
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
    const int W = zbord_window(c, n, p);
    const size_t lds = zbord_lds_bytes(p, W);
    PSD_CHECK(c->lds_limit(reinterpret_cast<const void*>(psd_zbord), lds));
    PSD_CHECK(psd_rt_h2d(ws.sel.ptr, select, (size_t)gc * n, c->stream));
    psd_zbord_args a;
    a.H = dH;
    a.Z = wantZ ? dZ : nullptr;
    a.st = (psd_ostate*)ws.st.ptr;
    a.desc = (psd_zapply_desc*)ws.desc.ptr;
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
    PSD_LAUNCH(psd_zbord, psd_dim3(gc), PSD_STEP_NT, lds, c->stream, a);
    PSD_LAUNCH(psd_zbord_values, psd_dim3((n + 63) / 64, gc), 64, 0, c->stream, a);
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
        if (hst[q].info == PSD_ZBORD_WINCAP) return PSD_INFO_RUNTIME + 0xfffd;  // (zordschur_dev's code of a run that does not end)
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

// the argument codes of the real entries (bord_checked); -9: alpha, beta or ascale missing
int zbord_checked(psd_ctx* c, int nb, int n, int p, const void* T, const void* Z, char orient, int schurindex,
                  const uint8_t* select, int wantZ, const double* alpha, const double* beta, const int32_t* ascale,
                  std::vector<int>& slotA, std::vector<int>& slotZ) {
    const double* vals = (alpha && beta && ascale) ? alpha : nullptr;
    return bord_checked(c, nb, n, p, T, Z, orient, schurindex, select, wantZ, vals, vals, slotA, slotZ);
}

}  // namespace

extern "C" {

int psd_z_ordschur_batch_dev(psd_ctx* c, int nb, int n, int p, void* dT, void* dZ, char orient, int schurindex,
                             const uint8_t* select, int wantZ, double* alpha, double* beta, int32_t* ascale, int* infos,
                             int* nswaps, psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    std::vector<int> slotA, slotZ;
    if ((*info = zbord_checked(c, nb, n, p, dT, dZ, orient, schurindex, select, wantZ, alpha, beta, ascale, slotA, slotZ)) != 0 ||
        nb == 0)
        return *info;
    const size_t nn = (size_t)n * n;
    int* pinfos = k.infos(infos, nb);
    psd_z* H = (psd_z*)dT;
    psd_z* Z = wantZ ? (psd_z*)dZ : nullptr;
    zbord_ws ws;
    auto group = [&](int q0, int gc) {
        return zbord_group(c, gc, n, p, H + (size_t)q0 * p * nn, Z ? Z + (size_t)q0 * p * nn : nullptr, select + (size_t)q0 * n,
                           wantZ, alpha + 2 * (size_t)q0 * n, beta + (size_t)q0 * n, ascale + (size_t)q0 * n, pinfos + q0,
                           nswaps ? nswaps + q0 : nullptr, k.s, ws);
    };
    return *info = bord_dev_run(c, nb, n, p, 2 * nn, (double*)H, (double*)Z, slotA, slotZ, zbord_fallback(c, n, p),
                                zbord_ws_bytes(n, p), ws, pinfos, group);
}

int psd_z_ordschur_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, char orient, int schurindex,
                         const uint8_t* select, int wantZ, double* alpha, double* beta, int32_t* ascale, int* infos,
                         int* nswaps, psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    std::vector<int> slotA, slotZ;
    if ((*info = zbord_checked(c, nb, n, p, T, Z, orient, schurindex, select, wantZ, alpha, beta, ascale, slotA, slotZ)) != 0 ||
        nb == 0)
        return *info;
    const size_t nn2 = 2 * (size_t)n * n;  // doubles of one factor
    // user slot <-> internal slot on the way through the staging buffer, as psd_z_ordschur copies
    const batch_list L[] = {{T, p, nn2, BATCH_IN | BATCH_OUT, slotA.data()},
                            {wantZ ? Z : nullptr, p, nn2, BATCH_IN | BATCH_OUT, slotZ.data()}};
    int* pinfos = k.infos(infos, nb);
    zbord_ws ws;
    auto extra = [&](int g) { return zbord_fallback(c, n, p) ? 0 : ws.alloc(g, n, p); };
    auto body = [&](int q0, int gc, double* const* d) {
        return zbord_group(c, gc, n, p, (psd_z*)d[0], (psd_z*)d[1], select + (size_t)q0 * n, wantZ, alpha + 2 * (size_t)q0 * n,
                           beta + (size_t)q0 * n, ascale + (size_t)q0 * n, pinfos + q0, nswaps ? nswaps + q0 : nullptr, k.s, ws);
    };
    *info = batch_staged(c, nb, sizeof(double) * (wantZ ? 2 : 1) * nn2 * p + zbord_ws_bytes(n, p), L, k.s, extra, body);
    if (*info != 0) return *info;
    return *info = batch_first_code(pinfos, nb);
}

}  // extern "C"
