// Host drivers of the complex SIGNED batched entries psd_z_gphessenberg_batch / psd_z_gpschur_batch /
// psd_z_gpschur_batch_dev / psd_z_gpschur_hess_batch: nb ComplexF64 periodic problems of one shape (n, p) and one
// signature S in one call — pschur!(A, S, lr) of generalized.jl:108-148 for each, the path behind gpschur(As, Bs).  Group
// sizing, staging path and buffers are those of psd_batch_host.inl; the workspace, the launch and read-back of the
// iteration kernel, the fallback loop and the bodies of the pschur entries those of psd_zbatch_host.inl.
//
//   reduction    stage 1: psd_zgbhess1, one workgroup per problem, the whole batch in one launch; stage 2: psd_zgbqz with
//                hessmode = 1, one wavefront per problem (psd_zgbqz.h)
//   iteration    psd_zgbqz with hessmode = 0: one wavefront per problem, from the first decision to the phase passes
//   'L'          psd_breverse_blocks over the whole batch, the signature reversed with the factors
//
// Above the order cap (zgb_nmax) the steps are those of the single call — zsghess_dev, zgrun_iteration —, problem by
// problem on the slices of the batch buffer.  A batch of one goes through the same kernels as any other.  An all-true
// (or NULL) signature is the business of psd_zbatch_host.inl: the bodies of the pschur entries take its path.

namespace {

// Largest order of the batched signed kernels: PSD_ZB_NMAX = 128, the cap of the all-true complex path (psd_zbhess.h),
// reused.  Measured for this path: the sweep of tools/pschur_batch_timing.py --signed (nb = 256, p = 8, alternating S,
// n = 8 ... 128) against the loop of single psd_z_pschur(..., S) calls — the batched call is ahead at every swept order,
// 65 x in wall time at n = 8 and 18 x at n = 128, the largest swept order (profiles/batch/README.md).  Orders above 128
// have not been swept.
int zgb_nmax(const psd_ctx* c) { return c->zb_nmax; }

// the workspace of psd_zgbqz for nb problems (zb_work, psd_zbatch_host.inl) with the signature S (host, p flags) behind it
using zgb_work = zb_work<psd_zgbqz_args>;
int zgb_work_alloc(psd_ctx* c, zgb_work& ws, int nb, int n, int p, int maxlog, const uint8_t* S) {
    if (int e = ws.alloc(c, nb, n, p, PSD_GTR_CAP, maxlog, (size_t)p)) return e;
    PSD_CHECK(psd_rt_h2d(ws.extra, S, (size_t)p, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));  // (S may be a temporary of the caller)
    ws.A.S = (const unsigned char*)ws.extra;
    return 0;
}

// what psd_zgbqz asks of zb_launch
struct zgbqz_signed {
    using args_t = psd_zgbqz_args;
    using state_t = psd_zgstate;
    static constexpr int esize = 16;
    static constexpr int capk = 8;  // (the slack of zgiterate_dev's tick loop)
    static constexpr int capw = 3;
    static size_t apply_lds(int) { return psd_zgbqz_apply_lds_bytes(); }
    static void set_hessmode(args_t& A, int hessmode) { A.hessmode = hessmode; }
    static const void* kernel() { return reinterpret_cast<const void*>(psd_zgbqz); }
    static void launch(psd_ctx* c, int nb, size_t lds, const args_t& A) {
        PSD_LAUNCH(psd_zgbqz, psd_dim3(nb), PSD_STEP_NT, lds, c->stream, A);
    }
};

// _phessenberg!(A, S; wantQ) (generalized.jl:988-1082) for nb problems on the device: dA / dQ [nb][p][n][n] internal
// order (dQ may be null), S (host, internal order, S[0] true).  infos (nb, may be null) receives a per-problem code of
// stage 2 (list overflow or tick bound; the reduction has no other way to fail); the return value is a call-wide code.
int zgbhess_dev(psd_ctx* c, int nb, int n, int p, psd_z* dA, psd_z* dQ, const uint8_t* S, int* infos, psd_stats* s) {
    const size_t nn = (size_t)n * n;
    if (infos)
        for (int q = 0; q < nb; ++q) infos[q] = 0;
    if (n > zgb_nmax(c)) {
        int rc = c->zreserve(n, p, false, 16);
        if (rc == 0) rc = c->zgreserve(n, p);
        if (rc != 0) return rc;
        for (int q = 0; q < nb; ++q) {
            psd_stats ps;
            memset(&ps, 0, sizeof(ps));
            rc = zsghess_dev(c, n, p, dA + (size_t)q * p * nn, dQ ? dQ + (size_t)q * p * nn : nullptr, S, &ps);
            if (rc != 0) return rc;
            s->ms_hess += ps.ms_hess;
            s->ms_formq += ps.ms_formq;
        }
        return 0;
    }
    zgb_work ws;
    int rc = zgb_work_alloc(c, ws, nb, n, p, 16, S);
    if (rc != 0) return rc;
    Timer t;
    t.start(c->stream);
    PSD_LAUNCH(psd_zgbhess1, psd_dim3(nb), PSD_HESS_NT, psd_zbhess_lds_bytes(n), c->stream, dA, dQ, ws.A.S, n, p);
    const double ms1 = t.stop(c->stream);
    t.start(c->stream);
    std::vector<psd_zgstate> hst;
    std::vector<int> hinfo;
    if ((rc = zb_launch<zgbqz_signed>(c, ws, nb, dA, dQ, 1, dQ ? 1 : 0, 1, 1, hst, hinfo)) != 0) return rc;
    const double ms2 = t.stop(c->stream);
    s->ms_hess += ms1 + ms2;
    s->ms_formq += ms1;  // (stage 1 accumulates Q as it goes: the convention of zsghess_dev)
    for (int q = 0; q < nb; ++q) {
        const int code = batch_info_code(hinfo[q]);
        if (infos) infos[q] = code;
        else if (code != 0) return code;
    }
    return 0;
}

// The signed iteration for nb Hessenberg-triangular problems on the device: dH / dZ [nb][p][n][n] internal order (dZ holds
// the Q_j on entry), S (host, internal order).  alpha (nb * n complex pairs), beta, ascale (nb * n), infos (nb): host.
// Per-problem codes go to infos; the return value is a call-wide (runtime / not-implemented) code or 0.
int zgbiterate_dev(psd_ctx* c, int nb, int n, int p, psd_z* dH, psd_z* dZ, const uint8_t* S, int wantT, int wantZ,
                   int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* s) {
    const size_t nn = (size_t)n * n;
    const int W = choose_window(p, 16);
    if (W == 0) return PSD_INFO_NOTIMPL;
    const int maxlog = 2 * maxitfac * n + n + 16;
    if (n > zgb_nmax(c)) {
        int rc = c->zreserve(n, p, false, maxlog);
        if (rc == 0) rc = c->zgreserve(n, p);
        if (rc != 0) return rc;
        // (the counts, not maxits: the single signed call keeps its train sweeps there)
        return zb_single_loop(nb, W, infos, s, {PSD_INFO_RUNTIME + 77, PSD_INFO_RUNTIME + 0xfffe}, [&](int q, psd_stats* ps) {
            const int e = zgrun_iteration(c, n, p, dH + (size_t)q * p * nn, wantZ ? dZ + (size_t)q * p * nn : nullptr, S, wantT,
                                          wantZ, maxitfac, alpha + 2 * (size_t)q * n, beta + (size_t)q * n,
                                          ascale + (size_t)q * n, ps);
            return e == PSD_INFO_RUNTIME + 0xfffc ? PSD_INFO_RUNTIME + 0xfffe : e;  // (the tick bound of the single call)
        });
    }
    zgb_work ws;
    int rc = zgb_work_alloc(c, ws, nb, n, p, maxlog, S);
    if (rc != 0) return rc;
    std::vector<psd_zgstate> hst;
    std::vector<int> hinfo;
    rc = zb_launch<zgbqz_signed>(c, ws, nb, dH, dZ, wantT, wantZ, maxitfac, 0, hst, hinfo, alpha, beta, ascale);
    if (rc != 0) return rc;
    for (int q = 0; q < nb; ++q) {
        infos[q] = batch_info_code(hinfo[q]);
        zbatch_add_state(s, hst[q]);
        s->reserved += hst[q].ncase2 + 1000 * hst[q].ncase3;
    }
    s->nlaunch_step += 1;
    s->window = W;
    return 0;
}

// the signature in working order: reversed with the factors for 'L' (generalized.jl:910-927, as zsigned_pschur_host)
std::vector<uint8_t> zgb_working_sig(const uint8_t* S, int p, bool left) {
    std::vector<int> sA, sZ;
    ord_slots(left ? 'L' : 'R', left ? p : 1, p, sA, sZ);
    std::vector<uint8_t> w(p, 1);
    for (int j = 0; j < p; ++j) w[j] = S[sA[j]] ? 1 : 0;
    return w;
}

// The whole signed path for nb problems resident on the device: dA / dZ [nb][p][n][n] in user order, S in user order.
// s receives the counters and times of this call.  Per-problem codes go to infos; returns a call-wide code or 0.
int zgpschur_batch_core(psd_ctx* c, int nb, int n, int p, psd_z* dA, const uint8_t* S, bool left, int wantT, int wantZ,
                        int maxitfac, psd_z* dZ, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* s) {
    memset(s, 0, sizeof(*s));
    if (c->shard_world > 1) return PSD_INFO_NOTIMPL;  // (a period-sharded context keeps a slice of Z: single problems only)
    const std::vector<uint8_t> Sw = zgb_working_sig(S, p, left);
    Timer tall, tph;
    tall.start(c->stream);
    const int rc = batch_reversed(c, left, nb, p, 2 * (size_t)n * n, (double*)dA, wantZ ? (double*)dZ : nullptr, [&]() {
        std::vector<int> hinfos(nb, 0);
        if (int e = zgbhess_dev(c, nb, n, p, dA, wantZ ? dZ : nullptr, Sw.data(), hinfos.data(), s)) return e;
        tph.start(c->stream);
        if (int e = zgbiterate_dev(c, nb, n, p, dA, dZ, Sw.data(), wantT, wantZ, maxitfac, alpha, beta, ascale, infos, s)) return e;
        s->ms_iter = tph.stop(c->stream);
        for (int q = 0; q < nb; ++q)
            if (hinfos[q] != 0) infos[q] = hinfos[q];  // (a reduction that gave up: what followed is not a decomposition)
        return 0;
    });
    if (rc != 0) return rc;
    s->ms_total = tall.stop(c->stream);
    s->bytes_hess = nb * 2.0 * 16.0 * p * (double)n * n * n;
    PSD_CHECK(psd_rt_last_error());
    return 0;
}

}  // namespace

extern "C" {

int psd_z_gphessenberg_batch(psd_ctx* c, int nb, int n, int p, double* const* A, const uint8_t* S, double* const* Q,
                             psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    if ((*info = k.head(c, nb, n, p)) != 0) return *info;
    if (!A) return *info = -5;
    if (S && !S[0]) return *info = -7;
    std::vector<uint8_t> Sw(p, 1);
    for (int j = 0; j < p; ++j) Sw[j] = (!S || S[j]) ? 1 : 0;
    const size_t nn2 = 2 * (size_t)n * n;  // doubles of one factor
    const batch_list L[] = {{A, p, nn2, BATCH_IN | BATCH_OUT}, {Q, p, nn2, BATCH_OUT}};
    auto body = [&](int, int gc, double* const* d) {
        return zgbhess_dev(c, gc, n, p, (psd_z*)d[0], (psd_z*)d[1], Sw.data(), nullptr, k.s);
    };
    *info = batch_staged(c, nb, sizeof(double) * ((Q ? 2 : 1) * nn2 + 2 * (size_t)n) * p, L, k.s, batch_no_extra, body);
    if (*info != 0) return *info;
    PSD_CHECK(psd_rt_last_error());
    k.s->ms_total = k.s->ms_hess;
    k.s->bytes_hess = nb * 2.0 * 16.0 * p * (double)n * n * n;
    return *info = 0;
}

// (the bodies, which take the signature: psd_zbatch_host.inl)
int psd_z_gpschur_batch_dev(psd_ctx* c, int nb, int n, int p, double* dA, const uint8_t* S, char orient, int wantT,
                            int wantZ, int maxitfac, double* dZ, double* alpha, double* beta, int32_t* ascale, int* infos,
                            int* schurindex, psd_stats* stats, int* info) {
    return zb_pschur_batch_dev(c, nb, n, p, dA, S, orient, wantT, wantZ, maxitfac, dZ, alpha, beta, ascale, infos, schurindex,
                               stats, info);
}

int psd_z_gpschur_batch(psd_ctx* c, int nb, int n, int p, double* const* A, const uint8_t* S, char orient, int wantT,
                        int wantZ, int maxitfac, double* const* Z, double* alpha, double* beta, int32_t* ascale, int* infos,
                        int* schurindex, psd_stats* stats, int* info) {
    return zb_pschur_batch(c, nb, n, p, A, S, orient, wantT, wantZ, maxitfac, Z, alpha, beta, ascale, infos, schurindex, stats,
                           info);
}

int psd_z_gpschur_hess_batch(psd_ctx* c, int nb, int n, int p, double* const* H, const uint8_t* S, double* const* Q,
                             int wantT, int wantZ, int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos,
                             psd_stats* stats, int* info) {
    return zb_pschur_hess_batch(c, nb, n, p, H, S, Q, wantT, wantZ, maxitfac, alpha, beta, ascale, infos, stats, info, -11);
}

}  // extern "C"
