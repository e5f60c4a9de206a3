// Host drivers of the complex SIGNED batched entries psd_z_gphessenberg_batch / psd_z_gpschur_batch /
// psd_z_gpschur_batch_dev / psd_z_gpschur_hess_batch: nb ComplexF64 periodic problems of one shape (n, p) and one
// signature S in one call — pschur!(A, S, lr) of generalized.jl:108-148 for each, the path behind gpschur(As, Bs).  Group
// sizing, staging path and buffers are those of psd_batch_host.inl / psd_zbatch_host.inl.
//
//   reduction    stage 1: psd_zgbhess1, one workgroup per problem, the whole batch in one launch; stage 2: psd_zgbqz with
//                hessmode = 1, one wavefront per problem (psd_zgbqz.h)
//   iteration    psd_zgbqz with hessmode = 0: one wavefront per problem, from the first decision to the phase passes
//   'L'          psd_breverse_blocks over the whole batch, the signature reversed with the factors
//
// Above the order cap (zgb_nmax) the steps are those of the single call — zsghess_dev, zgrun_iteration —, problem by
// problem on the slices of the batch buffer.  A batch of one goes through the same kernels as any other.  An all-true
// (or NULL) signature is the business of psd_zbatch_host.inl: the pschur entries forward to it.

namespace {

// Largest order of the batched signed kernels: PSD_ZB_NMAX = 128, the cap of the all-true complex path (psd_zbhess.h),
// reused.  Measured for this path: the sweep of tools/pschur_batch_timing.py --signed (nb = 256, p = 8, alternating S,
// n = 8 ... 128) against the loop of single psd_z_pschur(..., S) calls — the batched call is ahead at every swept order,
// 65 x in wall time at n = 8 and 18 x at n = 128, the largest swept order (profiles/batch/README.md).  Orders above 128
// have not been swept.
int zgb_nmax(const psd_ctx* c) { return c->zb_nmax; }

bool zgb_all_true(const uint8_t* S, int p) {
    if (S)
        for (int j = 0; j < p; ++j)
            if (!S[j]) return false;
    return true;
}

// per-problem workspace of psd_zgbqz for nb problems, carved from one allocation (every region 16-byte aligned)
struct zgb_work {
    psd_batchbuf buf;
    psd_zgbqz_args A;
    int alloc(psd_ctx* c, int nb, int n, int p, int maxlog, const uint8_t* S) {
        size_t off = 0;
        auto carve = [&off](size_t bytes) {
            const size_t o = off;
            off += (bytes + 15) & ~(size_t)15;
            return o;
        };
        const size_t o_st = carve(sizeof(psd_zgstate) * nb), o_desc = carve(sizeof(psd_gapply_desc) * nb);
        const size_t o_tr = carve(sizeof(psd_ztr) * (size_t)nb * p * PSD_GTR_CAP), o_cnt = carve(sizeof(int) * (size_t)nb * p);
        const size_t o_dG = carve(sizeof(psd_ztr) * (size_t)nb * (n + 2)), o_alpha = carve(sizeof(psd_z) * (size_t)nb * n);
        const size_t o_beta = carve(sizeof(double) * (size_t)nb * n), o_asc = carve(sizeof(int) * (size_t)nb * n);
        const size_t o_log = carve(sizeof(int) * (size_t)nb * 3 * maxlog), o_info = carve(sizeof(int) * nb);
        const size_t o_S = carve((size_t)p);
        PSD_CHECK(buf.alloc(off));
        PSD_CHECK(psd_rt_memset(buf.ptr, 0, off, c->stream));
        char* w = (char*)buf.ptr;
        PSD_CHECK(psd_rt_h2d(w + o_S, S, (size_t)p, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));  // (S may be a temporary of the caller)
        A.S = (const unsigned char*)(w + o_S);
        A.st = (psd_zgstate*)(w + o_st);
        A.desc = (psd_gapply_desc*)(w + o_desc);
        A.tr = (psd_ztr*)(w + o_tr);
        A.cnt = (int*)(w + o_cnt);
        A.dG = (psd_ztr*)(w + o_dG);
        A.alpha = (psd_z*)(w + o_alpha);
        A.beta = (double*)(w + o_beta);
        A.ascale = (int*)(w + o_asc);
        A.log = (int*)(w + o_log);
        A.infos = (int*)(w + o_info);
        A.n = n; A.p = p; A.maxlog = maxlog;
        return 0;
    }
};

// one launch of psd_zgbqz over nb problems; the states and per-problem codes (PSD_LIST_OVERFLOW, PSD_ZB_TICKCAP, level)
// come back in hst / hinfo
int zgb_launch(psd_ctx* c, zgb_work& ws, int nb, psd_z* dH, psd_z* dZ, int wantT, int wantZ, int maxitfac, int hessmode,
               std::vector<psd_zgstate>& hst, std::vector<int>& hinfo) {
    psd_zgbqz_args& A = ws.A;
    const int n = A.n, p = A.p;
    const int W = choose_window(p, 16);
    if (W == 0) return PSD_INFO_NOTIMPL;
    A.H = dH;
    A.Z = wantZ ? dZ : nullptr;
    A.wantT = wantT; A.wantZ = wantZ; A.W = W; A.maxitfac = maxitfac; A.hessmode = hessmode;
    const int nbmin = (W - 3 > 0) ? ((W - 3 < 8) ? (W - 3) : 8) : 1;  // (the bound of zgiterate_dev's tick loop)
    A.cap = (long long)maxitfac * n * ((long long)n / nbmin + 8) + 8LL * n + 1024 + (hessmode ? (long long)n * n : 0);
    size_t lds = step_lds_bytes(p, W, 16);
    if (psd_zgbqz_apply_lds_bytes() > lds) lds = psd_zgbqz_apply_lds_bytes();
    PSD_CHECK(c->lds_limit(reinterpret_cast<const void*>(psd_zgbqz), lds));
    PSD_LAUNCH(psd_zgbqz, psd_dim3(nb), PSD_STEP_NT, lds, c->stream, A);
    hst.resize(nb);
    hinfo.resize(nb);
    PSD_CHECK(psd_rt_d2h(hst.data(), A.st, sizeof(psd_zgstate) * nb, c->stream));
    PSD_CHECK(psd_rt_d2h(hinfo.data(), A.infos, sizeof(int) * nb, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    return 0;
}

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
    int rc = ws.alloc(c, nb, n, p, 16, S);
    if (rc != 0) return rc;
    Timer t;
    t.start(c->stream);
    PSD_LAUNCH(psd_zgbhess1, psd_dim3(nb), PSD_HESS_NT, psd_zbhess_lds_bytes(n), c->stream, dA, dQ, ws.A.S, n, p);
    const double ms1 = t.stop(c->stream);
    t.start(c->stream);
    std::vector<psd_zgstate> hst;
    std::vector<int> hinfo;
    if ((rc = zgb_launch(c, ws, nb, dA, dQ, 1, dQ ? 1 : 0, 1, 1, hst, hinfo)) != 0) return rc;
    const double ms2 = t.stop(c->stream);
    s->ms_hess += ms1 + ms2;
    s->ms_formq += ms1;  // (stage 1 accumulates Q as it goes: the convention of zsghess_dev)
    for (int q = 0; q < nb; ++q) {
        const int code = zbatch_info_code(hinfo[q]);
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
        for (int q = 0; q < nb; ++q) {
            psd_stats ps;
            memset(&ps, 0, sizeof(ps));
            int qinfo = 0;
            rc = zgrun_iteration(c, n, p, dH + (size_t)q * p * nn, wantZ ? dZ + (size_t)q * p * nn : nullptr, S, wantT, wantZ,
                                 maxitfac, alpha + 2 * (size_t)q * n, beta + (size_t)q * n, ascale + (size_t)q * n, &ps, &qinfo);
            if (rc == PSD_INFO_RUNTIME + 0xfffc) rc = PSD_INFO_RUNTIME + 0xfffe;  // (the tick bound of the single call)
            if (batch_fatal(rc) && rc != PSD_INFO_RUNTIME + 77 && rc != PSD_INFO_RUNTIME + 0xfffe) return rc;
            infos[q] = rc;
            s->niter += ps.niter;
            s->nsweeps += ps.nsweeps;
            s->nrqpass += ps.nrqpass;
            s->ndefl1 += ps.ndefl1;
            s->ndefl2 += ps.ndefl2;
            s->reserved += ps.reserved;
            s->nwindows += ps.nwindows;
            s->nlog += ps.nlog;
            s->nlaunch_step += ps.nlaunch_step;
        }
        s->window = W;
        return 0;
    }
    zgb_work ws;
    int rc = ws.alloc(c, nb, n, p, maxlog, S);
    if (rc != 0) return rc;
    std::vector<psd_zgstate> hst;
    std::vector<int> hinfo;
    if ((rc = zgb_launch(c, ws, nb, dH, dZ, wantT, wantZ, maxitfac, 0, hst, hinfo)) != 0) return rc;
    std::vector<int> hsc((size_t)nb * n);
    PSD_CHECK(psd_rt_d2h(alpha, ws.A.alpha, sizeof(psd_z) * (size_t)nb * n, c->stream));
    PSD_CHECK(psd_rt_d2h(beta, ws.A.beta, sizeof(double) * (size_t)nb * n, c->stream));
    PSD_CHECK(psd_rt_d2h(hsc.data(), ws.A.ascale, sizeof(int) * (size_t)nb * n, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    for (size_t e = 0; e < (size_t)nb * n; ++e) ascale[e] = hsc[e];
    for (int q = 0; q < nb; ++q) {
        const psd_zgstate& st = hst[q];
        infos[q] = zbatch_info_code(hinfo[q]);
        s->niter += st.jiter;
        s->nsweeps += st.nsweeps;
        s->nrqpass += st.nzshift;
        s->ndefl1 += st.nsplit;
        s->ndefl2 += st.ncase2;
        s->reserved += st.ncase2 + 1000 * st.ncase3;
        s->nwindows += st.nwindows;
        s->nlog += st.nlog;
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
    const size_t nn = (size_t)n * n;
    const std::vector<uint8_t> Sw = zgb_working_sig(S, p, left);
    int rc = 0;
    Timer tall, tph;
    tall.start(c->stream);
    if (left && p > 1)
        PSD_LAUNCH(psd_breverse_blocks, psd_dim3(nb * (p / 2)), PSD_HESS_NT, 0, c->stream, (double*)dA, 2 * nn, p, 0, p);
    std::vector<int> hinfos(nb, 0);
    if ((rc = zgbhess_dev(c, nb, n, p, dA, wantZ ? dZ : nullptr, Sw.data(), hinfos.data(), s)) != 0) return rc;
    tph.start(c->stream);
    if ((rc = zgbiterate_dev(c, nb, n, p, dA, dZ, Sw.data(), wantT, wantZ, maxitfac, alpha, beta, ascale, infos, s)) != 0)
        return rc;
    s->ms_iter = tph.stop(c->stream);
    for (int q = 0; q < nb; ++q)
        if (hinfos[q] != 0) infos[q] = hinfos[q];  // (a reduction that gave up: what followed is not a decomposition)
    if (left && p > 1) {
        PSD_LAUNCH(psd_breverse_blocks, psd_dim3(nb * (p / 2)), PSD_HESS_NT, 0, c->stream, (double*)dA, 2 * nn, p, 0, p);
        if (wantZ && p > 2)
            PSD_LAUNCH(psd_breverse_blocks, psd_dim3(nb * ((p - 1) / 2)), PSD_HESS_NT, 0, c->stream, (double*)dZ, 2 * nn, p, 1,
                       p - 1);
    }
    s->ms_total = tall.stop(c->stream);
    s->bytes_hess = nb * 2.0 * 16.0 * p * (double)n * n * n;
    PSD_CHECK(psd_rt_last_error());
    return 0;
}

}  // namespace

extern "C" {

int psd_z_gphessenberg_batch(psd_ctx* c, int nb, int n, int p, double* const* A, const uint8_t* S, double* const* Q,
                             psd_stats* stats, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c) return *info = -1;
    if (nb < 1) return *info = -2;
    if ((*info = check_dims(n, p)) != 0) return *info = *info - 1;
    if (!A) return *info = -5;
    if (S && !S[0]) return *info = -7;
    std::vector<uint8_t> Sw(p, 1);
    for (int j = 0; j < p; ++j) Sw[j] = (!S || S[j]) ? 1 : 0;
    const size_t nn2 = 2 * (size_t)n * n;  // doubles of one factor
    int g = batch_group(c, nb, sizeof(double) * ((Q ? 2 : 1) * nn2 + 2 * (size_t)n) * p);
    psd_batchbuf dbuf[2];
    psd_hostbuf hst;
    if ((*info = batch_buffers(g, nn2 * p, Q ? 2 : 1, dbuf, hst)) != 0) return *info;
    psd_stats local;
    memset(&local, 0, sizeof(local));
    psd_stats* s = stats ? stats : &local;
    Timer tc;
    for (int q0 = 0; q0 < nb; q0 += g) {
        const int gc = (nb - q0 < g) ? (nb - q0) : g;
        tc.start(c->stream);
        if ((*info = batch_upload(c, A, q0, gc, p, nn2, hst.d(), dbuf[0].d())) != 0) return *info;
        s->ms_copy += tc.stop(c->stream);
        if ((*info = zgbhess_dev(c, gc, n, p, (psd_z*)dbuf[0].ptr, Q ? (psd_z*)dbuf[1].ptr : nullptr, Sw.data(), nullptr, s)) != 0)
            return *info;
        tc.start(c->stream);
        if ((*info = batch_download(c, A, q0, gc, p, nn2, hst.d(), dbuf[0].d())) != 0) return *info;
        if (Q && (*info = batch_download(c, Q, q0, gc, p, nn2, hst.d(), dbuf[1].d())) != 0) return *info;
        s->ms_copy += tc.stop(c->stream);
    }
    PSD_CHECK(psd_rt_last_error());
    s->ms_total = s->ms_hess;
    s->bytes_hess = nb * 2.0 * 16.0 * p * (double)n * n * n;
    return *info = 0;
}

int psd_z_gpschur_batch_dev(psd_ctx* c, int nb, int n, int p, double* dA, const uint8_t* S, char orient, int wantT,
                            int wantZ, int maxitfac, double* dZ, double* alpha, double* beta, int32_t* ascale, int* infos,
                            int* schurindex, psd_stats* stats, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c) return *info = -1;
    if (nb < 1) return *info = -2;
    if ((*info = check_dims(n, p)) != 0) return *info = *info - 1;
    if (!dA) return *info = -5;
    if (orient != 'R' && orient != 'L') return *info = -6;  // PSD.jl:175-177
    if (S && !S[(orient == 'L') ? p - 1 : 0]) return *info = -7;  // generalized.jl:140
    if (maxitfac < 1) return *info = -9;
    if (wantZ && !dZ) return *info = -10;
    if (!alpha || !beta || !ascale) return *info = -11;
    if (zgb_all_true(S, p))  // (the tuned all-true path, as psd_z_pschur keeps it)
        return psd_z_pschur_batch_dev(c, nb, n, p, dA, orient, wantT, wantZ, maxitfac, dZ, alpha, beta, ascale, infos,
                                      schurindex, stats, info);
    psd_stats local;
    psd_stats* s = stats ? stats : &local;
    std::vector<int> linfo(infos ? 0 : nb, 0);
    int* pinfos = infos ? infos : linfo.data();
    const int rc = zgpschur_batch_core(c, nb, n, p, reinterpret_cast<psd_z*>(dA), S, orient == 'L', wantT, wantZ, maxitfac,
                                       reinterpret_cast<psd_z*>(dZ), alpha, beta, ascale, pinfos, s);
    if (schurindex) *schurindex = (orient == 'L') ? p : 1;
    return *info = (rc != 0) ? rc : zbatch_worst(pinfos, nb);
}

int psd_z_gpschur_batch(psd_ctx* c, int nb, int n, int p, double* const* A, const uint8_t* S, char orient, int wantT,
                        int wantZ, int maxitfac, double* const* Z, double* alpha, double* beta, int32_t* ascale, int* infos,
                        int* schurindex, psd_stats* stats, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c) return *info = -1;
    if (nb < 1) return *info = -2;
    if ((*info = check_dims(n, p)) != 0) return *info = *info - 1;
    if (!A) return *info = -5;
    if (orient != 'R' && orient != 'L') return *info = -6;
    if (S && !S[(orient == 'L') ? p - 1 : 0]) return *info = -7;
    if (maxitfac < 1) return *info = -9;
    if (wantZ && !Z) return *info = -10;
    if (!alpha || !beta || !ascale) return *info = -11;
    if (zgb_all_true(S, p))
        return psd_z_pschur_batch(c, nb, n, p, A, orient, wantT, wantZ, maxitfac, Z, alpha, beta, ascale, infos, schurindex,
                                  stats, info);
    const size_t nn2 = 2 * (size_t)n * n;
    int g = batch_group(c, nb, sizeof(double) * ((wantZ ? 2 : 1) * nn2 + 2 * (size_t)n) * p);
    psd_batchbuf dbuf[2];
    psd_hostbuf hst;
    if ((*info = batch_buffers(g, nn2 * p, wantZ ? 2 : 1, dbuf, hst)) != 0) return *info;
    psd_stats local;
    memset(&local, 0, sizeof(local));
    psd_stats* s = stats ? stats : &local;
    std::vector<int> linfo(infos ? 0 : nb, 0);
    int* pinfos = infos ? infos : linfo.data();
    Timer tc;
    for (int q0 = 0; q0 < nb; q0 += g) {
        const int gc = (nb - q0 < g) ? (nb - q0) : g;
        psd_stats gs;
        tc.start(c->stream);
        if ((*info = batch_upload(c, A, q0, gc, p, nn2, hst.d(), dbuf[0].d())) != 0) return *info;
        double ms_copy = tc.stop(c->stream);
        const int rc = zgpschur_batch_core(c, gc, n, p, (psd_z*)dbuf[0].ptr, S, orient == 'L', wantT, wantZ, maxitfac,
                                           (psd_z*)dbuf[1].ptr, alpha + 2 * (size_t)q0 * n, beta + (size_t)q0 * n,
                                           ascale + (size_t)q0 * n, pinfos + q0, &gs);
        if (rc != 0) return *info = rc;
        tc.start(c->stream);
        if ((*info = batch_download(c, A, q0, gc, p, nn2, hst.d(), dbuf[0].d())) != 0) return *info;
        if (wantZ && (*info = batch_download(c, Z, q0, gc, p, nn2, hst.d(), dbuf[1].d())) != 0) return *info;
        ms_copy += tc.stop(c->stream);
        batch_add_stats(s, gs);
        s->nlog += gs.nlog;
        s->ms_copy += ms_copy;
    }
    if (schurindex) *schurindex = (orient == 'L') ? p : 1;
    return *info = zbatch_worst(pinfos, nb);
}

int psd_z_gpschur_hess_batch(psd_ctx* c, int nb, int n, int p, double* const* H, const uint8_t* S, double* const* Q,
                             int wantT, int wantZ, int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos,
                             psd_stats* stats, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c) return *info = -1;
    if (nb < 1) return *info = -2;
    if ((*info = check_dims(n, p)) != 0) return *info = *info - 1;
    if (!H) return *info = -5;
    if (wantZ && !Q) return *info = -6;
    if (S && !S[0]) return *info = -7;
    if (maxitfac < 1) return *info = -9;
    if (!alpha || !beta || !ascale) return *info = -11;
    if (zgb_all_true(S, p))
        return psd_z_pschur_hess_batch(c, nb, n, p, H, Q, wantT, wantZ, maxitfac, alpha, beta, ascale, infos, stats, info);
    if (c->shard_world > 1) return *info = PSD_INFO_NOTIMPL;
    const size_t nn2 = 2 * (size_t)n * n;
    int g = batch_group(c, nb, sizeof(double) * ((wantZ ? 2 : 1) * nn2 + 2 * (size_t)n) * p);
    psd_batchbuf dbuf[2];
    psd_hostbuf hst;
    if ((*info = batch_buffers(g, nn2 * p, wantZ ? 2 : 1, dbuf, hst)) != 0) return *info;
    psd_stats local;
    memset(&local, 0, sizeof(local));
    psd_stats* s = stats ? stats : &local;
    std::vector<int> linfo(infos ? 0 : nb, 0);
    int* pinfos = infos ? infos : linfo.data();
    Timer tc, tk;
    for (int q0 = 0; q0 < nb; q0 += g) {
        const int gc = (nb - q0 < g) ? (nb - q0) : g;
        tc.start(c->stream);
        if ((*info = batch_upload(c, H, q0, gc, p, nn2, hst.d(), dbuf[0].d())) != 0) return *info;
        if (wantZ && (*info = batch_upload(c, Q, q0, gc, p, nn2, hst.d(), dbuf[1].d())) != 0) return *info;
        s->ms_copy += tc.stop(c->stream);
        tk.start(c->stream);
        const int rc = zgbiterate_dev(c, gc, n, p, (psd_z*)dbuf[0].ptr, (psd_z*)dbuf[1].ptr, S, wantT, wantZ, maxitfac,
                                      alpha + 2 * (size_t)q0 * n, beta + (size_t)q0 * n, ascale + (size_t)q0 * n, pinfos + q0, s);
        if (rc != 0) return *info = rc;
        s->ms_iter += tk.stop(c->stream);
        tc.start(c->stream);
        if ((*info = batch_download(c, H, q0, gc, p, nn2, hst.d(), dbuf[0].d())) != 0) return *info;
        if (wantZ && (*info = batch_download(c, Q, q0, gc, p, nn2, hst.d(), dbuf[1].d())) != 0) return *info;
        s->ms_copy += tc.stop(c->stream);
    }
    s->ms_total = s->ms_iter;
    return *info = zbatch_worst(pinfos, nb);
}

}  // extern "C"
