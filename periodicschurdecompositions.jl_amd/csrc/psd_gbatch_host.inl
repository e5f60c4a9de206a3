// Host drivers of the real SIGNED batched entries psd_d_gphessenberg_batch / psd_d_gpschur_batch /
// psd_d_gpschur_batch_dev / psd_d_gpschur_hess_batch: nb Float64 periodic problems of one shape (n, p) and one signature S
// in one call — pschur!(A, S, lr) of rgeneralized.jl:3-45 for each, the path behind gpschur(As, Bs) for real pairs: real
// quasi-triangular T_1, orthogonal Z_l, conjugate pairs as exact conjugates.  Group sizing, staging path and buffers are
// those of psd_batch_host.inl; the workspace, the launch and read-back of the iteration kernel, the fallback loop and the
// bodies of the pschur entries those of psd_zbatch_host.inl, the working signature that of psd_zgbatch_host.inl.
//
//   reduction    stage 1: psd_gbhess1, one workgroup per problem, the whole batch in one launch; stage 2: psd_gbqz with
//                hessmode = 1, one wavefront per problem (psd_gbqz.h)
//   iteration    psd_gbqz with hessmode = 0: one wavefront per problem, from the first decision to the last deflation
//   'L'          psd_breverse_blocks over the whole batch, the signature reversed with the factors
//
// Above the order cap (gb_nmax) the steps are those of the single call — sghess_dev, grun_iteration —, problem by problem
// on the slices of the batch buffer.  A batch of one goes through the same kernels as any other.  An all-true (or NULL)
// signature runs the same signed kernels, as psd_d_gpschur does for it and as pschur!(A, S, lr) does for real element
// types: it is NOT sent to psd_d_pschur_batch, whose outputs (wr, wi, no scaling) have another form.

namespace {

// Largest order of the batched real signed kernels: PSD_GB_NMAX = 128, the cap the other batch kernels start from
// (PSD_BH_NMAX, PSD_ZB_NMAX).  Measured for this path: the sweep of tools/pschur_batch_timing.py --signed-real (nb = 256,
// p = 8, alternating S, n = 8 ... 128) against the loop of single psd_d_gpschur calls — the batched call is ahead at every
// swept order, 52 x in wall time at n = 8 and 23 x at n = 128, the largest swept order, where the two repetitions differ
// by 0.02 % for the loop and 0.15 % for the batch (profiles/batch/README.md).  The cap is the largest swept order at
// which the batched call wins; orders above 128 have not been swept.  (The diagnostic build reads PSD_GB_NMAX from the
// environment: the simulation's tests reach the fallback with it.)
int gb_nmax(const psd_ctx* c) { return c->gb_nmax; }

// the workspace of psd_gbqz for nb problems (zb_work, psd_zbatch_host.inl); behind it the scratch of the 2x2 solvers,
// [nb][16 p + 16] doubles, and the signature S (host, p flags)
using gb_work = zb_work<psd_gbqz_args>;
int gb_work_alloc(psd_ctx* c, gb_work& ws, int nb, int n, int p, int maxlog, const uint8_t* S) {
    const size_t xb = sizeof(double) * (size_t)nb * psd_gbqz_xscr_doubles(p);
    if (int e = ws.alloc(c, nb, n, p, PSD_GTR_CAP, maxlog, xb + (size_t)p)) return e;
    PSD_CHECK(psd_rt_h2d(ws.extra + xb, S, (size_t)p, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));  // (S may be a temporary of the caller)
    ws.A.xscr = (double*)ws.extra;
    ws.A.S = (const unsigned char*)(ws.extra + xb);
    return 0;
}

// what psd_gbqz asks of zb_launch
struct gbqz_signed {
    using args_t = psd_gbqz_args;
    using state_t = psd_gstate;
    static constexpr int esize = 8;
    static constexpr int capk = 8;  // (the slack of giterate_dev's tick loop)
    static constexpr int capw = 5;  // (and the positions it takes off the window)
    static size_t apply_lds(int) { return psd_gbqz_apply_lds_bytes(); }
    static void set_hessmode(args_t& A, int hessmode) { A.hessmode = hessmode; }
    static const void* kernel() { return reinterpret_cast<const void*>(psd_gbqz); }
    static void launch(psd_ctx* c, int nb, size_t lds, const args_t& A) {
        PSD_LAUNCH(psd_gbqz, psd_dim3(nb), PSD_STEP_NT, lds, c->stream, A);
    }
};

// what the kernel left in one problem's state, added to the call's (stats_from_state, summed)
void gbatch_add_state(psd_stats* s, const psd_gstate& st) {
    s->niter += st.jiter;
    s->nsweeps += st.nsweeps;
    s->nrqpass += st.nzshift;
    s->ndefl1 += st.nsplit;
    s->ndefl2 += st.n2real + st.n2cplx;
    s->nwindows += st.nwindows;
    s->nlog += st.nlog;
    s->reserved += st.ncase2 + 1000 * st.ncase3;
}

// _phessenberg!(A, S; wantQ) (generalized.jl:988-1082) for nb problems on the device: dA / dQ [nb][p][n][n] internal
// order (dQ may be null), S (host, internal order, S[0] true).  infos (nb, may be null) receives a per-problem code of
// stage 2 (list overflow or tick bound; the reduction has no other way to fail); the return value is a call-wide code.
int gbhess_dev(psd_ctx* c, int nb, int n, int p, double* dA, double* dQ, const uint8_t* S, int* infos, psd_stats* s) {
    const size_t nn = (size_t)n * n;
    if (infos)
        for (int q = 0; q < nb; ++q) infos[q] = 0;
    if (n > gb_nmax(c)) {
        if (int e = c->reserve(n, p, false, 16)) return e;
        for (int q = 0; q < nb; ++q) {
            psd_stats ps;
            memset(&ps, 0, sizeof(ps));
            const int rc = sghess_dev(c, n, p, dA + (size_t)q * p * nn, dQ ? dQ + (size_t)q * p * nn : nullptr, S, &ps);
            if (rc != 0) return rc;
            s->ms_hess += ps.ms_hess;
            s->ms_formq += ps.ms_formq;
        }
        return 0;
    }
    gb_work ws;
    int rc = gb_work_alloc(c, ws, nb, n, p, 16, S);
    if (rc != 0) return rc;
    Timer t;
    t.start(c->stream);
    PSD_LAUNCH(psd_gbhess1, psd_dim3(nb), PSD_HESS_NT, psd_bhess_lds_bytes(n), c->stream, dA, dQ, ws.A.S, n, p);
    const double ms1 = t.stop(c->stream);
    t.start(c->stream);
    std::vector<psd_gstate> hst;
    std::vector<int> hinfo;
    if ((rc = zb_launch<gbqz_signed>(c, ws, nb, dA, dQ, 1, dQ ? 1 : 0, 1, 1, hst, hinfo)) != 0) return rc;
    const double ms2 = t.stop(c->stream);
    s->ms_hess += ms1 + ms2;
    s->ms_formq += ms1;  // (stage 1 accumulates Q as it goes: the convention of sghess_dev)
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
int gbiterate_dev(psd_ctx* c, int nb, int n, int p, double* dH, double* dZ, const uint8_t* S, int wantT, int wantZ,
                  int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* s) {
    const size_t nn = (size_t)n * n;
    const int W = choose_window(p, 8);
    if (W == 0) return PSD_INFO_NOTIMPL;
    const int maxlog = 2 * maxitfac * n + n + 16;
    if (n > gb_nmax(c)) {
        if (int e = c->reserve(n, p, false, 16)) return e;
        return zb_single_loop(nb, W, infos, s, {PSD_INFO_RUNTIME + 77, PSD_INFO_RUNTIME + 0xfffe}, [&](int q, psd_stats* ps) {
            const int e = grun_iteration(c, n, p, dH + (size_t)q * p * nn, wantZ ? dZ + (size_t)q * p * nn : nullptr, S, wantT,
                                         wantZ, maxitfac, alpha + 2 * (size_t)q * n, beta + (size_t)q * n,
                                         ascale + (size_t)q * n, ps, nullptr, 0);
            return e == PSD_INFO_RUNTIME + 0xfffd ? PSD_INFO_RUNTIME + 0xfffe : e;  // (the tick bound of the single call)
        });
    }
    gb_work ws;
    int rc = gb_work_alloc(c, ws, nb, n, p, maxlog, S);
    if (rc != 0) return rc;
    std::vector<psd_gstate> hst;
    std::vector<int> hinfo;
    rc = zb_launch<gbqz_signed>(c, ws, nb, dH, dZ, wantT, wantZ, maxitfac, 0, hst, hinfo, alpha, beta, ascale);
    if (rc != 0) return rc;
    for (int q = 0; q < nb; ++q) {
        infos[q] = batch_info_code(hinfo[q]);
        gbatch_add_state(s, hst[q]);
    }
    s->nlaunch_step += 1;
    s->window = W;
    return 0;
}

// The whole signed path for nb problems resident on the device: dA / dZ [nb][p][n][n] in user order, S in user order
// (null: all true).  s receives the counters and times of this call.  Per-problem codes go to infos; returns a call-wide
// code or 0.
int gpschur_batch_core(psd_ctx* c, int nb, int n, int p, double* dA, const uint8_t* S, bool left, int wantT, int wantZ,
                       int maxitfac, double* dZ, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* s) {
    memset(s, 0, sizeof(*s));
    if (c->shard_world > 1) return PSD_INFO_NOTIMPL;  // (a period-sharded context keeps a slice of Z: single problems only)
    const std::vector<uint8_t> Sw = S ? zgb_working_sig(S, p, left) : std::vector<uint8_t>(p, 1);
    Timer tall, tph;
    tall.start(c->stream);
    const int rc = batch_reversed(c, left, nb, p, (size_t)n * n, dA, wantZ ? dZ : nullptr, [&]() {
        std::vector<int> hinfos(nb, 0);
        if (int e = gbhess_dev(c, nb, n, p, dA, wantZ ? dZ : nullptr, Sw.data(), hinfos.data(), s)) return e;
        tph.start(c->stream);
        if (int e = gbiterate_dev(c, nb, n, p, dA, dZ, Sw.data(), wantT, wantZ, maxitfac, alpha, beta, ascale, infos, s)) return e;
        s->ms_iter = tph.stop(c->stream);
        for (int q = 0; q < nb; ++q)
            if (hinfos[q] != 0) infos[q] = hinfos[q];  // (a reduction that gave up: what followed is not a decomposition)
        return 0;
    });
    if (rc != 0) return rc;
    s->ms_total = tall.stop(c->stream);
    s->bytes_hess = nb * 2.0 * 8.0 * p * (double)n * n * n;
    PSD_CHECK(psd_rt_last_error());
    return 0;
}

// the real family of the bodies of the pschur entries (zb_complex, psd_zbatch_host.inl): every signature, the all-true
// one included, on the signed kernels
struct gb_real {
    using elem = double;
    static constexpr size_t dpe = 1;
    static int core(psd_ctx* c, int nb, int n, int p, double* dA, const uint8_t* S, bool left, int wantT, int wantZ, int maxitfac,
                    double* dZ, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* s) {
        return gpschur_batch_core(c, nb, n, p, dA, S, left, wantT, wantZ, maxitfac, dZ, alpha, beta, ascale, infos, s);
    }
    static int iterate(psd_ctx* c, int nb, int n, int p, double* dH, double* dZ, const uint8_t* S, int wantT, int wantZ,
                       int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* s) {
        const std::vector<uint8_t> Sw = S ? std::vector<uint8_t>(S, S + p) : std::vector<uint8_t>(p, 1);
        return gbiterate_dev(c, nb, n, p, dH, dZ, Sw.data(), wantT, wantZ, maxitfac, alpha, beta, ascale, infos, s);
    }
};

}  // namespace

extern "C" {

int psd_d_gphessenberg_batch(psd_ctx* c, int nb, int n, int p, double* const* A, const uint8_t* S, double* const* Q,
                             psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    if ((*info = k.head(c, nb, n, p)) != 0) return *info;
    if (!A) return *info = -5;
    if (S && !S[0]) return *info = -7;
    std::vector<uint8_t> Sw(p, 1);
    for (int j = 0; j < p; ++j) Sw[j] = (!S || S[j]) ? 1 : 0;
    const size_t nn = (size_t)n * n;  // doubles of one factor
    const batch_list L[] = {{A, p, nn, BATCH_IN | BATCH_OUT}, {Q, p, nn, BATCH_OUT}};
    auto body = [&](int, int gc, double* const* d) { return gbhess_dev(c, gc, n, p, d[0], d[1], Sw.data(), nullptr, k.s); };
    *info = batch_staged(c, nb, sizeof(double) * ((Q ? 2 : 1) * nn + 2 * (size_t)n) * p, L, k.s, batch_no_extra, body);
    if (*info != 0) return *info;
    PSD_CHECK(psd_rt_last_error());
    k.s->ms_total = k.s->ms_hess;
    k.s->bytes_hess = nb * 2.0 * 8.0 * p * (double)n * n * n;
    return *info = 0;
}

// (the bodies, which take the signature and the family: psd_zbatch_host.inl)
int psd_d_gpschur_batch_dev(psd_ctx* c, int nb, int n, int p, double* dA, const uint8_t* S, char orient, int wantT,
                            int wantZ, int maxitfac, double* dZ, double* alpha, double* beta, int32_t* ascale, int* infos,
                            int* schurindex, psd_stats* stats, int* info) {
    return zb_pschur_batch_dev<gb_real>(c, nb, n, p, dA, S, orient, wantT, wantZ, maxitfac, dZ, alpha, beta, ascale, infos,
                                        schurindex, stats, info);
}

int psd_d_gpschur_batch(psd_ctx* c, int nb, int n, int p, double* const* A, const uint8_t* S, char orient, int wantT,
                        int wantZ, int maxitfac, double* const* Z, double* alpha, double* beta, int32_t* ascale, int* infos,
                        int* schurindex, psd_stats* stats, int* info) {
    return zb_pschur_batch<gb_real>(c, nb, n, p, A, S, orient, wantT, wantZ, maxitfac, Z, alpha, beta, ascale, infos,
                                    schurindex, stats, info);
}

int psd_d_gpschur_hess_batch(psd_ctx* c, int nb, int n, int p, double* const* H, const uint8_t* S, double* const* Q,
                             int wantT, int wantZ, int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos,
                             psd_stats* stats, int* info) {
    return zb_pschur_hess_batch<gb_real>(c, nb, n, p, H, S, Q, wantT, wantZ, maxitfac, alpha, beta, ascale, infos, stats, info,
                                         -11);
}

}  // extern "C"
