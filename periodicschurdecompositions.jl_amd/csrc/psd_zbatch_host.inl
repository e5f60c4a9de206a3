// Host drivers of the complex batched entries psd_z_phessenberg_batch / psd_z_pschur_batch / psd_z_pschur_batch_dev /
// psd_z_pschur_hess_batch: nb ComplexF64 periodic problems of one shape (n, p) in one call, all signatures +1 — the
// complex counterpart of psd_batch_host.inl, whose group sizing, staging path and buffers it uses as they are (a complex
// matrix travels as 2 n^2 doubles).
//
//   reduction    psd_zbhess: one workgroup per problem, the whole batch in one launch (psd_zbhess.h)
//   Q formation  psd_zbformq: one workgroup per (problem, factor); psd_zbtriu
//   iteration    psd_zbqz: one wavefront per problem, from the first decision to the phase passes in one launch
//                (psd_zbqz.h)
//   'L'          psd_breverse_blocks over the whole batch, as the real driver
//
// Above PSD_ZB_NMAX the three steps are those of the single call — zhessenberg_dev, zformq_dev, ziterate_dev —, problem
// by problem on the slices of the batch buffer.  A batch of one goes through the same kernels as any other.

namespace {

// generalized.jl:988-1082 with S all true (= PSD.jl:213-259) for nb problems: dH [nb][p][n][n], dtau [nb][p][n]
int zbhessenberg_dev(psd_ctx* c, int nb, int n, int p, psd_z* dH, psd_z* dtau) {
    const size_t nn = (size_t)n * n;
    if (n <= c->zb_nmax) {
        PSD_CHECK(psd_rt_memset(dtau, 0, sizeof(psd_z) * (size_t)nb * p * n, c->stream));
        if (n < 2) return 0;
        PSD_LAUNCH(psd_zbhess, psd_dim3(nb), PSD_HESS_NT, psd_zbhess_lds_bytes(n), c->stream, dH, dtau, n, p);
        return 0;
    }
    for (int q = 0; q < nb; ++q) {
        const int rc = zhessenberg_dev(c, n, p, dH + (size_t)q * p * nn, dtau + (size_t)q * p * n);
        if (rc != 0) return rc;
    }
    return 0;
}

// Q_j of every problem (dQ may be null: the factors alone), then the clean-up of the reflector storage
int zbformq_dev(psd_ctx* c, int nb, int n, int p, psd_z* dH, const psd_z* dtau, psd_z* dQ) {
    const size_t nn = (size_t)n * n;
    if (dQ) {
        if (n <= c->zb_nmax) {
            PSD_LAUNCH(psd_zbformq, psd_dim3(nb * p), PSD_HESS_NT, PSD_HESS_NT * sizeof(psd_z), c->stream,
                       (const psd_z*)dH, dtau, dQ, n, p);
        } else {
            for (int q = 0; q < nb; ++q) {
                const int rc = zformq_dev(c, n, p, dH + (size_t)q * p * nn, dtau + (size_t)q * p * n, dQ + (size_t)q * p * nn);
                if (rc != 0) return rc;
            }
        }
    }
    PSD_LAUNCH(psd_zbtriu, psd_dim3(nb * p), PSD_HESS_NT, 0, c->stream, dH, n, p);
    return 0;
}


// Per-problem workspace of psd_zbqz / psd_zgbqz (Args: their argument struct) for nb problems, carved from one zeroed
// allocation, every region 16-byte aligned; `extra` bytes follow the per-problem arrays (the signed kernel's signature).
// alloc fills the workspace pointers and n, p, maxlog of A.
template <class Args>
struct zb_work {
    psd_batchbuf buf;
    Args A;
    char* extra = nullptr;
    int alloc(psd_ctx* c, int nb, int n, int p, int trcap, int maxlog, size_t extra_bytes = 0) {
        using State = typename std::remove_pointer<decltype(A.st)>::type;
        using Desc = typename std::remove_pointer<decltype(A.desc)>::type;
        size_t off = 0;
        auto carve = [&off](size_t bytes) {
            const size_t o = off;
            off += (bytes + 15) & ~(size_t)15;
            return o;
        };
        const size_t o_st = carve(sizeof(State) * nb), o_desc = carve(sizeof(Desc) * nb);
        const size_t o_tr = carve(sizeof(psd_ztr) * (size_t)nb * p * trcap), o_cnt = carve(sizeof(int) * (size_t)nb * p);
        const size_t o_dG = carve(sizeof(psd_ztr) * (size_t)nb * (n + 2)), o_alpha = carve(sizeof(psd_z) * (size_t)nb * n);
        const size_t o_beta = carve(sizeof(double) * (size_t)nb * n), o_asc = carve(sizeof(int) * (size_t)nb * n);
        const size_t o_log = carve(sizeof(int) * (size_t)nb * 3 * maxlog), o_info = carve(sizeof(int) * nb);
        const size_t o_extra = carve(extra_bytes);
        PSD_CHECK(buf.alloc(off));
        PSD_CHECK(psd_rt_memset(buf.ptr, 0, off, c->stream));
        char* w = (char*)buf.ptr;
        A.st = (State*)(w + o_st);
        A.desc = (Desc*)(w + o_desc);
        A.tr = (psd_ztr*)(w + o_tr);
        A.cnt = (int*)(w + o_cnt);
        A.dG = (psd_ztr*)(w + o_dG);
        A.alpha = (psd_z*)(w + o_alpha);
        A.beta = (double*)(w + o_beta);
        A.ascale = (int*)(w + o_asc);
        A.log = (int*)(w + o_log);
        A.infos = (int*)(w + o_info);
        extra = w + o_extra;
        A.n = n; A.p = p; A.maxlog = maxlog;
        return 0;
    }
};

// what the kernel left in one problem's state (psd_zstate, psd_zgstate), added to the call's
template <class State>
void zbatch_add_state(psd_stats* s, const State& st) {
    s->niter += st.jiter;
    s->nsweeps += st.nsweeps;
    s->nrqpass += st.nzshift;
    s->ndefl1 += st.nsplit;
    s->ndefl2 += st.ncase2;
    s->nwindows += st.nwindows;
    s->nlog += st.nlog;
}

// The iteration for nb Hessenberg-triangular problems on the device: dH / dZ [nb][p][n][n] internal order (dZ holds the
// Q_j on entry).  alpha (nb * n complex pairs), beta, ascale (nb * n), infos (nb): host.  Per-problem codes go to infos;
// the return value is a call-wide (runtime / not-implemented) code or 0.
int zbiterate_dev(psd_ctx* c, int nb, int n, int p, psd_z* dH, psd_z* dZ, int wantT, int wantZ, int maxitfac, double* alpha,
                  double* beta, int32_t* ascale, int* infos, psd_stats* s) {
    const size_t nn = (size_t)n * n;
    const int W = choose_window(p, 16);
    if (W == 0) return PSD_INFO_NOTIMPL;
    const int maxlog = 2 * maxitfac * n + n + 16;
    if (n > c->zb_nmax) {
        int rc = c->zreserve(n, p, false, maxlog);
        if (rc != 0) return rc;
        for (int q = 0; q < nb; ++q) {
            psd_stats ps;
            memset(&ps, 0, sizeof(ps));
            rc = zrun_iteration(c, n, p, dH + (size_t)q * p * nn, wantZ ? dZ + (size_t)q * p * nn : nullptr, wantT, wantZ,
                                maxitfac, alpha + 2 * (size_t)q * n, beta + (size_t)q * n, ascale + (size_t)q * n, &ps,
                                nullptr, 0);
            if (batch_fatal(rc) && rc != PSD_INFO_RUNTIME + 77) return rc;
            infos[q] = rc;
            batch_add_counts(s, ps);
        }
        s->window = W;
        return 0;
    }
    zb_work<psd_zbqz_args> ws;
    if (int e = ws.alloc(c, nb, n, p, PSD_ZTR_CAP, maxlog)) return e;
    psd_zbqz_args& A = ws.A;
    A.H = dH;
    A.Z = wantZ ? dZ : nullptr;
    A.wantT = wantT; A.wantZ = wantZ; A.W = W; A.maxitfac = maxitfac;
    const int nbmin = (W - 3 > 0) ? ((W - 3 < 8) ? (W - 3) : 8) : 1;  // (the bound of ziterate_dev's tick loop)
    A.cap = (long long)maxitfac * n * ((long long)n / nbmin + 4) + 4LL * n + 1024;
    size_t lds = step_lds_bytes(p, W, 16);
    if (psd_zbqz_apply_lds_bytes(W) > lds) lds = psd_zbqz_apply_lds_bytes(W);
    PSD_CHECK(c->lds_limit(reinterpret_cast<const void*>(psd_zbqz), lds));
    PSD_LAUNCH(psd_zbqz, psd_dim3(nb), PSD_STEP_NT, lds, c->stream, A);
    std::vector<psd_zstate> hst(nb);
    std::vector<int> hsc((size_t)nb * n), hinfo(nb);
    PSD_CHECK(psd_rt_d2h(hst.data(), A.st, sizeof(psd_zstate) * nb, c->stream));
    PSD_CHECK(psd_rt_d2h(alpha, A.alpha, sizeof(psd_z) * (size_t)nb * n, c->stream));
    PSD_CHECK(psd_rt_d2h(beta, A.beta, sizeof(double) * (size_t)nb * n, c->stream));
    PSD_CHECK(psd_rt_d2h(hsc.data(), A.ascale, sizeof(int) * (size_t)nb * n, c->stream));
    PSD_CHECK(psd_rt_d2h(hinfo.data(), A.infos, sizeof(int) * nb, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    for (size_t e = 0; e < (size_t)nb * n; ++e) ascale[e] = hsc[e];
    for (int q = 0; q < nb; ++q) {
        infos[q] = batch_info_code(hinfo[q]);
        zbatch_add_state(s, hst[q]);
    }
    s->nlaunch_step += 1;
    s->window = W;
    return 0;
}

// The whole path for nb problems resident on the device: dA / dZ [nb][p][n][n] in user order.  s receives the counters
// and times of this call.  Per-problem codes go to infos; returns a call-wide (argument / runtime) code or 0.
int zpschur_batch_core(psd_ctx* c, int nb, int n, int p, psd_z* dA, bool left, int wantT, int wantZ, int maxitfac, psd_z* dZ,
                       double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* s) {
    memset(s, 0, sizeof(*s));
    if (c->shard_world > 1) return PSD_INFO_NOTIMPL;  // (a period-sharded context keeps a slice of Z: single problems only)
    int rc = 0;
    if (n > c->zb_nmax && (rc = c->zreserve(n, p, false, 2 * maxitfac * n + n + 16)) != 0) return rc;
    psd_batchbuf dtau;
    PSD_CHECK(dtau.alloc(sizeof(psd_z) * (size_t)nb * p * n));
    Timer tall, tph;
    tall.start(c->stream);
    rc = batch_reversed(c, left, nb, p, 2 * (size_t)n * n, (double*)dA, wantZ ? (double*)dZ : nullptr, [&]() {
        tph.start(c->stream);
        if (int e = zbhessenberg_dev(c, nb, n, p, dA, (psd_z*)dtau.ptr)) return e;
        s->ms_hess = tph.stop(c->stream);
        tph.start(c->stream);
        if (int e = zbformq_dev(c, nb, n, p, dA, (const psd_z*)dtau.ptr, wantZ ? dZ : nullptr)) return e;
        s->ms_formq = tph.stop(c->stream);
        tph.start(c->stream);
        if (int e = zbiterate_dev(c, nb, n, p, dA, dZ, wantT, wantZ, maxitfac, alpha, beta, ascale, infos, s)) return e;
        s->ms_iter = tph.stop(c->stream);
        return 0;
    });
    if (rc != 0) return rc;
    s->ms_total = tall.stop(c->stream);
    s->bytes_hess = nb * 2.0 * 16.0 * p * (5.0 / 6.0) * (double)n * n * n;
    s->bytes_formq = wantZ ? nb * 2.0 * 16.0 * p * (double)n * n * n / 3.0 : 0.0;
    PSD_CHECK(psd_rt_last_error());
    return 0;
}

}  // namespace

extern "C" {

int psd_z_phessenberg_batch(psd_ctx* c, int nb, int n, int p, double* const* A, double* tau, psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    if ((*info = k.head(c, nb, n, p)) != 0) return *info;
    if (!A) return *info = -5;
    if (!tau) return *info = -6;
    if ((*info = c->zreserve(n, p, false, 16)) != 0) return *info;
    const size_t nn2 = 2 * (size_t)n * n;  // doubles of one factor
    const batch_list L[] = {{A, p, nn2, BATCH_IN | BATCH_OUT}};
    psd_batchbuf dtau;
    Timer tk;
    auto extra = [&](int g) { return psd_rt_code(dtau.alloc(sizeof(psd_z) * (size_t)g * p * n)); };
    auto body = [&](int q0, int gc, double* const* d) {
        tk.start(c->stream);
        if (int e = zbhessenberg_dev(c, gc, n, p, (psd_z*)d[0], (psd_z*)dtau.ptr)) return e;
        k.s->ms_hess += tk.stop(c->stream);
        tk.start(c->stream);
        PSD_CHECK(psd_rt_d2h(tau + 2 * (size_t)q0 * p * n, dtau.ptr, sizeof(psd_z) * (size_t)gc * p * n, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        k.s->ms_copy += tk.stop(c->stream);
        return 0;
    };
    *info = batch_staged(c, nb, sizeof(double) * (nn2 + 2 * (size_t)n) * p, L, k.s, extra, body);
    if (*info != 0) return *info;
    PSD_CHECK(psd_rt_last_error());
    k.s->ms_total = k.s->ms_hess;
    k.s->bytes_hess = nb * 2.0 * 16.0 * p * (5.0 / 6.0) * (double)n * n * n;
    return *info = 0;
}

int psd_z_pschur_batch_dev(psd_ctx* c, int nb, int n, int p, double* dA, char orient, int wantT, int wantZ, int maxitfac,
                           double* dZ, double* alpha, double* beta, int32_t* ascale, int* infos, int* schurindex,
                           psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    if ((*info = k.head(c, nb, n, p)) != 0) return *info;
    if (!dA) return *info = -5;
    if (orient != 'R' && orient != 'L') return *info = -6;  // PSD.jl:175-177
    if (maxitfac < 1) return *info = -9;
    if (wantZ && !dZ) return *info = -10;
    if (!alpha || !beta || !ascale) return *info = -11;
    int* pinfos = k.infos(infos, nb);
    const int rc = zpschur_batch_core(c, nb, n, p, reinterpret_cast<psd_z*>(dA), orient == 'L', wantT, wantZ, maxitfac,
                                      reinterpret_cast<psd_z*>(dZ), alpha, beta, ascale, pinfos, k.s);
    if (schurindex) *schurindex = (orient == 'L') ? p : 1;
    return *info = (rc != 0) ? rc : batch_first_code(pinfos, nb);
}

int psd_z_pschur_batch(psd_ctx* c, int nb, int n, int p, double* const* A, char orient, int wantT, int wantZ, int maxitfac,
                       double* const* Z, double* alpha, double* beta, int32_t* ascale, int* infos, int* schurindex,
                       psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    if ((*info = k.head(c, nb, n, p)) != 0) return *info;
    if (!A) return *info = -5;
    if (orient != 'R' && orient != 'L') return *info = -6;
    if (maxitfac < 1) return *info = -9;
    if (wantZ && !Z) return *info = -10;
    if (!alpha || !beta || !ascale) return *info = -11;
    const size_t nn2 = 2 * (size_t)n * n;
    const batch_list L[] = {{A, p, nn2, BATCH_IN | BATCH_OUT}, {wantZ ? Z : nullptr, p, nn2, BATCH_OUT}};
    int* pinfos = k.infos(infos, nb);
    auto body = [&](int q0, int gc, double* const* d) {
        psd_stats gs;
        // complex rule: the core returns call-wide codes only and each of them ends the group loop; the per-problem
        // codes wait in pinfos
        if (int e = zpschur_batch_core(c, gc, n, p, (psd_z*)d[0], orient == 'L', wantT, wantZ, maxitfac, (psd_z*)d[1],
                                       alpha + 2 * (size_t)q0 * n, beta + (size_t)q0 * n, ascale + (size_t)q0 * n,
                                       pinfos + q0, &gs))
            return e;
        batch_add_stats(k.s, gs, true);
        return 0;
    };
    *info = batch_staged(c, nb, sizeof(double) * ((wantZ ? 2 : 1) * nn2 + 2 * (size_t)n) * p, L, k.s, batch_no_extra, body);
    if (*info != 0) return *info;
    if (schurindex) *schurindex = (orient == 'L') ? p : 1;
    return *info = batch_first_code(pinfos, nb);
}

int psd_z_pschur_hess_batch(psd_ctx* c, int nb, int n, int p, double* const* H, double* const* Q, int wantT, int wantZ,
                            int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* stats,
                            int* info) {
    batch_call<psd_stats> k(info, stats);
    if ((*info = k.head(c, nb, n, p)) != 0) return *info;
    if (!H) return *info = -5;
    if (wantZ && !Q) return *info = -6;
    if (maxitfac < 1) return *info = -9;
    if (!alpha || !beta || !ascale) return *info = -10;
    if (c->shard_world > 1) return *info = PSD_INFO_NOTIMPL;
    const size_t nn2 = 2 * (size_t)n * n;
    const batch_list L[] = {{H, p, nn2, BATCH_IN | BATCH_OUT}, {wantZ ? Q : nullptr, p, nn2, BATCH_IN | BATCH_OUT}};
    int* pinfos = k.infos(infos, nb);
    Timer tk;
    auto body = [&](int q0, int gc, double* const* d) {
        tk.start(c->stream);
        if (int e = zbiterate_dev(c, gc, n, p, (psd_z*)d[0], (psd_z*)d[1], wantT, wantZ, maxitfac, alpha + 2 * (size_t)q0 * n,
                                  beta + (size_t)q0 * n, ascale + (size_t)q0 * n, pinfos + q0, k.s))
            return e;
        k.s->ms_iter += tk.stop(c->stream);
        return 0;
    };
    *info = batch_staged(c, nb, sizeof(double) * ((wantZ ? 2 : 1) * nn2 + 2 * (size_t)n) * p, L, k.s, batch_no_extra, body);
    if (*info != 0) return *info;
    k.s->ms_total = k.s->ms_iter;
    return *info = batch_first_code(pinfos, nb);
}

}  // extern "C"
