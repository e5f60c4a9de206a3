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
//
// The signed drivers (psd_zgbatch_host.inl, and psd_gbatch_host.inl for Float64) come in behind this file and share its
// workspace (zb_work), the launch and read-back of the iteration kernel (zb_launch), the fallback loop above the cap
// (zb_single_loop) and the bodies of the three kinds of entry with their argument codes (zb_pschur_batch_dev,
// zb_pschur_batch, zb_pschur_hess_batch), which take the signature and the family.

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


// Per-problem workspace of psd_zbqz / psd_zgbqz / psd_gbqz (Args: their argument struct, which names the types of the
// state, the descriptor and the rotation records) for nb problems, carved from one zeroed allocation, every region
// 16-byte aligned; `extra` bytes follow the per-problem arrays (the signed kernels' signature, the real kernel's xscr).
// alloc fills the workspace pointers and n, p, maxlog of A.
template <class Args>
struct zb_work {
    psd_batchbuf buf;
    Args A;
    char* extra = nullptr;
    int alloc(psd_ctx* c, int nb, int n, int p, int trcap, int maxlog, size_t extra_bytes = 0) {
        using State = typename std::remove_pointer<decltype(A.st)>::type;
        using Desc = typename std::remove_pointer<decltype(A.desc)>::type;
        using Rot = typename std::remove_pointer<decltype(A.tr)>::type;
        size_t off = 0;
        auto carve = [&off](size_t bytes) {
            const size_t o = off;
            off += (bytes + 15) & ~(size_t)15;
            return o;
        };
        const size_t o_st = carve(sizeof(State) * nb), o_desc = carve(sizeof(Desc) * nb);
        const size_t o_tr = carve(sizeof(Rot) * (size_t)nb * p * trcap), o_cnt = carve(sizeof(int) * (size_t)nb * p);
        const size_t o_dG = carve(sizeof(Rot) * (size_t)nb * (n + 2)), o_alpha = carve(sizeof(psd_z) * (size_t)nb * n);
        const size_t o_beta = carve(sizeof(double) * (size_t)nb * n), o_asc = carve(sizeof(int) * (size_t)nb * n);
        const size_t o_log = carve(sizeof(int) * (size_t)nb * 3 * maxlog), o_info = carve(sizeof(int) * nb);
        const size_t o_extra = carve(extra_bytes);
        PSD_CHECK(buf.alloc(off));
        PSD_CHECK(psd_rt_memset(buf.ptr, 0, off, c->stream));
        char* w = (char*)buf.ptr;
        A.st = (State*)(w + o_st);
        A.desc = (Desc*)(w + o_desc);
        A.tr = (Rot*)(w + o_tr);
        A.cnt = (int*)(w + o_cnt);
        A.dG = (Rot*)(w + o_dG);
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

// what psd_zbqz asks of zb_launch (the signed kernels: zgbqz_signed, psd_zgbatch_host.inl; gbqz_signed,
// psd_gbatch_host.inl)
struct zbqz_unsigned {
    using args_t = psd_zbqz_args;
    using state_t = psd_zstate;
    static constexpr int esize = 16;  // bytes of an element: the window choose_window / step_lds_bytes give
    static constexpr int capk = 4;    // (the slack of ziterate_dev's tick loop)
    static constexpr int capw = 3;    // (the positions it takes off the window for the shortest one)
    static size_t apply_lds(int W) { return psd_zbqz_apply_lds_bytes(W); }
    static void set_hessmode(args_t&, int) {}
    static const void* kernel() { return reinterpret_cast<const void*>(psd_zbqz); }
    static void launch(psd_ctx* c, int nb, size_t lds, const args_t& A) {
        PSD_LAUNCH(psd_zbqz, psd_dim3(nb), PSD_STEP_NT, lds, c->stream, A);
    }
};

// One launch of the iteration kernel K over the nb problems of ws (dH / dZ [nb][p][n][n]) and one read-back: the states
// and what the kernel left as per-problem codes (PSD_LIST_OVERFLOW, PSD_ZB_TICKCAP, level) in hst / hinfo, and with alpha
// (nb * n complex pairs, host) the scaled eigenvalues in alpha, beta, ascale.  hessmode: stage 2 of the signed reduction.
template <class K>
int zb_launch(psd_ctx* c, zb_work<typename K::args_t>& ws, int nb, decltype(K::args_t::H) dH, decltype(K::args_t::H) dZ,
              int wantT, int wantZ, int maxitfac, int hessmode, std::vector<typename K::state_t>& hst, std::vector<int>& hinfo, double* alpha = nullptr,
              double* beta = nullptr, int32_t* ascale = nullptr) {
    typename K::args_t& A = ws.A;
    const int n = A.n, p = A.p;
    const int W = choose_window(p, K::esize);
    if (W == 0) return PSD_INFO_NOTIMPL;
    A.H = dH;
    A.Z = wantZ ? dZ : nullptr;
    A.wantT = wantT; A.wantZ = wantZ; A.W = W; A.maxitfac = maxitfac;
    K::set_hessmode(A, hessmode);
    const int nbmin = (W - K::capw > 0) ? ((W - K::capw < 8) ? (W - K::capw) : 8) : 1;  // (the bound of the single drivers' tick loops)
    A.cap = (long long)maxitfac * n * ((long long)n / nbmin + K::capk) + (long long)K::capk * n + 1024 +
            (hessmode ? (long long)n * n : 0);
    const size_t lds = std::max(step_lds_bytes(p, W, K::esize), K::apply_lds(W));
    PSD_CHECK(c->lds_limit(K::kernel(), lds));
    K::launch(c, nb, lds, A);
    const size_t nv = alpha ? (size_t)nb * n : 0;
    std::vector<int> hsc(nv);
    hst.resize(nb);
    hinfo.resize(nb);
    PSD_CHECK(psd_rt_d2h(hst.data(), A.st, sizeof(typename K::state_t) * nb, c->stream));
    PSD_CHECK(psd_rt_d2h(hinfo.data(), A.infos, sizeof(int) * nb, c->stream));
    if (alpha) {
        PSD_CHECK(psd_rt_d2h(alpha, A.alpha, sizeof(psd_z) * nv, c->stream));
        PSD_CHECK(psd_rt_d2h(beta, A.beta, sizeof(double) * nv, c->stream));
        PSD_CHECK(psd_rt_d2h(hsc.data(), A.ascale, sizeof(int) * nv, c->stream));
    }
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    for (size_t e = 0; e < nv; ++e) ascale[e] = hsc[e];
    return 0;
}

// Above the order cap: single(q, &ps) runs the single-problem iteration on problem q.  A code that ends a single call
// ends the batch too unless it is one of `stay` (a list overflow, a tick bound: that problem's alone); W: the window the
// call reports.
template <class Single>
int zb_single_loop(int nb, int W, int* infos, psd_stats* s, std::initializer_list<int> stay, Single single) {
    for (int q = 0; q < nb; ++q) {
        psd_stats ps;
        memset(&ps, 0, sizeof(ps));
        const int rc = single(q, &ps);
        if (batch_fatal(rc) && std::find(stay.begin(), stay.end(), rc) == stay.end()) return rc;
        infos[q] = rc;
        batch_add_counts(s, ps);
    }
    s->window = W;
    return 0;
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
        if (int e = c->zreserve(n, p, false, maxlog)) return e;
        return zb_single_loop(nb, W, infos, s, {PSD_INFO_RUNTIME + 77}, [&](int q, psd_stats* ps) {
            return zrun_iteration(c, n, p, dH + (size_t)q * p * nn, wantZ ? dZ + (size_t)q * p * nn : nullptr, wantT, wantZ,
                                  maxitfac, alpha + 2 * (size_t)q * n, beta + (size_t)q * n, ascale + (size_t)q * n, ps, nullptr,
                                  0);
        });
    }
    zb_work<psd_zbqz_args> ws;
    if (int e = ws.alloc(c, nb, n, p, PSD_ZTR_CAP, maxlog)) return e;
    std::vector<psd_zstate> hst;
    std::vector<int> hinfo;
    if (int e = zb_launch<zbqz_unsigned>(c, ws, nb, dH, dZ, wantT, wantZ, maxitfac, 0, hst, hinfo, alpha, beta, ascale)) return e;
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

// The entries below are those of the signed family too (psd_zgbatch_host.inl), which passes its signature S; the unsigned
// entries pass S = null, and an all-true S is the same call (the tuned all-true kernels).
bool zgb_all_true(const uint8_t* S, int p) {
    if (S)
        for (int j = 0; j < p; ++j)
            if (!S[j]) return false;
    return true;
}
int zgbiterate_dev(psd_ctx* c, int nb, int n, int p, psd_z* dH, psd_z* dZ, const uint8_t* S, int wantT, int wantZ,
                   int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* s);
int zgpschur_batch_core(psd_ctx* c, int nb, int n, int p, psd_z* dA, const uint8_t* S, bool left, int wantT, int wantZ,
                        int maxitfac, psd_z* dZ, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* s);

// the head of the pschur entries: the argument codes; returns true when the call is over
bool zb_pschur_head(const batch_call<psd_stats>& k, psd_ctx* c, int nb, int n, int p, const void* A, const uint8_t* S,
                    char orient, int maxitfac, int wantZ, const void* Z, const double* alpha, const double* beta,
                    const int32_t* ascale, int* info) {
    if ((*info = k.head(c, nb, n, p)) != 0) return true;
    if (!A) *info = -5;
    else if (orient != 'R' && orient != 'L') *info = -6;  // PSD.jl:175-177
    else if (S && !S[(orient == 'L') ? p - 1 : 0]) *info = -7;  // generalized.jl:140
    else if (maxitfac < 1) *info = -9;
    else if (wantZ && !Z) *info = -10;
    else if (!alpha || !beta || !ascale) *info = -11;
    return *info != 0;
}

// What the three bodies below ask of a family F (zb_complex here; gb_real, psd_gbatch_host.inl): elem, the element type
// (dpe doubles each); core, the whole path for a batch on the device in user order; iterate, the iteration alone.  The
// complex family sends an all-true S to the tuned all-true kernels, the real one keeps it on the signed kernels (as
// psd_d_gpschur's outputs have another form than psd_d_pschur_batch's).
struct zb_complex {
    using elem = psd_z;
    static constexpr size_t dpe = 2;
    static int core(psd_ctx* c, int nb, int n, int p, psd_z* dA, const uint8_t* S, bool left, int wantT, int wantZ, int maxitfac,
                    psd_z* dZ, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* s) {
        return zgb_all_true(S, p)
                   ? zpschur_batch_core(c, nb, n, p, dA, left, wantT, wantZ, maxitfac, dZ, alpha, beta, ascale, infos, s)
                   : zgpschur_batch_core(c, nb, n, p, dA, S, left, wantT, wantZ, maxitfac, dZ, alpha, beta, ascale, infos, s);
    }
    static int iterate(psd_ctx* c, int nb, int n, int p, psd_z* dH, psd_z* dZ, const uint8_t* S, int wantT, int wantZ,
                       int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* s) {
        return zgb_all_true(S, p) ? zbiterate_dev(c, nb, n, p, dH, dZ, wantT, wantZ, maxitfac, alpha, beta, ascale, infos, s)
                                  : zgbiterate_dev(c, nb, n, p, dH, dZ, S, wantT, wantZ, maxitfac, alpha, beta, ascale, infos, s);
    }
};

// The cores return call-wide codes only and each of them ends the call; the per-problem codes wait in the infos.
template <class F = zb_complex>
int zb_pschur_batch_dev(psd_ctx* c, int nb, int n, int p, double* dA, const uint8_t* S, char orient, int wantT, int wantZ,
                        int maxitfac, double* dZ, double* alpha, double* beta, int32_t* ascale, int* infos, int* schurindex,
                        psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    if (zb_pschur_head(k, c, nb, n, p, dA, S, orient, maxitfac, wantZ, dZ, alpha, beta, ascale, info)) return *info;
    int* pinfos = k.infos(infos, nb);
    typename F::elem* A = reinterpret_cast<typename F::elem*>(dA);
    typename F::elem* Z = reinterpret_cast<typename F::elem*>(dZ);
    const bool left = orient == 'L';
    const int rc = F::core(c, nb, n, p, A, S, left, wantT, wantZ, maxitfac, Z, alpha, beta, ascale, pinfos, k.s);
    if (schurindex) *schurindex = left ? p : 1;
    return *info = (rc != 0) ? rc : batch_first_code(pinfos, nb);
}

template <class F = zb_complex>
int zb_pschur_batch(psd_ctx* c, int nb, int n, int p, double* const* A, const uint8_t* S, char orient, int wantT, int wantZ,
                    int maxitfac, double* const* Z, double* alpha, double* beta, int32_t* ascale, int* infos, int* schurindex,
                    psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    if (zb_pschur_head(k, c, nb, n, p, A, S, orient, maxitfac, wantZ, Z, alpha, beta, ascale, info)) return *info;
    const size_t nn2 = F::dpe * (size_t)n * n;  // doubles of one factor
    const batch_list L[] = {{A, p, nn2, BATCH_IN | BATCH_OUT}, {wantZ ? Z : nullptr, p, nn2, BATCH_OUT}};
    int* pinfos = k.infos(infos, nb);
    const bool left = orient == 'L';
    auto body = [&](int q0, int gc, double* const* d) {
        psd_stats gs;
        typename F::elem* dA = (typename F::elem*)d[0];
        typename F::elem* dZ = (typename F::elem*)d[1];
        double* al = alpha + 2 * (size_t)q0 * n;
        double* be = beta + (size_t)q0 * n;
        int32_t* sc = ascale + (size_t)q0 * n;
        if (int e = F::core(c, gc, n, p, dA, S, left, wantT, wantZ, maxitfac, dZ, al, be, sc, pinfos + q0, &gs)) return e;
        batch_add_stats(k.s, gs, true);
        return 0;
    };
    *info = batch_staged(c, nb, sizeof(double) * ((wantZ ? 2 : 1) * nn2 + 2 * (size_t)n) * p, L, k.s, batch_no_extra, body);
    if (*info != 0) return *info;
    if (schurindex) *schurindex = left ? p : 1;
    return *info = batch_first_code(pinfos, nb);
}

// noval: the code of missing eigenvalue arrays, which the two entries number differently
template <class F = zb_complex>
int zb_pschur_hess_batch(psd_ctx* c, int nb, int n, int p, double* const* H, const uint8_t* S, double* const* Q, int wantT,
                         int wantZ, int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* stats,
                         int* info, int noval) {
    batch_call<psd_stats> k(info, stats);
    if ((*info = k.head(c, nb, n, p)) != 0) return *info;
    if (!H) return *info = -5;
    if (wantZ && !Q) return *info = -6;
    if (S && !S[0]) return *info = -7;
    if (maxitfac < 1) return *info = -9;
    if (!alpha || !beta || !ascale) return *info = noval;
    if (c->shard_world > 1) return *info = PSD_INFO_NOTIMPL;
    const size_t nn2 = F::dpe * (size_t)n * n;
    const batch_list L[] = {{H, p, nn2, BATCH_IN | BATCH_OUT}, {wantZ ? Q : nullptr, p, nn2, BATCH_IN | BATCH_OUT}};
    int* pinfos = k.infos(infos, nb);
    Timer tk;
    auto body = [&](int q0, int gc, double* const* d) {
        typename F::elem* dH = (typename F::elem*)d[0];
        typename F::elem* dZ = (typename F::elem*)d[1];
        double* al = alpha + 2 * (size_t)q0 * n;
        double* be = beta + (size_t)q0 * n;
        int32_t* sc = ascale + (size_t)q0 * n;
        tk.start(c->stream);
        if (int e = F::iterate(c, gc, n, p, dH, dZ, S, wantT, wantZ, maxitfac, al, be, sc, pinfos + q0, k.s)) return e;
        k.s->ms_iter += tk.stop(c->stream);
        return 0;
    };
    *info = batch_staged(c, nb, sizeof(double) * ((wantZ ? 2 : 1) * nn2 + 2 * (size_t)n) * p, L, k.s, batch_no_extra, body);
    if (*info != 0) return *info;
    k.s->ms_total = k.s->ms_iter;
    return *info = batch_first_code(pinfos, nb);
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
    return zb_pschur_batch_dev(c, nb, n, p, dA, nullptr, orient, wantT, wantZ, maxitfac, dZ, alpha, beta, ascale, infos,
                               schurindex, stats, info);
}

int psd_z_pschur_batch(psd_ctx* c, int nb, int n, int p, double* const* A, char orient, int wantT, int wantZ, int maxitfac,
                       double* const* Z, double* alpha, double* beta, int32_t* ascale, int* infos, int* schurindex,
                       psd_stats* stats, int* info) {
    return zb_pschur_batch(c, nb, n, p, A, nullptr, orient, wantT, wantZ, maxitfac, Z, alpha, beta, ascale, infos, schurindex,
                           stats, info);
}

int psd_z_pschur_hess_batch(psd_ctx* c, int nb, int n, int p, double* const* H, double* const* Q, int wantT, int wantZ,
                            int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* stats,
                            int* info) {
    return zb_pschur_hess_batch(c, nb, n, p, H, nullptr, Q, wantT, wantZ, maxitfac, alpha, beta, ascale, infos, stats, info, -10);
}

}  // extern "C"
