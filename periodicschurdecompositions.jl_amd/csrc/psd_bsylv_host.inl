// Host driver of psd_?_psylv_batch[_dev] and psd_?_subcond_batch[_dev] (psd_bsylv.h): periodic Sylvester solves on the
// off-diagonal block of nb periodic Schur forms of one shape split at m[q], and the periodic form of xTRSEN's two numbers,
// s[q][l] = 1 / sqrt(1 + ||X_l||_F^2) and sep[q] = 1 / est(|| S^-1 ||_1).  Included at the end of psd_engine.cpp behind
// psd_batch_host.inl (psd_batchbuf, batch_call, batch_staged) and psd_bevec_host.inl (bevec_dev_groups).
//
// Per group of problems the condition entry launches one solve for X, one psd_bsyl_norms, and per step of the estimator
// one solve and one psd_bsyl_est_step (at most 2 * PSD_BSYL_ITMAX + 1 solves: xLACN2 needs no more); after every step one
// record per problem comes back, and the problems that are done leave the launches that follow.  A problem with m = 0 or
// m = n takes part in no launch.  Orders above bsyl_nmax, and periods whose small-block scratch does not fit the LDS:
// PSD_INFO_NOTIMPL — the batch entries do not fall back to the single-problem path (psd_sylv_host.inl, included behind
// this file, which shares the argument checks, the small arrays and the condition group below with it).

namespace {

struct bsylv_call {
    psd_ctx* c;
    int n, p, qsub;
    bool left;
    size_t xb;  // elements of a block of X
};

// capped: the batch entries, which end at bsyl_nmax
int bsylv_checked(const psd_ctx* c, bool cplx, int nb, int n, int p, const void* T, char orient, int schurindex,
                  const int* m, bool capped = true) {
    if (!c) return -1;
    if (nb < 0) return -2;
    if (n < 1) return -3;
    if (p < 1) return -4;
    if (nb == 0) return 0;
    if (!T) return -5;
    if (orient != 'R' && orient != 'L') return -6;
    if (schurindex < 1 || schurindex > p) return -7;
    if (!m) return -8;
    for (int q = 0; q < nb; ++q)
        if (m[q] < 0 || m[q] > n) return -8;
    if (c->shard_world > 1) return PSD_INFO_NOTIMPL;  // (as the other batch entries)
    if (capped && n > c->bsyl_nmax) return PSD_INFO_NOTIMPL;  // (the batch entries keep their cap)
    if (psd_bsyl_lds_bytes(p, cplx) > (size_t)160 * 1024) return PSD_INFO_NOTIMPL;  // (the scratch of p factors: ComplexF64 p > 19, Float64 p > 136)
    return 0;
}
size_t bsylv_xb_min(int nb, int n, const int* m) {
    size_t need = 0;
    for (int q = 0; q < nb; ++q) need = std::max(need, (size_t)m[q] * (size_t)(n - m[q]));
    return need;
}
// a split inside a 2x2 block of the quasi-triangular factor (Float64): -8
int bsylv_split_host(int nb, int n, int p, int qsub, double* const* T, const int* m) {
    for (int q = 0; q < nb; ++q)
        if (m[q] > 0 && m[q] < n && T[(size_t)q * p + qsub][(size_t)(m[q] - 1) * n + m[q]] != 0.0) return -8;
    return 0;
}
int bsylv_split_dev(psd_ctx* c, int nb, int n, int p, int qsub, const double* dT, const int* m) {
    psd_batchbuf b;
    PSD_CHECK(b.alloc(sizeof(int) * 2 * (size_t)nb));
    int* dm = (int*)b.ptr;
    PSD_CHECK(psd_rt_h2d(dm, m, sizeof(int) * nb, c->stream));
    PSD_LAUNCH(psd_bsyl_split, psd_dim3((nb + 63) / 64), 64, 0, c->stream, dT, (const int*)dm, dm + nb, nb, n, p, qsub);
    std::vector<int> bad(nb);
    PSD_CHECK(psd_rt_d2h(bad.data(), dm + nb, sizeof(int) * nb, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    for (int q = 0; q < nb; ++q)
        if (bad[q]) return -8;
    return 0;
}

// the small per-problem arrays of a group on the device: m, act, info, kase, the estimator's records
struct bsylv_small {
    psd_batchbuf b;
    int *m = nullptr, *act = nullptr, *info = nullptr, *kase = nullptr;
    psd_bsyl_est* rec = nullptr;
    int alloc(int g) {
        const size_t recs = (sizeof(int) * 4 * (size_t)g + 15) & ~(size_t)15;
        const int rc = b.alloc(recs + sizeof(psd_bsyl_est) * (size_t)g);
        if (rc != 0) return rc;
        m = (int*)b.ptr;
        act = m + g;
        info = act + g;
        kase = info + g;
        rec = (psd_bsyl_est*)((char*)b.ptr + recs);
        return 0;
    }
};

template <bool CPLX>
int bsylv_launch_solve(const bsylv_call& k, int gc, const double* dT, double* dX, const bsylv_small& sm, const int* ptrans,
                       int trans, int fromT, psd_bsylv_stats* st) {
    psd_bsyl_args g;
    g.T = dT; g.X = dX; g.m = sm.m; g.act = sm.act; g.ptrans = ptrans; g.info = sm.info;
    g.xb = k.xb; g.n = k.n; g.p = k.p; g.qsub = k.qsub; g.left = k.left; g.trans = trans; g.fromT = fromT;
    const size_t lds = psd_bsyl_lds_bytes(k.p, CPLX);
    PSD_CHECK(k.c->lds_limit(reinterpret_cast<const void*>(psd_bsyl_solve<CPLX>), lds));
    PSD_LAUNCH(psd_bsyl_solve<CPLX>, psd_dim3(gc), 64, lds, k.c->stream, g);
    st->nsolve += 1;
    return 0;
}

// m, act = (0 < m < n) and zeroed codes of a group go up; returns the number of active problems
int bsylv_begin(psd_ctx* c, int gc, int n, const int* m, bsylv_small& sm, std::vector<int>& act, int* nact) {
    act.resize(gc);
    *nact = 0;
    for (int q = 0; q < gc; ++q) *nact += (act[q] = (m[q] > 0 && m[q] < n) ? 1 : 0);
    if (*nact == 0) return 0;
    PSD_CHECK(psd_rt_h2d(sm.m, m, sizeof(int) * gc, c->stream));
    PSD_CHECK(psd_rt_h2d(sm.act, act.data(), sizeof(int) * gc, c->stream));
    PSD_CHECK(psd_rt_memset(sm.info, 0, sizeof(int) * gc, c->stream));
    return 0;
}

// psylv: gc problems on the device, dC [gc][p][xb] in/out
template <bool CPLX>
int bsylv_solve_group(const bsylv_call& k, int gc, const double* dT, double* dC, const int* m, int trans, int fromT,
                      bsylv_small& sm, int* infos, psd_bsylv_stats* st) {
    psd_ctx* c = k.c;
    st->ngroups += 1;
    std::vector<int> act;
    int nact = 0;
    for (int q = 0; q < gc; ++q) infos[q] = 0;
    if (int e = bsylv_begin(c, gc, k.n, m, sm, act, &nact)) return e;
    if (nact == 0) return 0;
    Timer tk;
    tk.start(c->stream);
    if (int e = bsylv_launch_solve<CPLX>(k, gc, dT, dC, sm, nullptr, trans, fromT, st)) return e;
    PSD_CHECK(psd_rt_d2h(infos, sm.info, sizeof(int) * gc, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    st->ms_kernels += tk.stop(c->stream);
    for (int q = 0; q < gc; ++q) st->nsingular += infos[q] != 0 ? 1 : 0;
    return 0;
}

// the workspaces of a group of the condition entry: X (where the caller has none), the estimator's vector and signs
struct bsylv_work {
    psd_batchbuf x, e, sg;
    bsylv_small sm;
    template <bool CPLX>
    int alloc(int g, int p, size_t xb, bool own_x) {
        const size_t bytes = sizeof(double) * (CPLX ? 2 : 1) * xb * p * g;
        if (own_x)
            if (int rc = x.alloc(bytes)) return rc;
        if (int rc = e.alloc(bytes)) return rc;
        if (!CPLX)
            if (int rc = sg.alloc(bytes)) return rc;
        return sm.alloc(g);
    }
};

// X of a problem = NaN
int bsylv_fill_nan(psd_ctx* c, double* dX, size_t doubles) {
    const std::vector<double> nans(doubles, NAN);
    PSD_CHECK(psd_rt_h2d(dX, nans.data(), sizeof(double) * doubles, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    return 0;
}

// subcond: gc problems on the device; dX [gc][p][xb] receives X (the caller's, or workspace); s [gc][p], sep [gc] host.
// solve(X, ptrans, fromT, rec) applies S^-1 or S^-H to the blocks X of the group in place: ptrans null: S^-1, otherwise
// the device array of the problems' kase, of which rec holds the host's copy (the single-problem walk orders its
// launches by it).
template <bool CPLX, class Solve>
int bsylv_cond_group(const bsylv_call& k, int gc, double* dX, bool want_x, const int* m, bsylv_work& w,
                     double* s, double* sep, int* infos, psd_bsylv_stats* st, Solve solve) {
    psd_ctx* c = k.c;
    const int p = k.p;
    constexpr int E = CPLX ? 2 : 1;
    bsylv_small& sm = w.sm;
    st->ngroups += 1;
    std::vector<int> act;
    int nact = 0;
    for (int q = 0; q < gc; ++q) {  // the trivial splits, and what the others start from
        infos[q] = 0;
        sep[q] = INFINITY;
        for (int l = 0; l < p; ++l) s[(size_t)q * p + l] = 1.0;
    }
    if (int e = bsylv_begin(c, gc, k.n, m, sm, act, &nact)) return e;
    if (nact == 0) return 0;
    Timer tk;
    tk.start(c->stream);
    psd_batchbuf ds;
    PSD_CHECK(ds.alloc(sizeof(double) * (size_t)gc * p));
    std::vector<psd_bsyl_est> rec(gc);
    if (int e = solve(dX, (const int*)nullptr, 1, rec)) return e;
    psd_bsyl_norm_args ng;
    ng.X = dX; ng.m = sm.m; ng.act = sm.act; ng.s = ds.d(); ng.xb = k.xb; ng.n = k.n; ng.p = p;
    PSD_LAUNCH(psd_bsyl_norms<CPLX>, psd_dim3(gc * p), 64, PSD_BSYL_RED_LDS, c->stream, ng);
    st->nnorms += 1;
    std::vector<double> hs((size_t)gc * p);
    PSD_CHECK(psd_rt_d2h(hs.data(), ds.d(), sizeof(double) * hs.size(), c->stream));
    PSD_CHECK(psd_rt_d2h(infos, sm.info, sizeof(int) * gc, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    for (int q = 0; q < gc; ++q) {
        if (!act[q]) continue;
        if (infos[q] != 0) {
            act[q] = 0;
            nact -= 1;
        } else {
            memcpy(s + (size_t)q * p, hs.data() + (size_t)q * p, sizeof(double) * p);
        }
    }
    // the estimator: x = 1 / N, then solve and step in turn until every problem is done
    std::vector<int> einfo(gc, 0);
    if (nact > 0) {
        PSD_CHECK(psd_rt_memset(sm.rec, 0, sizeof(psd_bsyl_est) * gc, c->stream));
        PSD_CHECK(psd_rt_memset(sm.kase, 0, sizeof(int) * gc, c->stream));
    }
    psd_bsyl_est_args eg;
    eg.X = w.e.d(); eg.SG = CPLX ? nullptr : w.sg.d(); eg.m = sm.m; eg.act = sm.act; eg.rec = sm.rec; eg.kase = sm.kase;
    eg.xb = k.xb; eg.n = k.n; eg.p = p;
    for (int step = 0; nact > 0; ++step) {
        if (step > 2 * PSD_BSYL_ITMAX + 1) return PSD_INFO_RUNTIME + 78;  // (xLACN2 cannot take more solves)
        PSD_CHECK(psd_rt_h2d(sm.act, act.data(), sizeof(int) * gc, c->stream));
        if (step > 0)
            if (int e = solve(w.e.d(), (const int*)sm.kase, 0, rec)) return e;
        PSD_LAUNCH(psd_bsyl_est_step<CPLX>, psd_dim3(gc), 64, PSD_BSYL_EST_LDS, c->stream, eg);
        st->nest_steps += 1;
        PSD_CHECK(psd_rt_d2h(rec.data(), sm.rec, sizeof(psd_bsyl_est) * gc, c->stream));
        PSD_CHECK(psd_rt_d2h(einfo.data(), sm.info, sizeof(int) * gc, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        PSD_CHECK(psd_rt_last_error());
        for (int q = 0; q < gc; ++q) {
            if (!act[q]) continue;
            const bool finite = rec[q].est - rec[q].est == 0.0;
            if (einfo[q] != 0 || !finite) {
                infos[q] = PSD_INFO_SINGULAR;
            } else if (rec[q].kase != 0) {
                continue;
            } else if (rec[q].est > 0.0) {
                sep[q] = 1.0 / rec[q].est;
                if (rec[q].iter > st->nest_iter) st->nest_iter = rec[q].iter;
            } else {
                infos[q] = PSD_INFO_SINGULAR;
            }
            act[q] = 0;
            nact -= 1;
        }
    }
    // a problem that ended with the singular code: s = 0, sep = 0, X = NaN
    for (int q = 0; q < gc; ++q) {
        if (infos[q] == 0) continue;
        st->nsingular += 1;
        sep[q] = 0.0;
        for (int l = 0; l < p; ++l) s[(size_t)q * p + l] = 0.0;
        if (want_x)
            if (int e = bsylv_fill_nan(c, dX + (size_t)q * E * k.xb * p, (size_t)E * k.xb * p)) return e;
    }
    st->ms_kernels += tk.stop(c->stream);
    return 0;
}

// the solve of the batch entries' condition group: one launch for the group
template <bool CPLX>
auto bsylv_batch_solver(const bsylv_call& k, int gc, const double* dT, const bsylv_small& sm, psd_bsylv_stats* st) {
    return [=, &k, &sm](double* X, const int* ptrans, int fromT, const std::vector<psd_bsyl_est>&) {
        return bsylv_launch_solve<CPLX>(k, gc, dT, X, sm, ptrans, 0, fromT, st);
    };
}

template <bool CPLX>
int bsylv_psylv_dev(psd_ctx* c, int nb, int n, int p, const double* dT, char orient, int schurindex, const int* m, double* dC,
                    int64_t xb, int trans, int from_t12, int* infos, psd_bsylv_stats* stats, int* info) {
    batch_call<psd_bsylv_stats> entry(info, stats);
    psd_bsylv_stats* st = entry.s;
    if ((*info = bsylv_checked(c, CPLX, nb, n, p, dT, orient, schurindex, m)) != 0 || nb == 0) return *info;
    if (!dC) return *info = -9;
    if (xb < 1 || (size_t)xb < bsylv_xb_min(nb, n, m)) return *info = -10;
    if (!CPLX && (*info = bsylv_split_dev(c, nb, n, p, schurindex - 1, dT, m)) != 0) return *info;
    const bsylv_call k{c, n, p, schurindex - 1, orient == 'L', (size_t)xb};
    constexpr int E = CPLX ? 2 : 1;
    const size_t tb = (size_t)E * n * n * p, cb = (size_t)E * xb * p;
    int* pinfos = entry.infos(infos, nb);
    st->nb = nb;
    *info = bevec_dev_groups(c, nb, 64, [&](int q0, int gc) {
        bsylv_small sm;
        PSD_CHECK(sm.alloc(gc));
        return bsylv_solve_group<CPLX>(k, gc, dT + q0 * tb, dC + q0 * cb, m + q0, trans, from_t12, sm, pinfos + q0, st);
    });
    return *info != 0 ? *info : (*info = batch_first_code(pinfos, nb));
}

template <bool CPLX>
int bsylv_psylv_host(psd_ctx* c, int nb, int n, int p, double* const* T, char orient, int schurindex, const int* m,
                     double* const* Cm, int64_t xb, int trans, int from_t12, int* infos, psd_bsylv_stats* stats, int* info) {
    batch_call<psd_bsylv_stats> entry(info, stats);
    psd_bsylv_stats* st = entry.s;
    if ((*info = bsylv_checked(c, CPLX, nb, n, p, T, orient, schurindex, m)) != 0 || nb == 0) return *info;
    if (!Cm) return *info = -9;
    if (xb < 1 || (size_t)xb < bsylv_xb_min(nb, n, m)) return *info = -10;
    if (!CPLX && (*info = bsylv_split_host(nb, n, p, schurindex - 1, T, m)) != 0) return *info;
    const bsylv_call k{c, n, p, schurindex - 1, orient == 'L', (size_t)xb};
    constexpr int E = CPLX ? 2 : 1;
    const size_t bd = (size_t)E * n * n, cd = (size_t)E * xb;
    const batch_list L[] = {{T, p, bd, BATCH_IN}, {Cm, p, cd, (from_t12 ? 0 : BATCH_IN) | BATCH_OUT}};
    int* pinfos = entry.infos(infos, nb);
    psd_stats copies;  // (batch_staged leaves the time of the copies in a psd_stats)
    memset(&copies, 0, sizeof(copies));
    bsylv_small sm;
    st->nb = nb;
    *info = batch_staged(c, nb, sizeof(double) * (bd + cd) * p + 64, L, &copies,
                         [&](int g) { return psd_rt_code(sm.alloc(g)); }, [&](int q0, int gc, double* const* d) {
        return bsylv_solve_group<CPLX>(k, gc, d[0], d[1], m + q0, trans, from_t12, sm, pinfos + q0, st);
    });
    st->ms_copy = copies.ms_copy;
    return *info != 0 ? *info : (*info = batch_first_code(pinfos, nb));
}

int bsylv_cond_checked(const double* s, const double* sep, const void* X, int64_t xb, int nb, int n, const int* m) {
    if (!s || !sep) return -9;
    if (X && (xb < 1 || (size_t)xb < bsylv_xb_min(nb, n, m))) return -10;
    return 0;
}

template <bool CPLX>
int bsylv_cond_dev(psd_ctx* c, int nb, int n, int p, const double* dT, char orient, int schurindex, const int* m, double* s,
                   double* sep, double* dX, int64_t xb, int* infos, psd_bsylv_stats* stats, int* info) {
    batch_call<psd_bsylv_stats> entry(info, stats);
    psd_bsylv_stats* st = entry.s;
    if ((*info = bsylv_checked(c, CPLX, nb, n, p, dT, orient, schurindex, m)) != 0 || nb == 0) return *info;
    if ((*info = bsylv_cond_checked(s, sep, dX, xb, nb, n, m)) != 0) return *info;
    if (!CPLX && (*info = bsylv_split_dev(c, nb, n, p, schurindex - 1, dT, m)) != 0) return *info;
    if (!dX) xb = (int64_t)std::max<size_t>(bsylv_xb_min(nb, n, m), 1);
    const bsylv_call k{c, n, p, schurindex - 1, orient == 'L', (size_t)xb};
    constexpr int E = CPLX ? 2 : 1;
    const size_t tb = (size_t)E * n * n * p, cb = (size_t)E * xb * p;
    int* pinfos = entry.infos(infos, nb);
    st->nb = nb;
    *info = bevec_dev_groups(c, nb, sizeof(double) * 3 * cb + 64, [&](int q0, int gc) {
        bsylv_work w;
        PSD_CHECK(w.alloc<CPLX>(gc, p, (size_t)xb, !dX));
        return bsylv_cond_group<CPLX>(k, gc, dX ? dX + q0 * cb : w.x.d(), dX != nullptr, m + q0, w, s + (size_t)q0 * p,
                                      sep + q0, pinfos + q0, st, bsylv_batch_solver<CPLX>(k, gc, dT + q0 * tb, w.sm, st));
    });
    return *info != 0 ? *info : (*info = batch_first_code(pinfos, nb));
}

template <bool CPLX>
int bsylv_cond_host(psd_ctx* c, int nb, int n, int p, double* const* T, char orient, int schurindex, const int* m, double* s,
                    double* sep, double* const* X, int64_t xb, int* infos, psd_bsylv_stats* stats, int* info) {
    batch_call<psd_bsylv_stats> entry(info, stats);
    psd_bsylv_stats* st = entry.s;
    if ((*info = bsylv_checked(c, CPLX, nb, n, p, T, orient, schurindex, m)) != 0 || nb == 0) return *info;
    if ((*info = bsylv_cond_checked(s, sep, X, xb, nb, n, m)) != 0) return *info;
    if (!CPLX && (*info = bsylv_split_host(nb, n, p, schurindex - 1, T, m)) != 0) return *info;
    if (!X) xb = (int64_t)std::max<size_t>(bsylv_xb_min(nb, n, m), 1);
    const bsylv_call k{c, n, p, schurindex - 1, orient == 'L', (size_t)xb};
    constexpr int E = CPLX ? 2 : 1;
    const size_t bd = (size_t)E * n * n, cd = (size_t)E * xb;
    const batch_list L[] = {{T, p, bd, BATCH_IN}, {X, p, cd, BATCH_OUT}};
    int* pinfos = entry.infos(infos, nb);
    psd_stats copies;
    memset(&copies, 0, sizeof(copies));
    bsylv_work w;
    st->nb = nb;
    *info = batch_staged(c, nb, sizeof(double) * (bd + 3 * cd) * p + 64, L, &copies,
                         [&](int g) { return psd_rt_code(w.alloc<CPLX>(g, p, (size_t)xb, !X)); },
                         [&](int q0, int gc, double* const* d) {
        return bsylv_cond_group<CPLX>(k, gc, X ? d[1] : w.x.d(), X != nullptr, m + q0, w, s + (size_t)q0 * p, sep + q0,
                                      pinfos + q0, st, bsylv_batch_solver<CPLX>(k, gc, d[0], w.sm, st));
    });
    st->ms_copy = copies.ms_copy;
    return *info != 0 ? *info : (*info = batch_first_code(pinfos, nb));
}

}  // namespace

extern "C" {

int psd_d_psylv_batch(psd_ctx* c, int nb, int n, int p, double* const* T, char orient, int schurindex, const int* m,
                      double* const* C, int64_t xb, int trans, int from_t12, int* infos, psd_bsylv_stats* stats, int* info) {
    return bsylv_psylv_host<false>(c, nb, n, p, T, orient, schurindex, m, C, xb, trans, from_t12, infos, stats, info);
}
int psd_z_psylv_batch(psd_ctx* c, int nb, int n, int p, double* const* T, char orient, int schurindex, const int* m,
                      double* const* C, int64_t xb, int trans, int from_t12, int* infos, psd_bsylv_stats* stats, int* info) {
    return bsylv_psylv_host<true>(c, nb, n, p, T, orient, schurindex, m, C, xb, trans, from_t12, infos, stats, info);
}
int psd_d_psylv_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, char orient, int schurindex, const int* m,
                          double* dC, int64_t xb, int trans, int from_t12, int* infos, psd_bsylv_stats* stats, int* info) {
    return bsylv_psylv_dev<false>(c, nb, n, p, dT, orient, schurindex, m, dC, xb, trans, from_t12, infos, stats, info);
}
int psd_z_psylv_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, char orient, int schurindex, const int* m,
                          double* dC, int64_t xb, int trans, int from_t12, int* infos, psd_bsylv_stats* stats, int* info) {
    return bsylv_psylv_dev<true>(c, nb, n, p, dT, orient, schurindex, m, dC, xb, trans, from_t12, infos, stats, info);
}

int psd_d_subcond_batch(psd_ctx* c, int nb, int n, int p, double* const* T, char orient, int schurindex, const int* m,
                        double* s, double* sep, double* const* X, int64_t xb, int* infos, psd_bsylv_stats* stats, int* info) {
    return bsylv_cond_host<false>(c, nb, n, p, T, orient, schurindex, m, s, sep, X, xb, infos, stats, info);
}
int psd_z_subcond_batch(psd_ctx* c, int nb, int n, int p, double* const* T, char orient, int schurindex, const int* m,
                        double* s, double* sep, double* const* X, int64_t xb, int* infos, psd_bsylv_stats* stats, int* info) {
    return bsylv_cond_host<true>(c, nb, n, p, T, orient, schurindex, m, s, sep, X, xb, infos, stats, info);
}
int psd_d_subcond_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, char orient, int schurindex, const int* m,
                            double* s, double* sep, double* dX, int64_t xb, int* infos, psd_bsylv_stats* stats, int* info) {
    return bsylv_cond_dev<false>(c, nb, n, p, dT, orient, schurindex, m, s, sep, dX, xb, infos, stats, info);
}
int psd_z_subcond_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, char orient, int schurindex, const int* m,
                            double* s, double* sep, double* dX, int64_t xb, int* infos, psd_bsylv_stats* stats, int* info) {
    return bsylv_cond_dev<true>(c, nb, n, p, dT, orient, schurindex, m, s, sep, dX, xb, infos, stats, info);
}

}  // extern "C"
