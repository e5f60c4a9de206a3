// Host driver of psd_?_psylv[_dev] and psd_?_subcond[_dev] (psd_sylv.h): the periodic Sylvester solve and xTRSEN's two
// numbers for ONE periodic Schur form of any order.  Included behind psd_bsylv_host.inl, whose argument checks
// (bsylv_checked), small device arrays (bsylv_small), workspaces (bsylv_work) and condition group with the estimator loop
// (bsylv_cond_group) it shares; the host entries stage their matrices through batch_staged as a batch of one.
//
// One application of S^-1 or S^-H is the tiled walk: per anti-diagonal of tiles one psd_syl_update (none for the first)
// and one psd_syl_solve, nothing read back in between; the singular word is read once behind the last launch.  The
// condition entry applies it once for X and once per step of the estimator (at most 11 times), with one
// psd_bsyl_norms and one psd_bsyl_est_step per step as the batch entries.

namespace {

// Device time per kind of launch without a read-back between the launches: an event behind every launch, read when the
// application is complete (the serial simulation: the host clock).
struct sylv_marks {
    enum { SOLVE = 0, UPDATE = 1, NKIND = 2 };
    double ms[NKIND] = {0.0, 0.0};
#ifdef PSD_HOSTSIM
    std::chrono::steady_clock::time_point last;
    void begin(psd_stream_t) { last = std::chrono::steady_clock::now(); }
    void mark(psd_stream_t, int kind) {
        const auto t = std::chrono::steady_clock::now();
        ms[kind] += std::chrono::duration<double, std::milli>(t - last).count();
        last = t;
    }
    void collect() {}
#else
    std::vector<hipEvent_t> ev;
    std::vector<int> kinds;  // kinds[i]: what ran between ev[i] and ev[i + 1]
    size_t used = 0;
    sylv_marks() {}
    sylv_marks(const sylv_marks&) = delete;
    sylv_marks& operator=(const sylv_marks&) = delete;
    ~sylv_marks() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    void record(psd_stream_t s) {
        if (used == ev.size()) {
            hipEvent_t e = nullptr;
            (void)hipEventCreate(&e);
            ev.push_back(e);
        }
        (void)hipEventRecord(ev[used++], s);
    }
    void begin(psd_stream_t s) {
        collect();
        record(s);
    }
    void mark(psd_stream_t s, int kind) {
        record(s);
        kinds.push_back(kind);
    }
    void collect() {
        if (used == 0) return;
        (void)hipEventSynchronize(ev[used - 1]);
        for (size_t i = 0; i < kinds.size(); ++i) {
            float t = 0.f;
            (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]);
            ms[kinds[i]] += (double)t;
        }
        used = 0;
        kinds.clear();
    }
#endif
};

// boundaries 0 = b[0] < b[1] < ... = len at multiples of t; sub (may be null): sub[off + y - 1] != 0 where a boundary at y
// would cut a 2x2 block, which moves it to y + 1
std::vector<int> sylv_bounds(int len, int t, const double* sub, int off) {
    std::vector<int> b(1, 0);
    for (int x = t; x < len; x += t) {
        const int y = (sub && sub[off + x - 1] != 0.0) ? x + 1 : x;
        if (y < len) b.push_back(y);
    }
    b.push_back(len);
    return b;
}

struct sylv_plan {
    psd_ctx* c = nullptr;
    int n = 0, p = 0, m = 0, qsub = 0, nI = 0, nJ = 0, nsb = 1, napply = 0;
    bool left = false;
    psd_batchbuf bounds;  // rb [nI + 1] | cb [nJ + 1]
    psd_sylv_stats* st = nullptr;
    sylv_marks marks;
    bool trivial() const { return m == 0 || m == n; }
    const int* rb() const { return (const int*)bounds.ptr; }
    const int* cb() const { return rb() + nI + 1; }
};

// The partition of a form on the device; Float64: the sub-diagonal of the quasi-triangular factor comes back once, for
// the split check (-8) and the boundaries; tile: the width of the call (0: the context's)
template <bool CPLX>
int sylv_prepare(sylv_plan& pl, psd_ctx* c, int n, int p, const double* dT, char orient, int schurindex, int m,
                 psd_sylv_stats* st, int tile = 0, std::vector<int>* bounds_out = nullptr) {
    pl.c = c; pl.n = n; pl.p = p; pl.m = m; pl.qsub = schurindex - 1; pl.left = orient == 'L'; pl.st = st;
    const int t = tile > 0 ? tile : c->syl_tile;
    st->tile = t;
    if (pl.trivial()) return 0;
    std::vector<double> sub;
    if (!CPLX && n > 1) {
        psd_batchbuf dsub;
        PSD_CHECK(dsub.alloc(sizeof(double) * n));
        PSD_LAUNCH(psd_syl_subdiag, psd_dim3(1), 64, 0, c->stream, dT + (size_t)pl.qsub * n * n, dsub.d(), n);
        sub.resize(n);
        PSD_CHECK(psd_rt_d2h(sub.data(), dsub.d(), sizeof(double) * (n - 1), c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        PSD_CHECK(psd_rt_last_error());
        if (sub[m - 1] != 0.0) return -8;
    }
    const std::vector<int> rb = sylv_bounds(m, t, sub.empty() ? nullptr : sub.data(), 0);
    const std::vector<int> cb = sylv_bounds(n - m, t, sub.empty() ? nullptr : sub.data(), m);
    pl.nI = (int)rb.size() - 1;
    pl.nJ = (int)cb.size() - 1;
    pl.nsb = (t + 1 + PSD_SYL_UB - 1) / PSD_SYL_UB;  // (a tile is at most t + 1 wide)
    std::vector<int> both(rb);
    both.insert(both.end(), cb.begin(), cb.end());
    if (bounds_out) *bounds_out = both;
    PSD_CHECK(pl.bounds.alloc(sizeof(int) * both.size()));
    PSD_CHECK(psd_rt_h2d(pl.bounds.ptr, both.data(), sizeof(int) * both.size(), c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));  // (the host vector goes away)
    st->ntiles = pl.nI * pl.nJ;
    st->ndiag = pl.nI + pl.nJ - 1;
    return 0;
}

psd_syl_args sylv_args(const sylv_plan& pl, const double* dT, double* dX, int* dflag, int trans, int fromT, int d) {
    psd_syl_args g;
    g.T = dT; g.X = dX; g.rb = pl.rb(); g.cb = pl.cb(); g.flag = dflag;
    g.n = pl.n; g.p = pl.p; g.m = pl.m; g.qsub = pl.qsub; g.left = pl.left; g.trans = trans; g.fromT = fromT;
    g.nI = pl.nI; g.nJ = pl.nJ; g.d = d; g.nsb = pl.nsb;
    return g;
}

// the update launch of anti-diagonal g.d >= 1 (the walk, and the diagnostic entry psd_?_syl_update)
template <bool CPLX>
void sylv_launch_update(const sylv_plan& pl, const psd_syl_args& g) {
    const int nt = psd_syl_diag_tiles(pl.nI, pl.nJ, g.d);
    PSD_LAUNCH(psd_syl_update<CPLX>, psd_dim3(nt * pl.nsb * pl.nsb, pl.p), PSD_SYL_NT, 0, pl.c->stream, g);
}

// X := S^-1 X (trans: S^-H X), with fromT of -T12, by the tiled walk; dflag: the singular word.  Nothing is read back.
template <bool CPLX>
int sylv_apply(sylv_plan& pl, const double* dT, double* dX, int* dflag, int trans, int fromT) {
    psd_ctx* c = pl.c;
    psd_syl_args g = sylv_args(pl, dT, dX, dflag, trans, fromT, 0);
    const size_t lds = psd_bsyl_lds_bytes(pl.p, CPLX);
    PSD_CHECK(c->lds_limit(reinterpret_cast<const void*>(psd_syl_solve<CPLX>), lds));
    pl.napply += 1;
    pl.marks.begin(c->stream);
    for (int d = 0; d < pl.nI + pl.nJ - 1; ++d) {
        const int nt = psd_syl_diag_tiles(pl.nI, pl.nJ, d);
        g.d = d;
        if (d > 0) {  // (every tile behind the first anti-diagonal has a neighbour that is solved)
            g.fromT = fromT;
            sylv_launch_update<CPLX>(pl, g);
            pl.st->nupdate += 1;
            pl.marks.mark(c->stream, sylv_marks::UPDATE);
        }
        g.fromT = d == 0 ? fromT : 0;  // (the update has loaded -T12)
        PSD_LAUNCH(psd_syl_solve<CPLX>, psd_dim3(nt), 64, lds, c->stream, g);
        pl.st->nsolve += 1;
        pl.marks.mark(c->stream, sylv_marks::SOLVE);
    }
    return 0;
}

void sylv_times(sylv_plan& pl, double ms_all) {
    pl.marks.collect();
    pl.st->ms_solve = pl.marks.ms[sylv_marks::SOLVE];
    pl.st->ms_update = pl.marks.ms[sylv_marks::UPDATE];
    const double rest = ms_all - pl.st->ms_solve - pl.st->ms_update;
    pl.st->ms_est = rest > 0.0 ? rest : 0.0;
}

// psylv on the device: dC [p][m k] in / out
template <bool CPLX>
int sylv_psylv_core(sylv_plan& pl, const double* dT, double* dC, int trans, int fromT, int* code) {
    psd_ctx* c = pl.c;
    *code = 0;
    if (pl.trivial()) return 0;
    bsylv_small sm;
    PSD_CHECK(sm.alloc(1));
    PSD_CHECK(psd_rt_memset(sm.info, 0, sizeof(int), c->stream));
    if (int e = sylv_apply<CPLX>(pl, dT, dC, sm.info, trans, fromT)) return e;
    int flag = 0;
    PSD_CHECK(psd_rt_d2h(&flag, sm.info, sizeof(int), c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    sylv_times(pl, 0.0);
    if (flag != 0) {
        pl.st->nsingular = 1;
        *code = PSD_INFO_SINGULAR;
        return bsylv_fill_nan(c, dC, (size_t)(CPLX ? 2 : 1) * pl.m * (pl.n - pl.m) * pl.p);
    }
    return 0;
}

// subcond on the device: s [p], sep host; dX (may be null) receives X
template <bool CPLX>
int sylv_cond_core(sylv_plan& pl, const double* dT, double* dX, double* s, double* sep, int* code) {
    const size_t xb = (size_t)pl.m * (pl.n - pl.m);
    bsylv_work w;
    PSD_CHECK(w.alloc<CPLX>(1, pl.p, std::max<size_t>(xb, 1), !dX));
    const bsylv_call k{pl.c, pl.n, pl.p, pl.qsub, pl.left, xb};
    psd_bsylv_stats bst;
    memset(&bst, 0, sizeof(bst));
    const int rc = bsylv_cond_group<CPLX>(k, 1, dX ? dX : w.x.d(), dX != nullptr, &pl.m, w, s, sep, code, &bst,
                                          [&](double* X, const int* ptrans, int fromT, const std::vector<psd_bsyl_est>& rec) {
        return sylv_apply<CPLX>(pl, dT, X, w.sm.info, (ptrans && rec[0].kase == 2) ? 1 : 0, fromT);
    });
    sylv_times(pl, bst.ms_kernels);
    pl.st->nnorms = bst.nnorms;
    pl.st->nest_steps = bst.nest_steps;
    pl.st->nest_iter = bst.nest_iter;
    pl.st->nest_solves = pl.napply > 0 ? pl.napply - 1 : 0;
    pl.st->nsingular = bst.nsingular;
    return rc;
}

int sylv_head(const psd_ctx* c, bool cplx, int n, int p, const void* T, char orient, int schurindex, int m) {
    return bsylv_checked(c, cplx, 1, n, p, T, orient, schurindex, &m, false);
}

template <bool CPLX>
int sylv_psylv_dev(psd_ctx* c, int n, int p, const double* dT, char orient, int schurindex, int m, double* dC, int trans,
                   int from_t12, psd_sylv_stats* stats, int* info) {
    batch_call<psd_sylv_stats> entry(info, stats);
    if ((*info = sylv_head(c, CPLX, n, p, dT, orient, schurindex, m)) != 0) return *info;
    if (!dC) return *info = -9;
    sylv_plan pl;
    if ((*info = sylv_prepare<CPLX>(pl, c, n, p, dT, orient, schurindex, m, entry.s)) != 0) return *info;
    int code = 0;
    *info = sylv_psylv_core<CPLX>(pl, dT, dC, trans, from_t12, &code);
    return *info != 0 ? *info : (*info = code);
}

template <bool CPLX>
int sylv_psylv_host(psd_ctx* c, int n, int p, double* const* T, char orient, int schurindex, int m, double* const* Cm,
                    int trans, int from_t12, psd_sylv_stats* stats, int* info) {
    batch_call<psd_sylv_stats> entry(info, stats);
    if ((*info = sylv_head(c, CPLX, n, p, T, orient, schurindex, m)) != 0) return *info;
    if (!Cm) return *info = -9;
    constexpr int E = CPLX ? 2 : 1;
    const size_t bd = (size_t)E * n * n, cd = (size_t)E * m * (n - m);
    const batch_list L[] = {{T, p, bd, BATCH_IN}, {Cm, p, cd, (from_t12 ? 0 : BATCH_IN) | BATCH_OUT}};
    psd_stats copies;
    memset(&copies, 0, sizeof(copies));
    int code = 0;
    *info = batch_staged(c, 1, sizeof(double) * (bd + cd) * p + 64, L, &copies, batch_no_extra, [&](int, int, double* const* d) {
        sylv_plan pl;
        if (int e = sylv_prepare<CPLX>(pl, c, n, p, d[0], orient, schurindex, m, entry.s)) return e;
        return sylv_psylv_core<CPLX>(pl, d[0], d[1], trans, from_t12, &code);
    });
    entry.s->ms_copy = copies.ms_copy;
    return *info != 0 ? *info : (*info = code);
}

template <bool CPLX>
int sylv_cond_dev(psd_ctx* c, int n, int p, const double* dT, char orient, int schurindex, int m, double* s, double* sep,
                  double* dX, psd_sylv_stats* stats, int* info) {
    batch_call<psd_sylv_stats> entry(info, stats);
    if ((*info = sylv_head(c, CPLX, n, p, dT, orient, schurindex, m)) != 0) return *info;
    if (!s || !sep) return *info = -9;
    sylv_plan pl;
    if ((*info = sylv_prepare<CPLX>(pl, c, n, p, dT, orient, schurindex, m, entry.s)) != 0) return *info;
    int code = 0;
    *info = sylv_cond_core<CPLX>(pl, dT, dX, s, sep, &code);
    return *info != 0 ? *info : (*info = code);
}

template <bool CPLX>
int sylv_cond_host(psd_ctx* c, int n, int p, double* const* T, char orient, int schurindex, int m, double* s, double* sep,
                   double* const* X, psd_sylv_stats* stats, int* info) {
    batch_call<psd_sylv_stats> entry(info, stats);
    if ((*info = sylv_head(c, CPLX, n, p, T, orient, schurindex, m)) != 0) return *info;
    if (!s || !sep) return *info = -9;
    constexpr int E = CPLX ? 2 : 1;
    const size_t bd = (size_t)E * n * n, cd = (size_t)E * m * (n - m);
    const batch_list L[] = {{T, p, bd, BATCH_IN}, {X, p, cd, BATCH_OUT}};
    psd_stats copies;
    memset(&copies, 0, sizeof(copies));
    int code = 0;
    *info = batch_staged(c, 1, sizeof(double) * (bd + 3 * cd) * p + 64, L, &copies, batch_no_extra,
                         [&](int, int, double* const* d) {
        sylv_plan pl;
        if (int e = sylv_prepare<CPLX>(pl, c, n, p, d[0], orient, schurindex, m, entry.s)) return e;
        return sylv_cond_core<CPLX>(pl, d[0], X ? d[1] : nullptr, s, sep, &code);
    });
    entry.s->ms_copy = copies.ms_copy;
    return *info != 0 ? *info : (*info = code);
}

// ---- diagnostic entry of the update kernel (test plumbing; include/psd_mi355x.h) -------------------------------------
// the checks and the partition of the walk at the width `tile`, then the update launch of anti-diagonal d alone, on host
// blocks staged as those of psd_?_psylv
template <bool CPLX>
int sylv_update_host(psd_ctx* c, int n, int p, double* const* T, char orient, int schurindex, int m, double* const* X,
                     int tile, int d, int trans, int from_t12, psd_syl_geom* geom, int32_t* bounds, int* info) {
    batch_call<psd_sylv_stats> entry(info, nullptr);
    if ((*info = sylv_head(c, CPLX, n, p, T, orient, schurindex, m)) != 0) return *info;
    if (!X) return *info = -9;
    if (tile < PSD_SYL_TILE_MIN || tile > PSD_SYL_TILE_MAX) return *info = -10;
    constexpr int E = CPLX ? 2 : 1;
    const size_t bd = (size_t)E * n * n, cd = (size_t)E * m * (n - m);
    const batch_list L[] = {{T, p, bd, BATCH_IN}, {X, p, cd, BATCH_IN | BATCH_OUT}};
    return *info = batch_staged(c, 1, sizeof(double) * (bd + cd) * p + 64, L, nullptr, batch_no_extra,
                                [&](int, int, double* const* dv) {
        sylv_plan pl;
        std::vector<int> both;
        if (int e = sylv_prepare<CPLX>(pl, c, n, p, dv[0], orient, schurindex, m, entry.s, tile, &both)) return e;
        if (geom) {
            geom->nI = pl.nI;
            geom->nJ = pl.nJ;
            geom->nsb = pl.nsb;
            geom->ndtiles = 0;
        }
        if (d < 1 || d > pl.nI + pl.nJ - 2) return -11;  // (the trivial splits have no anti-diagonal at all)
        if (geom) geom->ndtiles = psd_syl_diag_tiles(pl.nI, pl.nJ, d);
        if (bounds) std::copy(both.begin(), both.end(), bounds);
        bsylv_small sm;
        PSD_CHECK(sm.alloc(1));
        PSD_CHECK(psd_rt_memset(sm.info, 0, sizeof(int), c->stream));
        sylv_launch_update<CPLX>(pl, sylv_args(pl, dv[0], dv[1], sm.info, trans != 0, from_t12 != 0, d));
        PSD_CHECK(psd_rt_sync(c->stream));
        PSD_CHECK(psd_rt_last_error());
        return 0;
    });
}

}  // namespace

extern "C" {

int psd_d_psylv(psd_ctx* c, int n, int p, double* const* T, char orient, int schurindex, int m, double* const* C, int trans,
                int from_t12, psd_sylv_stats* stats, int* info) {
    return sylv_psylv_host<false>(c, n, p, T, orient, schurindex, m, C, trans, from_t12, stats, info);
}
int psd_z_psylv(psd_ctx* c, int n, int p, double* const* T, char orient, int schurindex, int m, double* const* C, int trans,
                int from_t12, psd_sylv_stats* stats, int* info) {
    return sylv_psylv_host<true>(c, n, p, T, orient, schurindex, m, C, trans, from_t12, stats, info);
}
int psd_d_psylv_dev(psd_ctx* c, int n, int p, const double* dT, char orient, int schurindex, int m, double* dC, int trans,
                    int from_t12, psd_sylv_stats* stats, int* info) {
    return sylv_psylv_dev<false>(c, n, p, dT, orient, schurindex, m, dC, trans, from_t12, stats, info);
}
int psd_z_psylv_dev(psd_ctx* c, int n, int p, const double* dT, char orient, int schurindex, int m, double* dC, int trans,
                    int from_t12, psd_sylv_stats* stats, int* info) {
    return sylv_psylv_dev<true>(c, n, p, dT, orient, schurindex, m, dC, trans, from_t12, stats, info);
}

int psd_d_subcond(psd_ctx* c, int n, int p, double* const* T, char orient, int schurindex, int m, double* s, double* sep,
                  double* const* X, psd_sylv_stats* stats, int* info) {
    return sylv_cond_host<false>(c, n, p, T, orient, schurindex, m, s, sep, X, stats, info);
}
int psd_z_subcond(psd_ctx* c, int n, int p, double* const* T, char orient, int schurindex, int m, double* s, double* sep,
                  double* const* X, psd_sylv_stats* stats, int* info) {
    return sylv_cond_host<true>(c, n, p, T, orient, schurindex, m, s, sep, X, stats, info);
}
int psd_d_subcond_dev(psd_ctx* c, int n, int p, const double* dT, char orient, int schurindex, int m, double* s, double* sep,
                      double* dX, psd_sylv_stats* stats, int* info) {
    return sylv_cond_dev<false>(c, n, p, dT, orient, schurindex, m, s, sep, dX, stats, info);
}
int psd_z_subcond_dev(psd_ctx* c, int n, int p, const double* dT, char orient, int schurindex, int m, double* s, double* sep,
                      double* dX, psd_sylv_stats* stats, int* info) {
    return sylv_cond_dev<true>(c, n, p, dT, orient, schurindex, m, s, sep, dX, stats, info);
}

int psd_d_syl_update(psd_ctx* c, int n, int p, double* const* T, char orient, int schurindex, int m, double* const* X,
                     int tile, int d, int trans, int from_t12, psd_syl_geom* geom, int32_t* bounds, int* info) {
    return sylv_update_host<false>(c, n, p, T, orient, schurindex, m, X, tile, d, trans, from_t12, geom, bounds, info);
}
int psd_z_syl_update(psd_ctx* c, int n, int p, double* const* T, char orient, int schurindex, int m, double* const* X,
                     int tile, int d, int trans, int from_t12, psd_syl_geom* geom, int32_t* bounds, int* info) {
    return sylv_update_host<true>(c, n, p, T, orient, schurindex, m, X, tile, d, trans, from_t12, geom, bounds, info);
}

}  // extern "C"
