// Host drivers of psd_d_ordschur_batch / psd_d_ordschur_batch_dev (psd_bord.h): ordschur!(P, select) for nb periodic Schur
// forms of one shape, as psd_d_pschur_batch leaves them.  Included at the end of psd_engine.cpp behind psd_batch_host.inl
// (psd_batchbuf, batch_group, batch_alloc_halving, batch_staged).
//
// The first part is what the three reorder families share (psd_zbord_host.inl and psd_zgbord_host.inl come in behind this
// file): the description of a call (bord_call, bord_vals), the argument checks, the fallback loop over single calls, the
// codes and counters of a launched group, the device permutations and the bodies of the two kinds of entry.  A family is a
// type with the members of bord_real below.
//
// The real family, per group of problems: the selections go up once, then psd_bord — every problem's whole reordering in
// one launch —, psd_bord_values and psd_bord_cleanup, and one read-back of the per-problem states, codes and eigenvalues.
// Orders above PSD_BORD_NMAX, and periods whose narrowest window does not fit the LDS, run rordschur_dev problem by problem
// on the slices of the batch buffers.

namespace {

// The eigenvalue rows of a reorder call and their per-problem strides: wr, wi of the real family (sc null); alpha (complex
// pairs), beta, ascale of the complex ones
struct bord_vals {
    double* a;
    double* b;
    int32_t* sc;
    bord_vals at(size_t q, int n) const { return {a + (sc ? 2 : 1) * q * n, b + q * n, sc ? sc + q * n : nullptr}; }
};

// A reorder call behind its checks, or (at) the rows of its problems from q0 on.  S: the signature of a signed call in the
// internal order (host, p flags), otherwise null; select, v, infos, nswaps (may be null): host rows; the groups add to s
struct bord_call {
    psd_ctx* c;
    int n, p, wantZ;
    const uint8_t* S;
    const uint8_t* select;
    bord_vals v;
    int* infos;
    int* nswaps;
    psd_stats* s;
    bord_call at(size_t q0) const {
        return {c, n, p, wantZ, S, select + q0 * n, v.at(q0, n), infos + q0, nswaps ? nswaps + q0 : nullptr, s};
    }
};

// The fallback of every family: single(q, &ps) runs the single-problem driver on problem q of a group of gc; its code is
// the problem's unless it ends the call, and what it counted and timed is added to the call's
template <class Single>
int bord_single_loop(const bord_call& k, int gc, Single single) {
    for (int q = 0; q < gc; ++q) {
        psd_stats ps;
        memset(&ps, 0, sizeof(ps));
        const int rc = single(q, &ps);
        if (batch_fatal(rc)) return rc;
        k.infos[q] = rc;
        if (k.nswaps) k.nswaps[q] = ps.nsweeps;
        k.s->nsweeps += ps.nsweeps;
        k.s->nwindows += ps.nwindows;
        k.s->nlaunch_step += ps.nlaunch_step;
        k.s->window = ps.window;
        k.s->ms_iter += ps.ms_iter;
        k.s->ms_total += ps.ms_total;
    }
    return 0;
}

// What the launches of a group (window W, ms on the device) left in the states hst of its problems (psd_rostate,
// psd_ostate): the codes — 0, 2000 + row (IllConditionedException), 3000 (SingularException); `giveup` ends the call with
// `fatal` —, the swaps and the counters.  keep(q) copies the eigenvalues of a problem whose code is 0.
template <class State, class Keep>
int bord_collect(const bord_call& k, const std::vector<State>& hst, int giveup, int fatal, int W, double ms, Keep keep) {
    for (size_t q = 0; q < hst.size(); ++q) {
        if (hst[q].info == giveup) return fatal;
        k.infos[q] = hst[q].info;
        if (k.nswaps) k.nswaps[q] = hst[q].nswaps;
        if (hst[q].info == 0) keep(q);
        k.s->nsweeps += hst[q].nswaps;
        k.s->nwindows += hst[q].nwindows;
    }
    k.s->nlaunch_step += 1;
    k.s->window = W;
    k.s->ms_iter += ms;
    k.s->ms_total += ms;
    return 0;
}

int bord_checked(psd_ctx* c, int nb, int n, int p, const void* T, const void* Z, char orient, int schurindex,
                 const uint8_t* select, int wantZ, const double* wr, const double* wi, std::vector<int>& slotA,
                 std::vector<int>& slotZ) {
    if (!c) return -1;
    if (n < 1) return -2;
    if (p < 1) return -3;
    if (nb < 0) return -11;
    if (nb == 0) return 0;
    if (!T) return -4;
    if (wantZ && !Z) return -5;
    if (orient != 'R' && orient != 'L') return -6;
    if (!ord_slots(orient, schurindex, p, slotA, slotZ)) return -7;  // rordschur.jl:25
    if (!select) return -8;
    if (!wr || !wi) return -9;
    if (c->shard_world > 1) return PSD_INFO_NOTIMPL;  // (a period-sharded context keeps a slice of Z: single problems only)
    return 0;
}

bool bord_identity(const std::vector<int>& slot) {
    for (size_t j = 0; j < slot.size(); ++j)
        if (slot[j] != (int)j) return false;
    return true;
}
// slot is the reversal of the cnt blocks from `first` on and the identity before them
bool bord_reversal(const std::vector<int>& slot, int first) {
    const int p = (int)slot.size();
    for (int j = 0; j < p; ++j)
        if (slot[j] != (j < first ? j : p - 1 - (j - first))) return false;
    return true;
}

// The [nb][p] blocks of X between the user order and the internal order, in place where the permutation is its own
// inverse (the reversals of psd_d_pschur_batch's 'L' results: psd_breverse_blocks), otherwise gt problems at a time
// through tmp [gt][p][nn] (gt == 0: not allocated yet; a group that fits the free memory, halved until it does)
int bord_permute_dev(psd_ctx* c, int nb, int p, size_t nn, double* X, const std::vector<int>& slot, int first, bool to_internal,
                     psd_batchbuf& tmp, int& gt, psd_batchbuf& dslot) {
    if (bord_identity(slot)) return 0;
    if (bord_reversal(slot, first)) {
        const int cnt = p - first;
        if (cnt >= 2) PSD_LAUNCH(psd_breverse_blocks, psd_dim3(nb * (cnt / 2)), PSD_HESS_NT, 0, c->stream, X, nn, p, first, cnt);
        return 0;
    }
    const size_t per = sizeof(double) * nn * p;
    if (gt == 0) {
        int g = batch_group(c, nb, per);
        if (int e = batch_alloc_halving(g, [&](int gg) { return tmp.alloc(per * gg); })) return e;
        gt = g;
    }
    PSD_CHECK(dslot.alloc(sizeof(int) * (size_t)p));
    PSD_CHECK(psd_rt_h2d(dslot.ptr, slot.data(), sizeof(int) * (size_t)p, c->stream));
    for (int q0 = 0; q0 < nb; q0 += gt) {
        const int gc = (nb - q0 < gt) ? (nb - q0) : gt;
        double* Xg = X + (size_t)q0 * p * nn;
        PSD_LAUNCH(psd_bord_permute, psd_dim3(gc * p), PSD_HESS_NT, 0, c->stream, tmp.d(), (const double*)Xg,
                   (const int*)dslot.ptr, nn, p, to_internal ? 1 : 0);
        PSD_CHECK(psd_rt_d2d(Xg, tmp.d(), per * gc, c->stream));
    }
    PSD_CHECK(psd_rt_sync(c->stream));  // (dslot is reused)
    return 0;
}

// The device-resident entry of a family F behind its checks: nb problems in dT / dZ (used with wantZ) [nb][p] blocks in
// the user order.  The factors stay where they are: to the internal order, groups of what the workspace allows through
// F::group — ws.alloc(g, n, p) in the halving loop unless the call takes the fallback —, and back to the user order.
template <class F>
int bord_entry_dev(const bord_call& k, int nb, void* dT, void* dZ, const std::vector<int>& slotA, const std::vector<int>& slotZ) {
    psd_ctx* c = k.c;
    const int n = k.n, p = k.p;
    const size_t bd = F::ed * (size_t)n * n;
    double* H = (double*)dT;
    double* Z = k.wantZ ? (double*)dZ : nullptr;
    typename F::ws_t ws;
    int g = batch_group(c, nb, F::ws_bytes(n, p));
    if (!F::fallback(c, n, p))
        if (int e = batch_alloc_halving(g, [&](int gg) { return ws.alloc(gg, n, p); })) return e;
    psd_batchbuf tmp, dslot;
    int gt = 0;
    const int firstZ = (slotZ[0] == 0) ? 1 : 0;
    if (int e = bord_permute_dev(c, nb, p, bd, H, slotA, 0, true, tmp, gt, dslot)) return e;
    if (Z)
        if (int e = bord_permute_dev(c, nb, p, bd, Z, slotZ, firstZ, true, tmp, gt, dslot)) return e;
    int fatal = 0;
    for (int q0 = 0; q0 < nb && fatal == 0; q0 += g)
        fatal = F::group(k.at(q0), (nb - q0 < g) ? (nb - q0) : g, H + (size_t)q0 * p * bd, Z ? Z + (size_t)q0 * p * bd : nullptr,
                         ws);
    // back to the user order, also behind a runtime failure: the caller's blocks keep their places
    int rc = bord_permute_dev(c, nb, p, bd, H, slotA, 0, false, tmp, gt, dslot);
    if (rc == 0 && Z) rc = bord_permute_dev(c, nb, p, bd, Z, slotZ, firstZ, false, tmp, gt, dslot);
    if (rc == 0) rc = psd_rt_sync(c->stream) != 0 ? PSD_INFO_RUNTIME + 1 : 0;
    if (fatal != 0) return fatal;
    if (rc != 0) return rc;
    return batch_first_code(k.infos, nb);
}

// The host entry of a family F behind its checks: user slot <-> internal slot on the way through the staging buffer, as
// the single-problem entries copy
template <class F>
int bord_entry_host(const bord_call& k, int nb, double* const* T, double* const* Z, const std::vector<int>& slotA,
                    const std::vector<int>& slotZ) {
    psd_ctx* c = k.c;
    const int n = k.n, p = k.p;
    const size_t bd = F::ed * (size_t)n * n;
    const batch_list L[] = {{T, p, bd, BATCH_IN | BATCH_OUT, slotA.data()},
                            {k.wantZ ? Z : nullptr, p, bd, BATCH_IN | BATCH_OUT, slotZ.data()}};
    typename F::ws_t ws;
    auto extra = [&](int g) { return F::fallback(c, n, p) ? 0 : ws.alloc(g, n, p); };
    auto body = [&](int q0, int gc, double* const* d) { return F::group(k.at(q0), gc, d[0], d[1], ws); };
    const int rc = batch_staged(c, nb, sizeof(double) * (k.wantZ ? 2 : 1) * bd * p + F::ws_bytes(n, p), L, k.s, extra, body);
    return rc != 0 ? rc : batch_first_code(k.infos, nb);
}

// ------------------------------------------------------------------------------------------------
// the real family

struct bord_real {
    static constexpr int ed = 1;  // doubles of a matrix element

    // Window of the batched kernel: the smallest candidate of choose_window_rord's list that holds the whole problem if
    // its LDS fits, otherwise the widest that fits (0: none), and no wider than the longest span psd_bord gives a window
    // (PSD_BORD_SPAN1: the LDS of rows that no window reaches would only keep other problems off the CU); PSD_BORD_W
    // narrows it
    static int window(const psd_ctx* c, int n, int p) {
        int W = choose_window_rord(p, n);
        if (W > PSD_BORD_SPAN1) W = PSD_BORD_SPAN1;
        if (W != 0 && c->bord_w >= PSD_BORD_WMIN && c->bord_w < W) W = c->bord_w;
        return W;
    }
    static bool fallback(const psd_ctx* c, int n, int p) { return n > c->bord_nmax || window(c, n, p) == 0; }

    // device workspace of one problem besides its factors
    static size_t ws_bytes(int n, int p) {
        return sizeof(psd_rostate) + sizeof(psd_apply_desc) + sizeof(psd_tq) * (size_t)p * PSD_RORD_CAP +
               sizeof(int) * (size_t)(p + 1) + (size_t)n + sizeof(double) * (2 * (size_t)n + 8 * (size_t)n * p);
    }
    struct ws_t {
        psd_batchbuf st, desc, tq, cnt, sel, wr, wi, xscr, infos;
        int alloc(int g, int n, int p) {
            PSD_CHECK(st.alloc(sizeof(psd_rostate) * (size_t)g));
            PSD_CHECK(desc.alloc(sizeof(psd_apply_desc) * (size_t)g));
            PSD_CHECK(tq.alloc(sizeof(psd_tq) * (size_t)g * p * PSD_RORD_CAP));
            PSD_CHECK(cnt.alloc(sizeof(int) * (size_t)g * p));
            PSD_CHECK(sel.alloc((size_t)g * n));
            PSD_CHECK(wr.alloc(sizeof(double) * (size_t)g * n));
            PSD_CHECK(wi.alloc(sizeof(double) * (size_t)g * n));
            PSD_CHECK(xscr.alloc(sizeof(double) * 8 * (size_t)g * n * p));
            PSD_CHECK(infos.alloc(sizeof(int) * (size_t)g));
            return 0;
        }
    };

    // gc problems resident on the device in the internal order (dH, dZ [gc][p][n][n]) and their rows k.  wr / wi of a
    // problem whose code is non-zero are not written.
    static int group(const bord_call& k, int gc, double* dH, double* dZ, ws_t& ws) {
        psd_ctx* c = k.c;
        const int n = k.n, p = k.p;
        const size_t nn = (size_t)n * n;
        if (fallback(c, n, p)) {
            if (int e = c->reserve(n, p, false, 16)) return e;
            std::vector<double> lr(n), li(n);
            return bord_single_loop(k, gc, [&](int q, psd_stats* ps) {
                int pinfo = 0;
                const int rc = rordschur_dev(c, n, p, dH + (size_t)q * p * nn, k.wantZ ? dZ + (size_t)q * p * nn : nullptr,
                                             k.select + (size_t)q * n, k.wantZ, lr.data(), li.data(), ps, &pinfo);
                if (rc == 0) {
                    memcpy(k.v.a + (size_t)q * n, lr.data(), sizeof(double) * n);
                    memcpy(k.v.b + (size_t)q * n, li.data(), sizeof(double) * n);
                }
                return rc;
            });
        }
        const int W = window(c, n, p);
        const size_t lds = rord_lds_bytes(p, W);
        PSD_CHECK(c->lds_limit(reinterpret_cast<const void*>(psd_bord), lds));
        PSD_CHECK(psd_rt_h2d(ws.sel.ptr, k.select, (size_t)gc * n, c->stream));
        psd_bord_args a;
        a.H = dH;
        a.Z = k.wantZ ? dZ : nullptr;
        a.st = (psd_rostate*)ws.st.ptr;
        a.desc = (psd_apply_desc*)ws.desc.ptr;
        a.tq = (psd_tq*)ws.tq.ptr;
        a.cnt = (int*)ws.cnt.ptr;
        a.select = (const unsigned char*)ws.sel.ptr;
        a.wr = ws.wr.d();
        a.wi = ws.wi.d();
        a.xscr = ws.xscr.d();
        a.infos = (int*)ws.infos.ptr;
        a.n = n; a.p = p; a.wantZ = k.wantZ; a.W = W;
        a.maxwin = 2 * n * (n + 2) + 1024;  // (a block moves up by a row or more per window, and at most n blocks move)
        Timer t;
        t.start(c->stream);
        PSD_LAUNCH(psd_bord, psd_dim3(gc), PSD_STEP_NT, lds, c->stream, a);
        PSD_LAUNCH(psd_bord_values, psd_dim3((n + 63) / 64, gc), 64, 0, c->stream, a);
        PSD_LAUNCH(psd_bord_cleanup, psd_dim3(n, gc), 64, 0, c->stream, a);
        const double ms = t.stop(c->stream);
        std::vector<psd_rostate> hst(gc);
        std::vector<double> hw(2 * (size_t)gc * n);
        PSD_CHECK(psd_rt_d2h(hst.data(), ws.st.ptr, sizeof(psd_rostate) * (size_t)gc, c->stream));
        PSD_CHECK(psd_rt_d2h(hw.data(), ws.wr.ptr, sizeof(double) * (size_t)gc * n, c->stream));
        PSD_CHECK(psd_rt_d2h(hw.data() + (size_t)gc * n, ws.wi.ptr, sizeof(double) * (size_t)gc * n, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        PSD_CHECK(psd_rt_last_error());
        return bord_collect(k, hst, PSD_LIST_OVERFLOW, PSD_INFO_RUNTIME + 77, W, ms, [&](size_t q) {
            memcpy(k.v.a + q * n, hw.data() + q * n, sizeof(double) * n);
            memcpy(k.v.b + q * n, hw.data() + (gc + q) * n, sizeof(double) * n);
        });
    }
};

}  // namespace

extern "C" {

int psd_d_ordschur_batch_dev(psd_ctx* c, int nb, int n, int p, void* dT, void* dZ, char orient, int schurindex,
                             const uint8_t* select, int wantZ, double* wr, double* wi, int* infos, int* nswaps,
                             psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    std::vector<int> slotA, slotZ;
    if ((*info = bord_checked(c, nb, n, p, dT, dZ, orient, schurindex, select, wantZ, wr, wi, slotA, slotZ)) != 0 || nb == 0)
        return *info;
    const bord_call call{c, n, p, wantZ, nullptr, select, {wr, wi, nullptr}, k.infos(infos, nb), nswaps, k.s};
    return *info = bord_entry_dev<bord_real>(call, nb, dT, dZ, slotA, slotZ);
}

int psd_d_ordschur_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, char orient, int schurindex,
                         const uint8_t* select, int wantZ, double* wr, double* wi, int* infos, int* nswaps, psd_stats* stats,
                         int* info) {
    batch_call<psd_stats> k(info, stats);
    std::vector<int> slotA, slotZ;
    if ((*info = bord_checked(c, nb, n, p, T, Z, orient, schurindex, select, wantZ, wr, wi, slotA, slotZ)) != 0 || nb == 0)
        return *info;
    const bord_call call{c, n, p, wantZ, nullptr, select, {wr, wi, nullptr}, k.infos(infos, nb), nswaps, k.s};
    return *info = bord_entry_host<bord_real>(call, nb, T, Z, slotA, slotZ);
}

}  // extern "C"
