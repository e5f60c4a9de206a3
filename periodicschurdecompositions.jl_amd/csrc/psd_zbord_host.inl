// Host drivers of psd_z_ordschur_batch / psd_z_ordschur_batch_dev (psd_zbord.h): ordschur!(P, select) for nb ComplexF64
// periodic Schur forms of one shape, as psd_z_pschur_batch leaves them.  Included at the end of psd_engine.cpp behind
// psd_bord_host.inl, whose call description, argument checks, fallback loop, code collection, device permutations and
// entry bodies it shares (a complex matrix travels as 2 n^2 doubles).
//
// zbord_family is the one group path of both complex families; a description (zbord_unsigned here, zgbord_signed in
// psd_zgbord_host.inl) names what differs between them.  Per group of problems: the selections go up once, then the
// family's reorder kernel (psd_zbord) — every problem's whole reordering in one launch — and its values kernel
// (psd_zbord_values), and one read-back of the per-problem states, codes and scaled eigenvalues.  Orders above
// PSD_BORD_NMAX, and periods whose narrowest window does not fit the LDS, run the single-problem driver (zordschur_dev)
// problem by problem on the slices of the batch buffers.

namespace {

// The reorder family of a description D:
//   args_t                 the argument struct of the two kernels (its st and desc members give the state and descriptor)
//   trcap, wmin, giveup    the transform-list cap, the least window PSD_BORD_W may ask for, the state code of a run
//                          that does not end
//   has_sig                the call has a signature: one more buffer, uploaded per group into args_t::S
//   window_lds(p, w), apply_lds(W)   the LDS bytes of the windows and of the apply phase
//   reserve(c, n, p)       what the single-problem driver needs of the context
//   single(...)            that driver on one problem
//   kernel(), launch(c, gc, n, lds, a)   the reorder kernel, and the launches of a group
template <class D>
struct zbord_family {
    using args_t = typename D::args_t;
    using state_t = typename std::remove_pointer<decltype(args_t::st)>::type;
    using desc_t = typename std::remove_pointer<decltype(args_t::desc)>::type;
    static constexpr int ed = 2;  // doubles of a matrix element

    // Window of the batched kernel: the single driver's choice, narrowed to the smallest candidate that still holds the
    // whole problem when one does (the windows stay the same ones — a window never reaches above row 1 — and less LDS per
    // workgroup lets more problems share a CU); 0: none fits.  PSD_BORD_W narrows it further.
    static int window(const psd_ctx* c, int n, int p) {
        int W = choose_window_lds({32, 24, 20, 16, 12, 10, 8, 6, 4}, [&](int w) { return D::window_lds(p, w); }, n);
        if (W != 0 && c->bord_w >= D::wmin && c->bord_w < W) W = c->bord_w;
        return W;
    }
    static bool fallback(const psd_ctx* c, int n, int p) { return n > c->bord_nmax || window(c, n, p) == 0; }

    // device workspace of one problem besides its factors
    static size_t ws_bytes(int n, int p) {
        return sizeof(state_t) + sizeof(desc_t) + sizeof(psd_ztr) * (size_t)p * D::trcap + sizeof(int) * (size_t)(p + 1) +
               (size_t)n + (sizeof(psd_z) + sizeof(double) + sizeof(int)) * (size_t)n;
    }
    // (S: the signature of a signed call in the internal order, p flags)
    struct ws_t {
        psd_batchbuf st, desc, tr, cnt, sel, alpha, beta, ascale, infos, S;
        int alloc(int g, int n, int p) {
            PSD_CHECK(st.alloc(sizeof(state_t) * (size_t)g));
            PSD_CHECK(desc.alloc(sizeof(desc_t) * (size_t)g));
            PSD_CHECK(tr.alloc(sizeof(psd_ztr) * (size_t)g * p * D::trcap));
            PSD_CHECK(cnt.alloc(sizeof(int) * (size_t)g * p));
            PSD_CHECK(sel.alloc((size_t)g * n));
            PSD_CHECK(alpha.alloc(sizeof(psd_z) * (size_t)g * n));
            PSD_CHECK(beta.alloc(sizeof(double) * (size_t)g * n));
            PSD_CHECK(ascale.alloc(sizeof(int) * (size_t)g * n));
            PSD_CHECK(infos.alloc(sizeof(int) * (size_t)g));
            if (D::has_sig) PSD_CHECK(S.alloc((size_t)p + 16));
            return 0;
        }
    };

    // gc problems resident on the device in the internal order (dH, dZ [gc][p][n][n] complex) and their rows k.  The
    // eigenvalue rows of a problem whose code is non-zero are not written.
    static int group(const bord_call& k, int gc, double* dH, double* dZ, ws_t& ws) {
        psd_ctx* c = k.c;
        const int n = k.n, p = k.p;
        psd_z* H = (psd_z*)dH;
        psd_z* Z = k.wantZ ? (psd_z*)dZ : nullptr;
        if (fallback(c, n, p)) {
            if (int e = D::reserve(c, n, p)) return e;
            return bord_single_loop(k, gc, [&](int q, psd_stats* ps) {
                const size_t o = (size_t)q * p * n * n;
                const bord_vals v = k.v.at(q, n);
                int pinfo = 0;
                // (the eigenvalues come down only behind a run that ended with code 0)
                return D::single(c, n, p, H + o, Z ? Z + o : nullptr, k.S, k.select + (size_t)q * n, k.wantZ, v.a, v.b, v.sc, ps,
                                 &pinfo);
            });
        }
        const int W = window(c, n, p);
        const size_t lds = std::max(D::window_lds(p, W), D::apply_lds(W));
        PSD_CHECK(c->lds_limit(D::kernel(), lds));
        PSD_CHECK(psd_rt_h2d(ws.sel.ptr, k.select, (size_t)gc * n, c->stream));
        args_t a;
        if constexpr (D::has_sig) {
            PSD_CHECK(psd_rt_h2d(ws.S.ptr, k.S, (size_t)p, c->stream));
            a.S = (const unsigned char*)ws.S.ptr;
        }
        a.H = H;
        a.Z = Z;
        a.st = (state_t*)ws.st.ptr;
        a.desc = (desc_t*)ws.desc.ptr;
        a.tr = (psd_ztr*)ws.tr.ptr;
        a.cnt = (int*)ws.cnt.ptr;
        a.select = (const unsigned char*)ws.sel.ptr;
        a.alpha = (psd_z*)ws.alpha.ptr;
        a.beta = ws.beta.d();
        a.ascale = (int*)ws.ascale.ptr;
        a.infos = (int*)ws.infos.ptr;
        a.n = n; a.p = p; a.wantZ = k.wantZ; a.W = W;
        a.maxwin = n * (n + 2) + 1024;  // (a selected eigenvalue moves up by a row or more per window, and at most n of them move)
        Timer t;
        t.start(c->stream);
        D::launch(c, gc, n, lds, a);
        const double ms = t.stop(c->stream);
        const size_t gn = (size_t)gc * n;
        std::vector<state_t> hst(gc);
        std::vector<psd_z> ha(gn);
        std::vector<double> hb(gn);
        std::vector<int> hsc(gn);
        PSD_CHECK(psd_rt_d2h(hst.data(), ws.st.ptr, sizeof(state_t) * (size_t)gc, c->stream));
        PSD_CHECK(psd_rt_d2h(ha.data(), ws.alpha.ptr, sizeof(psd_z) * gn, c->stream));
        PSD_CHECK(psd_rt_d2h(hb.data(), ws.beta.ptr, sizeof(double) * gn, c->stream));
        PSD_CHECK(psd_rt_d2h(hsc.data(), ws.ascale.ptr, sizeof(int) * gn, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        PSD_CHECK(psd_rt_last_error());
        // (0xfffd: the single drivers' code of a run that does not end)
        return bord_collect(k, hst, D::giveup, PSD_INFO_RUNTIME + 0xfffd, W, ms, [&](size_t q) {
            const bord_vals v = k.v.at(q, n);
            memcpy(v.a, ha.data() + q * n, sizeof(psd_z) * n);
            memcpy(v.b, hb.data() + q * n, sizeof(double) * n);
            for (int j = 0; j < n; ++j) v.sc[j] = hsc[q * n + j];
        });
    }
};

struct zbord_unsigned {
    using args_t = psd_zbord_args;
    static constexpr int trcap = PSD_ZTR_CAP, wmin = PSD_ZBORD_WMIN, giveup = PSD_ZBORD_WINCAP;
    static constexpr bool has_sig = false;
    static size_t window_lds(int p, int w) { return ord_lds_bytes(p, w); }
    static size_t apply_lds(int W) { return psd_zbqz_apply_lds_bytes(W); }
    static int reserve(psd_ctx* c, int n, int p) { return c->zreserve(n, p, false, 16); }
    static int single(psd_ctx* c, int n, int p, psd_z* H, psd_z* Z, const uint8_t*, const uint8_t* select, int wantZ,
                      double* alpha, double* beta, int32_t* ascale, psd_stats* ps, int* pinfo) {
        return zordschur_dev(c, n, p, H, Z, select, wantZ, alpha, beta, ascale, ps, pinfo);
    }
    static const void* kernel() { return reinterpret_cast<const void*>(psd_zbord); }
    static void launch(psd_ctx* c, int gc, int n, size_t lds, const args_t& a) {
        PSD_LAUNCH(psd_zbord, psd_dim3(gc), PSD_STEP_NT, lds, c->stream, a);
        PSD_LAUNCH(psd_zbord_values, psd_dim3((n + 63) / 64, gc), 64, 0, c->stream, a);
    }
};
using zbord_plain = zbord_family<zbord_unsigned>;

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
    const bord_call call{c, n, p, wantZ, nullptr, select, {alpha, beta, ascale}, k.infos(infos, nb), nswaps, k.s};
    return *info = bord_entry_dev<zbord_plain>(call, nb, dT, dZ, slotA, slotZ);
}

int psd_z_ordschur_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, char orient, int schurindex,
                         const uint8_t* select, int wantZ, double* alpha, double* beta, int32_t* ascale, int* infos,
                         int* nswaps, psd_stats* stats, int* info) {
    batch_call<psd_stats> k(info, stats);
    std::vector<int> slotA, slotZ;
    if ((*info = zbord_checked(c, nb, n, p, T, Z, orient, schurindex, select, wantZ, alpha, beta, ascale, slotA, slotZ)) != 0 ||
        nb == 0)
        return *info;
    const bord_call call{c, n, p, wantZ, nullptr, select, {alpha, beta, ascale}, k.infos(infos, nb), nswaps, k.s};
    return *info = bord_entry_host<zbord_plain>(call, nb, T, Z, slotA, slotZ);
}

}  // extern "C"
