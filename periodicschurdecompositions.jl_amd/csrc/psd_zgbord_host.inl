// Host drivers of psd_z_gordschur_batch / psd_z_gordschur_batch_dev (psd_zgbord.h): ordschur!(P, select) for nb ComplexF64
// generalized periodic Schur forms of one shape and one signature, as psd_z_gpschur_batch leaves them.  Included at the
// end of psd_engine.cpp behind psd_zbord_host.inl: the group path is its zbord_family with the description below —
// psd_zgbord and psd_zgbord_values per group, zgordschur_dev problem by problem above PSD_BORD_NMAX or where no window fits
// the LDS —, the checks are its zbord_checked and the entry bodies those of psd_bord_host.inl.  A null or all-true
// signature is the call of psd_z_ordschur_batch[_dev].
//
// Measured for this path: the sweep of tools/ordschur_batch_timing.py --signed (nb = 256, alternating S, n = 8 ... 64,
// p = 4 and 16) against the loop of single psd_z_gordschur calls — the batched call is ahead at every swept shape, 38 to
// 101 x in wall time (profiles/batch/README.md).  Orders 65 ... 128 have not been swept; the cap is the shared
// PSD_BORD_NMAX.

namespace {

struct zgbord_signed {
    using args_t = psd_zgbord_args;
    static constexpr int trcap = PSD_GTR_CAP, wmin = PSD_ZGBORD_WMIN, giveup = PSD_ZGBORD_WINCAP;
    static constexpr bool has_sig = true;
    static size_t window_lds(int p, int w) { return zgord_lds_bytes(p, w); }
    static size_t apply_lds(int) { return psd_zgbqz_apply_lds_bytes(); }
    static int reserve(psd_ctx* c, int n, int p) {
        const int rc = c->zreserve(n, p, false, 16);
        return rc != 0 ? rc : c->zgreserve(n, p);
    }
    static int single(psd_ctx* c, int n, int p, psd_z* H, psd_z* Z, const uint8_t* S, const uint8_t* select, int wantZ,
                      double* alpha, double* beta, int32_t* ascale, psd_stats* ps, int* pinfo) {
        return zgordschur_dev(c, n, p, H, Z, S, select, wantZ, alpha, beta, ascale, ps, pinfo);
    }
    static const void* kernel() { return reinterpret_cast<const void*>(psd_zgbord); }
    static void launch(psd_ctx* c, int gc, int n, size_t lds, const args_t& a) {
        PSD_LAUNCH(psd_zgbord, psd_dim3(gc), PSD_STEP_NT, lds, c->stream, a);
        PSD_LAUNCH(psd_zgbord_values, psd_dim3((n + 63) / 64, gc), 64, 0, c->stream, a);
    }
};

// the argument codes of psd_z_ordschur_batch (zbord_checked) and the working order of the signed call; -10: the entry
// of S that lands first in that order is false (generalized.jl:182)
int zgbord_checked(psd_ctx* c, int nb, int n, int p, const void* T, const void* Z, const uint8_t* S, char orient,
                   int schurindex, const uint8_t* select, int wantZ, const double* alpha, const double* beta,
                   const int32_t* ascale, signed_order& o) {
    std::vector<int> slotA, slotZ;
    if (int e = zbord_checked(c, nb, n, p, T, Z, orient, schurindex, select, wantZ, alpha, beta, ascale, slotA, slotZ)) return e;
    if (nb == 0) return 0;
    return signed_slots(orient, schurindex, p, S, o) != 0 ? -10 : 0;
}

}  // namespace

extern "C" {

int psd_z_gordschur_batch_dev(psd_ctx* c, int nb, int n, int p, void* dT, void* dZ, const uint8_t* S, char orient,
                              int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta,
                              int32_t* ascale, int* infos, int* nswaps, psd_stats* stats, int* info) {
    if (zgb_all_true(S, p))  // (the all-true kernel, as psd_z_gpschur_batch_dev keeps it)
        return psd_z_ordschur_batch_dev(c, nb, n, p, dT, dZ, orient, schurindex, select, wantZ, alpha, beta, ascale, infos,
                                        nswaps, stats, info);
    batch_call<psd_stats> k(info, stats);
    signed_order o;
    if ((*info = zgbord_checked(c, nb, n, p, dT, dZ, S, orient, schurindex, select, wantZ, alpha, beta, ascale, o)) != 0 ||
        nb == 0)
        return *info;
    const bord_call call{c, n, p, wantZ, o.S.data(), select, {alpha, beta, ascale}, k.infos(infos, nb), nswaps, k.s};
    return *info = bord_entry_dev<zbord_family<zgbord_signed>>(call, nb, dT, dZ, o.sA, o.sZ);
}

int psd_z_gordschur_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, const uint8_t* S, char orient,
                          int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta, int32_t* ascale,
                          int* infos, int* nswaps, psd_stats* stats, int* info) {
    if (zgb_all_true(S, p))
        return psd_z_ordschur_batch(c, nb, n, p, T, Z, orient, schurindex, select, wantZ, alpha, beta, ascale, infos, nswaps,
                                    stats, info);
    batch_call<psd_stats> k(info, stats);
    signed_order o;
    if ((*info = zgbord_checked(c, nb, n, p, T, Z, S, orient, schurindex, select, wantZ, alpha, beta, ascale, o)) != 0 ||
        nb == 0)
        return *info;
    const bord_call call{c, n, p, wantZ, o.S.data(), select, {alpha, beta, ascale}, k.infos(infos, nb), nswaps, k.s};
    return *info = bord_entry_host<zbord_family<zgbord_signed>>(call, nb, T, Z, o.sA, o.sZ);
}

}  // extern "C"
