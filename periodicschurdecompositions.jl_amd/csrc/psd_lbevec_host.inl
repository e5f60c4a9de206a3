// Host driver of psd_eigcond_batch / psd_eigcond_batch_dev (psd_bev_cond, psd_lbevec.h): the reciprocal condition numbers
// of the eigenvalues of nb periodic Schur decompositions with respect to every factor, from the right and left vectors
// the eigenvector entries write (shifted layout, complex for both families).  Included at the end of psd_engine.cpp behind
// psd_batch_host.inl (psd_batchbuf, batch_staged).  One launch per group, one read-back.

namespace {

int eigcond_checked(psd_ctx* c, int nb, int n, int p, const void* V, const void* W, char orient, int maxvec,
                    const int* nvec, const double* s) {
    if (!c) return -1;
    if (n < 1) return -2;
    if (p < 1) return -3;
    if (nb < 0) return -11;
    if (nb == 0) return 0;
    if (!V) return -4;
    if (!W) return -5;
    if (orient != 'L' && orient != 'R') return -7;
    if (!nvec) return -12;
    if (maxvec < 1) return -10;
    for (int q = 0; q < nb; ++q)
        if (nvec[q] < 0 || nvec[q] > maxvec) return -10;
    if (!s) return -13;
    if (c->shard_world > 1) return PSD_INFO_NOTIMPL;  // (as the eigenvector entries)
    return 0;
}

// gc problems on the device: dV, dW [gc][p][maxvec][n] complex; s: host [gc][maxvec][p]
int eigcond_group(psd_ctx* c, int gc, int n, int p, const double* dV, const double* dW, bool left, int maxvec,
                  const int* nvec, double* s) {
    const size_t ns = (size_t)gc * maxvec * p;
    psd_batchbuf bN, bS;
    PSD_CHECK(bN.alloc(sizeof(int) * gc));
    PSD_CHECK(bS.alloc(sizeof(double) * ns));
    PSD_CHECK(psd_rt_h2d(bN.ptr, nvec, sizeof(int) * gc, c->stream));
    psd_bev_cond_args g;
    g.V = dV; g.W = dW; g.nvec = (const int*)bN.ptr; g.s = bS.d();
    g.n = n; g.p = p; g.maxvec = maxvec; g.left = left;
    PSD_LAUNCH(psd_bev_cond, psd_dim3(gc * maxvec), 64, PSD_BEV_COND_LDS, c->stream, g);
    PSD_CHECK(psd_rt_d2h(s, bS.d(), sizeof(double) * ns, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    return 0;
}

}  // namespace

extern "C" {

int psd_eigcond_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dV, const double* dW, char orient, int maxvec,
                          const int* nvec, double* s, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if ((*info = eigcond_checked(c, nb, n, p, dV, dW, orient, maxvec, nvec, s)) != 0 || nb == 0) return *info;
    const size_t vb = 2 * (size_t)n * maxvec * p;  // doubles of a problem's vectors of one side
    // (the grid is one workgroup per column: groups keep it below 2^31 - 1)
    const int g = (int)std::min<size_t>((size_t)nb, (size_t)INT_MAX / maxvec);
    for (int q0 = 0; q0 < nb; q0 += g) {
        const int gc = nb - q0 < g ? nb - q0 : g;
        if ((*info = eigcond_group(c, gc, n, p, dV + (size_t)q0 * vb, dW + (size_t)q0 * vb, orient == 'L', maxvec, nvec + q0,
                                   s + (size_t)q0 * maxvec * p)) != 0)
            return *info;
    }
    return *info = 0;
}

int psd_eigcond_batch(psd_ctx* c, int nb, int n, int p, double* const* V, double* const* W, char orient, int maxvec,
                      const int* nvec, double* s, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if ((*info = eigcond_checked(c, nb, n, p, V, W, orient, maxvec, nvec, s)) != 0 || nb == 0) return *info;
    const size_t vb = 2 * (size_t)n * maxvec;
    const batch_list L[] = {{V, p, vb, BATCH_IN}, {W, p, vb, BATCH_IN}};
    auto body = [&](int q0, int gc, double* const* d) {
        return eigcond_group(c, gc, n, p, d[0], d[1], orient == 'L', maxvec, nvec + q0, s + (size_t)q0 * maxvec * p);
    };
    const size_t per = sizeof(double) * (2 * vb * p + (size_t)maxvec * p);
    return *info = batch_staged(c, nb, per, L, nullptr, batch_no_extra, body);
}

}  // extern "C"
