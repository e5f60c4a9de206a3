// Host driver of psd_d_eigvecs_batch / psd_d_eigvecs_batch_dev (psd_bevec.h): eigenvectors by back-substitution for nb
// periodic Schur decompositions of one shape, as psd_d_pschur_batch leaves them.  Included at the end of psd_engine.cpp
// behind psd_evec_host.inl (eigvecs_dev, psd_ev_root) and psd_batch_host.inl (psd_batchbuf, batch_group, batch_staged).
//
// Per group of problems: the tables (row-block map, solve columns, roots, eigenvalues, the list of units) are built on
// the host and uploaded once; then psd_bev_solve, psd_bev_backtransform for V_1, psd_bev_norm, psd_bev_backtransform for
// the other factors — four launches whatever nb and n are — and one read-back of the counters.  Orders above
// PSD_BEV_NMAX run eigvecs_dev problem by problem on the slices of the batch buffers.
//
// The complex and signed drivers (psd_zbevec_host.inl, psd_zgbevec_host.inl, psd_gbevec_host.inl) come in behind this
// file and share the argument checks, the call description, bevec_itab, bevec_launch, the single-path loop, the
// statistics and the bodies of the two kinds of entry (bevec_entry_dev, bevec_entry_host).
//
// psd_d_leigvecs_batch / psd_d_leigvecs_batch_dev (the LEFT eigenvectors, psd_lbevec.h) are the same two bodies with
// lside set: lbevec_run puts the flip-adjoint form of a group into workspace (one launch), the group run above works on
// it with the tables of the flipped form (lbevec_rows, bevec_root), and one launch turns the columns round.

namespace {

// the 2x2 row blocks of every problem from the sub-diagonals sub [nb][n] of the quasi-triangular factors; completes select
// to whole conjugate pairs and counts the columns
void bevec_blocks(int nb, int n, const double* sub, uint8_t* select, std::vector<int>& bsz, int* nvec) {
    bsz.assign((size_t)nb * n, 1);
    for (int q = 0; q < nb; ++q) {
        int* b = bsz.data() + (size_t)q * n;
        uint8_t* s = select + (size_t)q * n;
        for (int i = 0; i + 1 < n; ++i)
            if (b[i] == 1 && sub && sub[(size_t)q * n + i] != 0.0) {
                b[i] = 2;
                b[i + 1] = 0;
            }
        int nv = 0;
        for (int i = 0; i < n; i += b[i]) {
            if (b[i] == 2 && (s[i] || s[i + 1])) s[i] = s[i + 1] = 1;
            if (s[i]) nv += b[i];
        }
        nvec[q] = nv;
    }
}

struct bevec_call {
    psd_ctx* c;
    int n, p, six, schurindex, shifted, maxvec;
    bool left;
    char orient;
    // a left-vector call (psd_lbevec.h): n, p, left, orient and six describe the FLIPPED form the solve runs on, the
    // eigenvalues, selections and row blocks handed down are the caller's and are flipped where the tables are built
    bool lconj = false;
};

// The flipped form of gc problems of a left-vector call: rows reversed, eigenvalues conjugated.  The roots follow in
// bevec_root.
struct lbevec_rows {
    std::vector<double> wr, wi;
    std::vector<uint8_t> select;
    std::vector<int> bsz;
    lbevec_rows(int gc, int n, const double* wr_, const double* wi_, const uint8_t* select_, const int* bsz_)
        : wr((size_t)gc * n), wi((size_t)gc * n), select((size_t)gc * n), bsz(bsz_ ? (size_t)gc * n : 0) {
        for (int q = 0; q < gc; ++q)
            for (int i = 0; i < n; ++i) {
                const size_t o = (size_t)q * n + i, f = (size_t)q * n + n - 1 - i;
                wr[f] = wr_[o];
                wi[f] = -wi_[o];
                select[f] = select_[o];
                if (bsz_ && bsz_[o] != 0) {  // (the block at rows i, i + b - 1 stands at rows n - i - b, ... of the flipped form)
                    bsz[f - (bsz_[o] - 1)] = bsz_[o];
                    if (bsz_[o] == 2) bsz[f] = 0;
                }
            }
    }
};

// the root the solve divides by.  l: the eigenvalue of the form the solve runs on.  Of a flipped form it is
// conj(psd_ev_root(caller's lambda)), NOT psd_ev_root(l): the two differ for a negative real lambda (psd_ev_root drops the
// sign of a zero imaginary part), and the left vectors have to belong to the root the right vectors belong to
std::complex<double> bevec_root(const bevec_call& k, std::complex<double> l) {
    return k.lconj ? std::conj(psd_ev_root(std::conj(l), k.p)) : psd_ev_root(l, k.p);
}

// The device part of a group, for both families (CPLX: the kernels of psd_zbevec.h): the tables of gc problems (itab, dtab,
// the units behind them) go up, then the solve, the back-transformation of V_1, its norms and phases, the other factors,
// and one read-back of the counters into cnt3 [gc][3].  sgn: the senses of the working factors of a signed batch.  Complex:
// psd_zgbev_solve (psd_zgbevec.h) is the solve then, there are no doubles to upload (dtab is empty), and the third
// counter is the columns with a zero scalar, from flags of their own behind the counters (no NaN columns).  Real:
// psd_gbev_solve (psd_gbevec.h), dtab the scalars of the solve columns; the third counter stays zero here (the caller
// counts the zero scalars on the host)
template <bool CPLX>
int bevec_launch(const bevec_call& k, int gc, const double* dT, const double* dZ, std::vector<int>& itab,
                 const std::vector<double>& dtab, const std::vector<int>& units, int nsm, double* dV, int32_t* cnt3,
                 psd_bevec_stats* st, const int* sgn = nullptr) {
    psd_ctx* c = k.c;
    const int n = k.n, p = k.p, nmat = k.shifted ? p : 1;
    const int nunits = (int)(units.size() / 2);
    PSD_CHECK(psd_rt_memset(dV, 0, sizeof(double) * 2 * (size_t)gc * nmat * n * k.maxvec, c->stream));
    if (nunits == 0) {
        PSD_CHECK(psd_rt_sync(c->stream));
        return 0;
    }
    itab.insert(itab.end(), units.begin(), units.end());
    const size_t isgn = itab.size();
    if (sgn) itab.insert(itab.end(), sgn, sgn + p);
    const size_t ncnt = 3 * (size_t)gc * n, nflag = sgn && CPLX ? (size_t)gc * n : 0;
    psd_batchbuf bI, bD, bX, bR, bS, bC;
    PSD_CHECK(bI.alloc(sizeof(int) * itab.size()));
    if (!dtab.empty()) PSD_CHECK(bD.alloc(sizeof(double) * dtab.size()));
    PSD_CHECK(bX.alloc(sizeof(double) * 2 * (size_t)gc * p * n * nsm));
    if (p > 64) PSD_CHECK(bR.alloc(sizeof(double) * 4 * (size_t)nunits * p));
    PSD_CHECK(bS.alloc(sizeof(double) * 2 * (size_t)gc * n));
    PSD_CHECK(bC.alloc(sizeof(int) * (ncnt + nflag)));
    PSD_CHECK(psd_rt_h2d(bI.ptr, itab.data(), sizeof(int) * itab.size(), c->stream));
    if (!dtab.empty()) PSD_CHECK(psd_rt_h2d(bD.ptr, dtab.data(), sizeof(double) * dtab.size(), c->stream));
    PSD_CHECK(psd_rt_memset(bC.ptr, 0, sizeof(int) * (ncnt + nflag), c->stream));
    Timer tsolve, tback;
    tsolve.start(c->stream);
    psd_bev_args a;
    a.T = dT; a.itab = (const int*)bI.ptr; a.dtab = bD.d(); a.X = bX.d(); a.R = bR.d(); a.cnt = (int*)bC.ptr;
    a.n = n; a.p = p; a.nsm = nsm; a.nunits = nunits; a.gc = gc; a.six = k.six;
    const int C = 64 / psd_bev_lw(p);
    if (sgn && !CPLX) {
        psd_gbev_args ga;
        ga.b = a; ga.sgn = (const int*)bI.ptr + isgn;
        PSD_LAUNCH(psd_gbev_solve, psd_dim3((nunits + C - 1) / C), 64, PSD_GBEV_LDS, c->stream, ga);
    } else if (sgn) {
        psd_zgbev_args ga;
        ga.b = a; ga.sgn = (const int*)bI.ptr + isgn; ga.zc = (int*)bC.ptr + ncnt;
        PSD_LAUNCH(psd_zgbev_solve, psd_dim3((nunits + C - 1) / C), 64, PSD_ZGBEV_LDS, c->stream, ga);
    } else if (CPLX) PSD_LAUNCH(psd_zbev_solve, psd_dim3((nunits + C - 1) / C), 64, PSD_BEV_LDS, c->stream, a);
    else PSD_LAUNCH(psd_bev_solve, psd_dim3((nunits + C - 1) / C), 64, PSD_BEV_LDS, c->stream, a);
    st->nlaunch += 1;
    st->ms_solve += tsolve.stop(c->stream);
    // V_l = Z_l x_l: V_1 first, its norms and phases, then the other factors with the column factors
    tback.start(c->stream);
    psd_bev_bt_args g;
    g.Z = dZ; g.X = bX.d(); g.itab = (const int*)bI.ptr; g.S = nullptr; g.cnt = (const int*)bC.ptr; g.V = dV;
    g.n = n; g.p = p; g.nsm = nsm; g.nmat = nmat; g.maxvec = k.maxvec; g.z0 = 0; g.nz = 1;
    const int tiles = (int)(((size_t)nsm * n + PSD_BEV_NT - 1) / PSD_BEV_NT);
    if (CPLX) PSD_LAUNCH(psd_zbev_backtransform, psd_dim3(gc, tiles), PSD_BEV_NT, 0, c->stream, g);
    else PSD_LAUNCH(psd_bev_backtransform, psd_dim3(gc, tiles), PSD_BEV_NT, 0, c->stream, g);
    PSD_LAUNCH(psd_bev_norm, psd_dim3((int)(((size_t)gc * n + PSD_BEV_NT - 1) / PSD_BEV_NT)), PSD_BEV_NT, 0, c->stream, dV,
               (const int*)bI.ptr, (const int*)bC.ptr, bS.d(), n, p, gc, nmat, k.maxvec);
    st->nlaunch += 2;
    if (nmat > 1) {
        g.S = bS.d(); g.z0 = 1; g.nz = nmat - 1;
        if (CPLX) PSD_LAUNCH(psd_zbev_backtransform, psd_dim3(gc * (nmat - 1), tiles), PSD_BEV_NT, 0, c->stream, g);
        else PSD_LAUNCH(psd_bev_backtransform, psd_dim3(gc * (nmat - 1), tiles), PSD_BEV_NT, 0, c->stream, g);
        st->nlaunch += 1;
    }
    st->ms_backtransform += tback.stop(c->stream);
    std::vector<int> cnt(ncnt + nflag);
    PSD_CHECK(psd_rt_d2h(cnt.data(), bC.ptr, sizeof(int) * (ncnt + nflag), c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    for (int q = 0; q < gc; ++q)
        for (int j = 0; j < n; ++j) {
            const int* e = cnt.data() + 3 * ((size_t)q * n + j);
            cnt3[3 * q] += e[0];
            cnt3[3 * q + 1] += e[1] > 0;
            cnt3[3 * q + 2] += nflag ? cnt[ncnt + (size_t)q * n + j] : e[2];
        }
    return 0;
}

// The integer tables of gc real problems from their completed selections and row blocks (itab, and the units): one solve
// column per selected block.  col(q, ns, i): solve column ns of problem q stands on the block at row i (the doubles of the
// family).  Returns the largest number of solve columns of a problem.
template <class Col>
int bevec_itab(const bevec_call& k, int gc, const uint8_t* select, const int* bsz, std::vector<int>& itab,
               std::vector<int>& units, Col col) {
    const int n = k.n, p = k.p;
    const int IS = psd_bev_istride(n), IH = psd_bev_ihead(p);
    itab.assign((size_t)IH + (size_t)gc * IS, 0);
    units.clear();
    for (int j = 0; j < p; ++j) {  // working form (left orientation), as eigvecs_dev
        itab[j] = k.left ? j : p - 1 - j;
        itab[p + j] = k.left ? j : (p - j) % p;
    }
    int nsm = 0;
    for (int q = 0; q < gc; ++q) {
        int* tab = itab.data() + IH + (size_t)q * IS;
        const int* b = bsz + (size_t)q * n;
        const uint8_t* s = select + (size_t)q * n;
        int ns = 0, nvec = 0, nblk = 0;
        for (int i = 0; i < n; i += b[i]) {
            ++nblk;
            if (!s[i]) continue;
            tab[n + ns] = i;
            tab[2 * n + ns] = b[i];
            tab[3 * n + ns] = i + b[i];
            tab[4 * n + ns] = nvec;
            tab[5 * n + ns] = b[i] == 2;
            tab[6 * n + ns] = nblk;
            col(q, ns, i);
            units.push_back(q);
            units.push_back(ns);
            nvec += b[i];
            ++ns;
        }
        for (int i = 0; i < n; ++i) tab[i] = b[i];
        tab[7 * n] = ns;
        nsm = ns > nsm ? ns : nsm;
    }
    return nsm;
}

// gc problems resident on the device (dT, dZ [gc][p][n][n], dV [gc][nmat][maxvec][n] complex), their eigenvalues, completed
// selections and row blocks; cnt3 [gc][3] receives the counters per problem
int bevec_group(const bevec_call& k, int gc, const double* dT, const double* dZ, const double* wr, const double* wi,
                const uint8_t* select, const int* bsz, double* dV, int32_t* cnt3, psd_bevec_stats* st) {
    const int n = k.n, DS = psd_bev_dstride(n);
    std::vector<int> itab, units;
    std::vector<double> dtab((size_t)gc * DS, 0.0);
    const int nsm = bevec_itab(k, gc, select, bsz, itab, units, [&](int q, int ns, int i) {
        double* dt = dtab.data() + (size_t)q * DS;
        const std::complex<double> l(wr[(size_t)q * n + i], wi[(size_t)q * n + i]), u = bevec_root(k, l);
        dt[2 * ns] = u.real();
        dt[2 * ns + 1] = u.imag();
        dt[2 * n + 2 * ns] = l.real();
        dt[2 * n + 2 * ns + 1] = l.imag();
    });
    for (int q = 0; q < gc; ++q)
        for (int i = 0; i < n; ++i) {
            dtab[(size_t)q * DS + 4 * n + 2 * i] = wr[(size_t)q * n + i];
            dtab[(size_t)q * DS + 4 * n + 2 * i + 1] = wi[(size_t)q * n + i];
        }
    return bevec_launch<false>(k, gc, dT, dZ, itab, dtab, units, nsm, dV, cnt3, st);
}

// above PSD_BEV_NMAX, for every family: a single path on the slices of the batch buffers (its V blocks are n x nvec:
// through a staging block into the n x maxvec blocks of the batch).  select: completed; single(q, sel, dVq, es) runs the
// single driver on problem q with its row of select, for nvec[q] columns
template <class Single>
int bevec_single_loop(const bevec_call& k, int gc, const uint8_t* select, const int* nvec, double* dV, int32_t* cnt3,
                      psd_bevec_stats* st, Single single) {
    psd_ctx* c = k.c;
    const int n = k.n, p = k.p, nmat = k.shifted ? p : 1;
    const size_t vb = 2 * (size_t)n * k.maxvec;
    PSD_CHECK(psd_rt_memset(dV, 0, sizeof(double) * vb * nmat * gc, c->stream));
    psd_batchbuf stage;
    PSD_CHECK(stage.alloc(sizeof(double) * vb * nmat));
    for (int q = 0; q < gc; ++q) {
        if (nvec[q] == 0) continue;
        std::vector<uint8_t> sel(select + (size_t)q * n, select + (size_t)(q + 1) * n);
        psd_evec_stats es;
        memset(&es, 0, sizeof(es));
        const int rc = single(q, sel.data(), stage.d(), &es);
        if (rc != 0) return rc;
        for (int l = 0; l < nmat; ++l)
            PSD_CHECK(psd_rt_d2d(dV + ((size_t)q * nmat + l) * vb, stage.d() + 2 * (size_t)l * n * nvec[q],
                                 sizeof(double) * 2 * n * nvec[q], c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        cnt3[3 * q] += es.nperturbed;
        cnt3[3 * q + 1] += es.nrescaled;
        cnt3[3 * q + 2] += es.nzero;
        st->ms_solve += es.ms_solve;
        st->ms_backtransform += es.ms_backtransform;
        st->nlaunch += 3 + 2 * ((n + PSD_EV_CH - 1) / PSD_EV_CH);  // (an upper bound: a launch pair per chunk)
    }
    return 0;
}

// eigvecs_dev as that single path.  lam [gc][n]: the eigenvalues
template <bool CPLX>
int bevec_single(const bevec_call& k, int gc, const double* dT, const double* dZ, const std::complex<double>* lam,
                 const uint8_t* select, const int* nvec, double* dV, int32_t* cnt3, psd_bevec_stats* st) {
    const int n = k.n, p = k.p;
    const size_t bd = (CPLX ? 2 : 1) * (size_t)n * n;
    return bevec_single_loop(k, gc, select, nvec, dV, cnt3, st, [&](int q, uint8_t* sel, double* dVq, psd_evec_stats* es) {
        return eigvecs_dev<CPLX>(k.c, n, p, dT + (size_t)q * p * bd, dZ + (size_t)q * p * bd, lam + (size_t)q * n, k.orient,
                                 k.schurindex, sel, k.shifted, dVq, nvec[q], es, nullptr, k.lconj);
    });
}

// the group loop of a device entry: groups of at most batch_group(c, nb, per) problems, body(q0, gc) for each (a
// non-zero code ends the call)
template <class Body>
int bevec_dev_groups(psd_ctx* c, int nb, size_t per, Body body) {
    const int g = batch_group(c, nb, per);
    for (int q0 = 0; q0 < nb; q0 += g)
        if (const int rc = body(q0, nb - q0 < g ? nb - q0 : g)) return rc;
    return 0;
}

int bevec_run(const bevec_call& k, int gc, const double* dT, const double* dZ, const double* wr, const double* wi,
              const uint8_t* select, const int* bsz, const int* nvec, double* dV, int32_t* cnt3, psd_bevec_stats* st) {
    st->ngroups += 1;
    std::optional<lbevec_rows> f;
    if (k.lconj) {
        f.emplace(gc, k.n, wr, wi, select, bsz);
        wr = f->wr.data(); wi = f->wi.data(); select = f->select.data(); bsz = f->bsz.data();
    }
    if (k.n <= k.c->bev_nmax) return bevec_group(k, gc, dT, dZ, wr, wi, select, bsz, dV, cnt3, st);
    std::vector<std::complex<double>> lam((size_t)gc * k.n);
    for (size_t e = 0; e < lam.size(); ++e) lam[e] = std::complex<double>(wr[e], wi[e]);
    return bevec_single<false>(k, gc, dT, dZ, lam.data(), select, nvec, dV, cnt3, st);
}

// A group of a left-vector call (CPLX: a complex form).  The flip-adjoint of dT and the reversed dZ go into workspace
// (psd_lbev_flip: one launch), run(fT, fZ) is the family's group run on them into dV, and psd_lbev_reverse turns the
// columns of dV into the caller's order (one launch): two launches more than the right call, whatever gc and n are.
template <bool CPLX, class Run>
int lbevec_run(const bevec_call& k, int gc, const double* dT, const double* dZ, double* dV, const int* nvec,
               psd_bevec_stats* st, Run run) {
    psd_ctx* c = k.c;
    const int n = k.n, p = k.p, nmat = k.shifted ? p : 1;
    const size_t tot = (CPLX ? 2 : 1) * (size_t)gc * p * n * n;
    psd_batchbuf bF, bN;
    PSD_CHECK(bF.alloc(sizeof(double) * 2 * tot));
    PSD_CHECK(bN.alloc(sizeof(int) * gc));
    PSD_CHECK(psd_rt_h2d(bN.ptr, nvec, sizeof(int) * gc, c->stream));
    const int nt = (n + PSD_LBEV_TILE - 1) / PSD_LBEV_TILE;
    const int tiles = nt * nt < PSD_LBEV_TILES_MAX ? nt * nt : PSD_LBEV_TILES_MAX;
    Timer tflip, trev;
    tflip.start(c->stream);
    if (CPLX) PSD_LAUNCH(psd_zlbev_flip, psd_dim3(2 * gc * p, tiles), PSD_BEV_NT, PSD_LBEV_LDS(true), c->stream, dT, dZ, bF.d(), n, gc * p);
    else PSD_LAUNCH(psd_lbev_flip, psd_dim3(2 * gc * p, tiles), PSD_BEV_NT, PSD_LBEV_LDS(false), c->stream, dT, dZ, bF.d(), n, gc * p);
    st->nlaunch += 1;
    st->ms_solve += tflip.stop(c->stream);
    if (const int rc = run((const double*)bF.d(), (const double*)bF.d() + tot)) return rc;
    int mv = 0;
    for (int q = 0; q < gc; ++q) mv = nvec[q] > mv ? nvec[q] : mv;
    const size_t pairs = (size_t)(mv / 2) * n;
    const int rt = (int)((pairs + PSD_BEV_NT - 1) / PSD_BEV_NT);
    trev.start(c->stream);
    PSD_LAUNCH(psd_lbev_reverse, psd_dim3(gc * nmat, rt < 1 ? 1 : (rt < PSD_LBEV_TILES_MAX ? rt : PSD_LBEV_TILES_MAX)), PSD_BEV_NT, 0,
               c->stream, dV, (const int*)bN.ptr, n, nmat, k.maxvec);
    st->nlaunch += 1;
    st->ms_backtransform += trev.stop(c->stream);
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    return 0;
}

int bevec_checked(psd_ctx* c, int nb, int n, int p, const void* T, const void* Z, const double* wr, const double* wi,
                  char orient, int schurindex, const uint8_t* select, int* nvec, psd_bevec_stats* st) {
    if (!c) return -1;
    if (n < 1) return -2;
    if (p < 1) return -3;
    if (nb < 0) return -11;
    if (nb == 0) return 0;
    if (!T) return -4;
    if (!Z) return -5;
    if (!wr || !wi) return -6;
    if (orient != 'L' && orient != 'R') return -7;
    if (schurindex < 1 || schurindex > p) return -8;
    if (!select) return -9;
    if (!nvec) return -12;
    if (c->shard_world > 1) return PSD_INFO_NOTIMPL;  // (a period-sharded context keeps a slice of Z: single problems only)
    (void)st;
    return 0;
}

void bevec_finish(int nb, const int* nvec, const int32_t* cnt3, int32_t* pcnt, psd_bevec_stats* st) {
    st->nb = nb;
    for (int q = 0; q < nb; ++q) {
        st->nvec_total += nvec[q];
        st->nperturbed += cnt3[3 * q];
        st->nrescaled += cnt3[3 * q + 1];
        st->nzero += cnt3[3 * q + 2];
    }
    st->ms_kernels = st->ms_solve + st->ms_backtransform;
    if (pcnt) memcpy(pcnt, cnt3, sizeof(int32_t) * 3 * (size_t)nb);
}

// The device entry of every family behind its checks and counts (mv: the most columns of a problem, at most k.maxvec): nb
// problems in dT / dZ [nb][p] blocks of bd doubles, dV [nb][nmat][maxvec][n] complex.  run(q0, gc, dT, dZ, dV, cnt3) is
// the family's group run on the device blocks and counters of the problems from q0 on.
template <class Run>
int bevec_entry_dev(const bevec_call& k, int nb, size_t bd, const double* dT, const double* dZ, double* dV, int mv,
                    const int* nvec, int32_t* pcnt, psd_bevec_stats* st, Run run) {
    const size_t flipped = k.lconj ? sizeof(double) * 2 * bd * k.p : 0;  // (the flipped copies of T and Z of a left call)
    psd_ctx* c = k.c;
    const int n = k.n, p = k.p, nmat = k.shifted ? p : 1;
    std::vector<int32_t> cnt3(3 * (size_t)nb, 0);
    if (mv > 0) {
        const int rc = bevec_dev_groups(c, nb, sizeof(double) * 2 * (size_t)p * n * mv + flipped, [&](int q0, int gc) {
            return run(q0, gc, dT + (size_t)q0 * p * bd, dZ + (size_t)q0 * p * bd, dV + 2 * (size_t)q0 * nmat * n * k.maxvec,
                       cnt3.data() + 3 * (size_t)q0);
        });
        if (rc != 0) return rc;
    } else {  // nothing selected
        PSD_CHECK(psd_rt_memset(dV, 0, sizeof(double) * 2 * (size_t)nb * nmat * n * k.maxvec, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
    }
    bevec_finish(nb, nvec, cnt3.data(), pcnt, st);
    return 0;
}

// The host entry likewise: T, Z (nb * p matrices of bd doubles) and V (nb * nmat of n x maxvec complex) through the
// staged group loop (16 bytes per element of V and of the X planes)
template <class Run>
int bevec_entry_host(const bevec_call& k, int nb, size_t bd, double* const* T, double* const* Z, double* const* V, int mv,
                     const int* nvec, int32_t* pcnt, psd_bevec_stats* st, Run run) {
    const int n = k.n, p = k.p, nmat = k.shifted ? p : 1;
    const size_t vb = 2 * (size_t)n * k.maxvec;
    std::vector<int32_t> cnt3(3 * (size_t)nb, 0);
    if (mv == 0 || k.maxvec == 0) {  // nothing selected
        for (size_t e = 0; e < (size_t)nb * nmat; ++e) memset(V[e], 0, sizeof(double) * vb);
    } else {
        const batch_list L[] = {{T, p, bd, BATCH_IN}, {Z, p, bd, BATCH_IN}, {V, nmat, vb, BATCH_OUT}};
        auto body = [&](int q0, int gc, double* const* d) { return run(q0, gc, d[0], d[1], d[2], cnt3.data() + 3 * (size_t)q0); };
        // (a left call holds the flipped copies of T and Z beside them)
        const size_t per = sizeof(double) * ((k.lconj ? 4 : 2) * bd * p + vb * nmat + 2 * (size_t)p * n * mv);
        if (const int rc = batch_staged(k.c, nb, per, L, nullptr, batch_no_extra, body)) return rc;
    }
    bevec_finish(nb, nvec, cnt3.data(), pcnt, st);
    return 0;
}

// The two real entries behind their names.  lside: the left vectors (psd_lbevec.h): the solve runs on the flipped form,
// which has the opposite orientation and the same schurindex
int bevec_d_dev(bool lside, psd_ctx* c, int nb, int n, int p, const double* dT, const double* dZ, const double* wr,
                const double* wi, char orient, int schurindex, uint8_t* select, int shifted, double* dV, int maxvec,
                int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info) {
    batch_call<psd_bevec_stats> entry(info, stats);
    psd_bevec_stats* st = entry.s;
    if ((*info = bevec_checked(c, nb, n, p, dT, dZ, wr, wi, orient, schurindex, select, nvec, st)) != 0 || nb == 0)
        return *info;
    const size_t nn = (size_t)n * n, tot = (size_t)nb * n;
    const bool left = (orient == 'L') != lside;
    bool any = false;
    for (size_t e = 0; e < tot && !any; ++e) any = select[e] != 0;
    std::vector<double> sub;
    if (any && n > 1) {  // one kernel and one read-back define the 2x2 row blocks of the whole batch
        psd_batchbuf bsub;
        PSD_CHECK(bsub.alloc(sizeof(double) * tot));
        PSD_LAUNCH(psd_bev_subdiag, psd_dim3((int)((tot + PSD_BEV_NT - 1) / PSD_BEV_NT)), PSD_BEV_NT, 0, c->stream, dT, n, p,
                   schurindex - 1, nb, bsub.d());
        st->nlaunch += 1;
        sub.resize(tot);
        PSD_CHECK(psd_rt_d2h(sub.data(), bsub.d(), sizeof(double) * tot, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
    }
    std::vector<int> bsz;
    bevec_blocks(nb, n, sub.empty() ? nullptr : sub.data(), select, bsz, nvec);
    int mv = 0;
    for (int q = 0; q < nb; ++q) mv = nvec[q] > mv ? nvec[q] : mv;
    if (!dV) return *info = 0;
    if (mv > maxvec) return *info = -10;
    // (a selected row is a column or two: mv > 0 exactly when anything is selected)
    const bevec_call k{c, n, p, left ? schurindex - 1 : p - schurindex, schurindex, shifted, maxvec, left, left ? 'L' : 'R', lside};
    return *info = bevec_entry_dev(k, nb, nn, dT, dZ, dV, mv, nvec, pcnt, st,
                                   [&](int q0, int gc, const double* dTg, const double* dZg, double* dVg, int32_t* cnt3) {
        auto run = [&](const double* gT, const double* gZ) {
            return bevec_run(k, gc, gT, gZ, wr + (size_t)q0 * n, wi + (size_t)q0 * n, select + (size_t)q0 * n,
                             bsz.data() + (size_t)q0 * n, nvec + q0, dVg, cnt3, st);
        };
        return lside ? lbevec_run<false>(k, gc, dTg, dZg, dVg, nvec + q0, st, run) : run(dTg, dZg);
    });
}

int bevec_d_host(bool lside, psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, const double* wr,
                 const double* wi, char orient, int schurindex, uint8_t* select, int shifted, double* const* V, int maxvec,
                 int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info) {
    batch_call<psd_bevec_stats> entry(info, stats);
    psd_bevec_stats* st = entry.s;
    if ((*info = bevec_checked(c, nb, n, p, T, Z, wr, wi, orient, schurindex, select, nvec, st)) != 0 || nb == 0)
        return *info;
    const size_t nn = (size_t)n * n, tot = (size_t)nb * n;
    const bool left = (orient == 'L') != lside;
    std::vector<double> sub(tot, 0.0);  // (the factors are on the host: no kernel)
    for (int q = 0; q < nb; ++q) {
        const double* t = T[(size_t)q * p + schurindex - 1];
        for (int i = 0; i + 1 < n; ++i) sub[(size_t)q * n + i] = t[(size_t)i * n + i + 1];
    }
    std::vector<int> bsz;
    bevec_blocks(nb, n, sub.data(), select, bsz, nvec);
    int mv = 0;
    for (int q = 0; q < nb; ++q) mv = nvec[q] > mv ? nvec[q] : mv;
    if (!V) return *info = 0;
    if (mv > maxvec) return *info = -10;
    const bevec_call k{c, n, p, left ? schurindex - 1 : p - schurindex, schurindex, shifted, maxvec, left, left ? 'L' : 'R', lside};
    return *info = bevec_entry_host(k, nb, nn, T, Z, V, mv, nvec, pcnt, st,
                                    [&](int q0, int gc, const double* dTg, const double* dZg, double* dVg, int32_t* cnt3) {
        auto run = [&](const double* gT, const double* gZ) {
            return bevec_run(k, gc, gT, gZ, wr + (size_t)q0 * n, wi + (size_t)q0 * n, select + (size_t)q0 * n,
                             bsz.data() + (size_t)q0 * n, nvec + q0, dVg, cnt3, st);
        };
        return lside ? lbevec_run<false>(k, gc, dTg, dZg, dVg, nvec + q0, st, run) : run(dTg, dZg);
    });
}

}  // namespace

extern "C" {

int psd_d_eigvecs_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, const double* dZ, const double* wr,
                            const double* wi, char orient, int schurindex, uint8_t* select, int shifted, double* dV,
                            int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info) {
    return bevec_d_dev(false, c, nb, n, p, dT, dZ, wr, wi, orient, schurindex, select, shifted, dV, maxvec, nvec, pcnt, stats,
                       info);
}

int psd_d_eigvecs_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, const double* wr,
                        const double* wi, char orient, int schurindex, uint8_t* select, int shifted, double* const* V,
                        int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info) {
    return bevec_d_host(false, c, nb, n, p, T, Z, wr, wi, orient, schurindex, select, shifted, V, maxvec, nvec, pcnt, stats,
                        info);
}

int psd_d_leigvecs_batch_dev(psd_ctx* c, int nb, int n, int p, const double* dT, const double* dZ, const double* wr,
                             const double* wi, char orient, int schurindex, uint8_t* select, int shifted, double* dV,
                             int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info) {
    return bevec_d_dev(true, c, nb, n, p, dT, dZ, wr, wi, orient, schurindex, select, shifted, dV, maxvec, nvec, pcnt, stats,
                       info);
}

int psd_d_leigvecs_batch(psd_ctx* c, int nb, int n, int p, double* const* T, double* const* Z, const double* wr,
                         const double* wi, char orient, int schurindex, uint8_t* select, int shifted, double* const* V,
                         int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info) {
    return bevec_d_host(true, c, nb, n, p, T, Z, wr, wi, orient, schurindex, select, shifted, V, maxvec, nvec, pcnt, stats,
                        info);
}

}  // extern "C"
