// Host driver of the periodic Krylov-Schur method: partial_pschur(As, nev, which; ...), src/krylov.jl:446-798.
// Included at the end of psd_engine.cpp (one translation unit), after psd_check_host.inl (psd_devbuf).
//
// The factors, the bases V_l (n x (maxdim + 1), ld n) and a copy of the projected factors live in buffers this driver
// owns (never the context's dH / dZ: the projected pschur_hess / ordschur calls reserve those at their own order).  The
// projected problems are solved through the engine's own entry points on the same context, on host copies of order
// <= maxdim.  Indices below follow the reference: 1-based where a line of krylov.jl is restated.
//
// The factors are dense ([p][n][n], read through psd_kr_mv) or sparse (p CSR triples, read through psd_kr_csr_mv, which
// writes the work vector directly); everything behind the product sees them only through that vector.
#include <algorithm>
#include <complex>
#include <type_traits>

namespace {

// p sparse factors on the device: host arrays of p device pointers, and log2 of the group width of each factor
struct KrylovCsr {
    const int64_t* const* rowptr;
    const int32_t* const* colind;
    const double* const* val;
    const int* lg;
};

// ---- launch geometry and launches, shared by the driver and by the diagnostic entries (psd_?_dense_matvec,
// psd_?_kr_orth, psd_?_kr_basis) so that the two cannot drift apart ---------------------------------------------------
// Geometry at order n and subspace order kmax; dA: the dense factors (nullptr: none, counts as aligned).  The two-row
// body of the Float64 matvec needs an even n (a pair never straddles a column) and a 16-byte aligned base (its loads).
template <bool Z>
psd_krylov_geom kr_geometry(int n, int kmax, const double* dA) {
    psd_krylov_geom g;
    g.rp = (!Z && n % 2 == 0 && ((uintptr_t)dA & 15) == 0) ? 2 : 1;
    g.tiles = (n + PSD_KR_NT * g.rp - 1) / (PSD_KR_NT * g.rp);
    // about 1024 workgroups (4 per compute unit) of at least 32 columns each
    g.nchunk = std::max(1, std::min((1024 + g.tiles - 1) / g.tiles, (n + 31) / 32));
    g.ccols = (n + g.nchunk - 1) / g.nchunk;
    g.nchunk = (n + g.ccols - 1) / g.ccols;
    g.nblk = (n + PSD_KR_NT - 1) / PSD_KR_NT;
    g.ldp = kmax + 2;
    return g;
}
// part[chunk][r] = the partial products of A u (A: one n x n factor on the device)
template <bool Z>
void kr_launch_mv(psd_ctx* c, const psd_krylov_geom& g, const double* A, const double* u, double* part, int n,
                  const int* st) {
    if (g.rp == 2) PSD_LAUNCH((psd_kr_mv<Z, 2>), psd_dim3(g.tiles, g.nchunk), PSD_KR_NT, 0, c->stream, A, u, part, n, g.ccols, st);
    else PSD_LAUNCH((psd_kr_mv<Z, 1>), psd_dim3(g.tiles, g.nchunk), PSD_KR_NT, 0, c->stream, A, u, part, n, g.ccols, st);
}
template <bool Z>
void kr_launch_dots(psd_ctx* c, const psd_kr_args& a, const double* part, int nch, int gate) {
    const size_t e = sizeof(double) * (Z ? 2 : 1);
    PSD_LAUNCH(psd_kr_dots<Z>, psd_dim3(a.nblk), PSD_KR_NT, 2 * PSD_KR_NT * e, c->stream, a, part, nch, gate);
}
// orthogonalise v (summed from the matvec partials when nch > 0) against U[:, 0:ncols), store into U[:, ncols)
template <bool Z>
void kr_launch_stage(psd_ctx* c, const psd_kr_args& a, const double* part, int nch) {
    const size_t e = sizeof(double) * (Z ? 2 : 1);
    kr_launch_dots<Z>(c, a, part, nch, 0);
    if (a.ncols > 0) {
        const size_t lx = (PSD_KR_NT + (size_t)a.ncols) * e;
        PSD_LAUNCH(psd_kr_axpy<Z>, psd_dim3(a.nblk), PSD_KR_NT, lx, c->stream, a, 1);
        kr_launch_dots<Z>(c, a, part, 0, 1);
        PSD_LAUNCH(psd_kr_axpy<Z>, psd_dim3(a.nblk), PSD_KR_NT, lx, c->stream, a, 2);
    }
    PSD_LAUNCH(psd_kr_store<Z>, psd_dim3(a.nblk), PSD_KR_NT, 0, c->stream, a);
}
// rows per workgroup of the basis update: the R x m tile fits the LDS budget
template <bool Z>
int kr_basis_rows(int m) {
    const size_t e = sizeof(double) * (Z ? 2 : 1);
    const int R = (int)std::min<size_t>(64, PSD_KR_BASIS_LDS / ((size_t)m * e));
    return R < 1 ? 1 : R;
}
// V_l[:, a0:a0+m) <- V_l[:, a0:a0+m) Q_l for every l (V: p blocks vstride elements apart, ld n; Q: [p][m][m]); returns R
template <bool Z>
int kr_launch_basis(psd_ctx* c, double* V, size_t vstride, const double* Q, int n, int p, int a0, int m) {
    const size_t e = sizeof(double) * (Z ? 2 : 1);
    const int R = kr_basis_rows<Z>(m);
    PSD_LAUNCH(psd_kr_basis<Z>, psd_dim3((n + R - 1) / R, p), PSD_KR_NT, (size_t)R * m * e, c->stream, V, vstride, Q, n,
               a0, m, R);
    return R;
}
inline psd_kr_args kr_args(const psd_krylov_geom& g, int n, int ncols, int lfac, double tol1, double* U, double* v,
                           double* pA, double* pB, double* w1, double* w2, double* h, double* Hcol, int* st) {
    psd_kr_args a;
    a.n = n;
    a.ncols = ncols;
    a.nblk = g.nblk;
    a.ldp = g.ldp;
    a.lfac = lfac;
    a.eta = 1.0 / sqrt(2.0);
    a.tol1 = tol1;
    a.U = U;
    a.v = v;
    a.pA = pA;
    a.pB = pB;
    a.w1 = w1;
    a.w2 = w2;
    a.h = h;
    a.Hcol = Hcol;
    a.st = st;
    return a;
}

template <bool Z>
struct KrylovRun {
    typedef typename std::conditional<Z, std::complex<double>, double>::type T;
    static constexpr int ES = Z ? 2 : 1;
    psd_ctx* c;
    int n, p, kmin, kmax, nev;
    char which;
    double tol, tol1;
    uint64_t seed, draw = 0;
    psd_krylov_stats* st;
    const double* dA = nullptr;     // dense factors [p][n][n], or
    const KrylovCsr* csr = nullptr;  // sparse factors
    // device
    psd_devbuf bV, bpart, bv, bpA, bpB, bw1, bw2, bh, bH, bQ, bst;
    psd_krylov_geom g;
    size_t vstride = 0, hstride = 0;
    int ldh = 0;
    // host copy of the projected factors: H_l ((kmax + 1) x kmax, ld kmax + 1), l = 1..p; H_p holds the footer row
    std::vector<T> H;
    int kcur = 0;

    double* V(int l) const { return bV.d() + (size_t)l * vstride * ES; }  // l 0-based
    T& h(int l, int i, int j) { return H[(size_t)(l - 1) * hstride + (size_t)(j - 1) * ldh + (i - 1)]; }  // 1-based

    int alloc() {
        vstride = (size_t)n * (kmax + 1);
        ldh = kmax + 1;
        hstride = (size_t)ldh * kmax;
        g = kr_geometry<Z>(n, kmax, dA);
        const int nchunk = g.nchunk, nblk = g.nblk, ldp = g.ldp;
        const size_t e = sizeof(double) * ES;
        PSD_CHECK(bV.alloc((size_t)p * vstride * e));
        if (!csr) PSD_CHECK(bpart.alloc((size_t)nchunk * n * e));  // (a CSR product has no partial sums)
        PSD_CHECK(bv.alloc((size_t)n * e));
        PSD_CHECK(bpA.alloc((size_t)nblk * ldp * e));
        PSD_CHECK(bpB.alloc((size_t)nblk * ldp * e));
        PSD_CHECK(bw1.alloc((size_t)nblk * sizeof(double)));
        PSD_CHECK(bw2.alloc((size_t)nblk * sizeof(double)));
        PSD_CHECK(bh.alloc((size_t)ldp * e));
        PSD_CHECK(bH.alloc((size_t)p * hstride * e));
        PSD_CHECK(bQ.alloc((size_t)p * kmax * kmax * e));
        PSD_CHECK(bst.alloc(sizeof(int) * PSD_KR_ST_WORDS));
        PSD_CHECK(psd_rt_memset(bV.p, 0, (size_t)p * vstride * e, c->stream));
        PSD_CHECK(psd_rt_memset(bst.p, 0, sizeof(int) * PSD_KR_ST_WORDS, c->stream));
        H.assign((size_t)p * hstride, T(0));
        return 0;
    }
    int* dst() const { return (int*)bst.p; }

    psd_kr_args args(double* U, int ncols, double* Hcol, int lfac) {
        return kr_args(g, n, ncols, lfac, tol1, U, bv.d(), bpA.d(), bpB.d(), bw1.d(), bw2.d(), bh.d(), Hcol, dst());
    }
    void stage(const psd_kr_args& a, int nch) { kr_launch_stage<Z>(c, a, bpart.d(), nch); }
    // factor l (0-based) of Krylov step j (1-based), krylov.jl:262-333 / :335-371
    void factor(int l, int j) {
        const double* u = V(l) + (size_t)(j - 1) * n * ES;
        const int lo = (l + 1) % p;
        const int ncols = (l < p - 1) ? j - 1 : j;
        double* Hcol = bH.d() + ((size_t)l * hstride + (size_t)(j - 1) * ldh) * ES;
        if (csr) {
            const int rows = PSD_KR_NT >> csr->lg[l];
            PSD_LAUNCH(psd_kr_csr_mv<Z>, psd_dim3((n + rows - 1) / rows), PSD_KR_NT, PSD_KR_NT * sizeof(double) * ES,
                       c->stream, csr->rowptr[l], csr->colind[l], csr->val[l], u, bv.d(), n, csr->lg[l], dst());
            stage(args(V(lo), ncols, Hcol, l), 0);
            return;
        }
        const double* Al = dA + (size_t)l * n * n * ES;
        kr_launch_mv<Z>(c, g, Al, u, bpart.d(), n, dst());
        stage(args(V(lo), ncols, Hcol, l), g.nchunk);
    }
    int read_state(int* s) {
        PSD_CHECK(psd_rt_d2h(s, bst.p, sizeof(int) * PSD_KR_ST_WORDS, c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        PSD_CHECK(psd_rt_last_error());
        return 0;
    }
    // _reinitialize!(PK, l, j), krylov.jl:152-182: a random column j + 1 of V_l orthogonal to its first j.  ok = false:
    // still in the span (PKSFailure)
    int reinit(int l, int j, bool& ok) {
        PSD_LAUNCH(psd_kr_reset, psd_dim3(1), 64, 0, c->stream, dst());
        PSD_LAUNCH(psd_kr_rand, psd_dim3((n * ES + PSD_KR_NT - 1) / PSD_KR_NT), PSD_KR_NT, 0, c->stream, bv.d(), n * ES,
                   seed, draw++);
        stage(args(V(l), j, nullptr, l), 0);
        int s[PSD_KR_ST_WORDS];
        PSD_CHECK(read_state(s));
        ok = !s[PSD_KR_ST_STOP];
        if (st) st->nreinit += 1;
        PSD_LAUNCH(psd_kr_reset, psd_dim3(1), 64, 0, c->stream, dst());
        return 0;
    }
    int upload_H() {
        PSD_CHECK(psd_rt_h2d(bH.p, H.data(), H.size() * sizeof(T), c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        return 0;
    }
    int download_H() {
        PSD_CHECK(psd_rt_d2h(H.data(), bH.p, H.size() * sizeof(T), c->stream));
        PSD_CHECK(psd_rt_sync(c->stream));
        return 0;
    }
    // V_l[:, a0:a0+m) <- V_l[:, a0:a0+m) Q_l for every l; Q: p host m x m matrices
    int basis(int a0, int m, const std::vector<std::vector<T>>& Q) {
        if (m <= 0) return 0;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<T> q((size_t)p * m * m);
        for (int l = 0; l < p; ++l) std::copy(Q[l].begin(), Q[l].end(), q.begin() + (size_t)l * m * m);
        PSD_CHECK(psd_rt_h2d(bQ.p, q.data(), q.size() * sizeof(T), c->stream));
        kr_launch_basis<Z>(c, bV.d(), vstride, bQ.d(), n, p, a0, m);
        PSD_CHECK(psd_rt_sync(c->stream));
        PSD_CHECK(psd_rt_last_error());
        if (st) st->ms_basis += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    }

    // _deflate!(H1, Hs, Z, ldeflate, jdeflate), krylov.jl:184-226, on the host copy; Zs: p identity j x j on entry
    void deflate(int jdef, int j, std::vector<std::vector<T>>& Zs) {
        const int nc = kmax;
        std::vector<double> gc(nc + 1);
        std::vector<T> gs(nc + 1);
        auto givens = [](T f, T g, double& cs, T& sn, T& r) {
            const double af = std::abs(f), ag = std::abs(g);
            if (ag == 0.0) {
                cs = 1.0;
                sn = T(0);
                r = f;
            } else if (af == 0.0) {
                cs = 0.0;
                if constexpr (Z) sn = std::conj(g) / ag, r = T(ag);
                else sn = 1.0, r = g;
            } else {
                const double nr = std::hypot(af, ag);
                cs = af / nr;
                const T ph = f / af;
                if constexpr (Z) sn = ph * std::conj(g) / nr;
                else sn = ph * g / nr;
                r = ph * nr;
            }
        };
        // rows (i, i+1) of columns [c0, c1] of factor l: G = [c s; -conj(s) c] from the left
        auto lrot = [&](int l, int i, int c0, int c1, double cs, T sn) {
            for (int q = c0; q <= c1; ++q) {
                const T a1 = h(l, i, q), a2 = h(l, i + 1, q);
                h(l, i, q) = cs * a1 + sn * a2;
                if constexpr (Z) h(l, i + 1, q) = -std::conj(sn) * a1 + cs * a2;
                else h(l, i + 1, q) = -sn * a1 + cs * a2;
            }
        };
        // columns (i, i+1) of rows [1, r1] times G^H = [c -s; conj(s) c]
        auto rrot = [&](T* M, int ld, int r1, int i, double cs, T sn) {
            for (int q = 1; q <= r1; ++q) {
                T& a1 = M[(size_t)(i - 1) * ld + (q - 1)];
                T& a2 = M[(size_t)i * ld + (q - 1)];
                const T x1 = a1, x2 = a2;
                if constexpr (Z) a1 = cs * x1 + std::conj(sn) * x2;
                else a1 = cs * x1 + sn * x2;
                a2 = -sn * x1 + cs * x2;
            }
        };
        auto Hp = [&](int l) { return &H[(size_t)(l - 1) * hstride]; };
        for (int i = 1; i <= jdef - 1; ++i) {
            T r;
            givens(h(p, i, i), h(p, i + 1, i), gc[i], gs[i], r);
            h(p, i, i) = r;
            h(p, i + 1, i) = T(0);
            lrot(p, i, i + 1, nc, gc[i], gs[i]);
        }
        for (int i = 1; i <= jdef - 1; ++i) rrot(Zs[0].data(), j, j, i, gc[i], gs[i]);
        for (int l = 1; l <= p - 1; ++l) {
            for (int i = 1; i <= jdef - 1; ++i) {
                rrot(Hp(l), ldh, i + 1, i, gc[i], gs[i]);
                T r;
                givens(h(l, i, i), h(l, i + 1, i), gc[i], gs[i], r);
                h(l, i, i) = r;
                h(l, i + 1, i) = T(0);
                lrot(l, i, i + 1, nc, gc[i], gs[i]);
            }
            for (int i = 1; i <= jdef - 1; ++i) rrot(Zs[l].data(), j, j, i, gc[i], gs[i]);
        }
        for (int i = 1; i <= jdef - 2; ++i) rrot(Hp(p), ldh, i + 1, i, gc[i], gs[i]);
    }

    // periodic_arnoldi!(As, PK, k1:k2, V_1[:, k1]), krylov.jl:228-414.  pa_ok = false: too many singularities.
    int arnoldi(int k1, int k2, bool& pa_ok, int* info) {
        const auto t0 = std::chrono::steady_clock::now();
        pa_ok = true;
        PSD_CHECK(upload_H());
        int singularities = 0;
        int s[PSD_KR_ST_WORDS];
        for (int j = k1; j <= k2;) {
            int ldef = 0, jdef = 0;
            bool again = false;
            int l0 = 0;
            for (;;) {
                PSD_LAUNCH(psd_kr_reset, psd_dim3(1), 64, 0, c->stream, dst());
                for (int l = l0; l < p; ++l) factor(l, j);
                PSD_CHECK(read_state(s));  // the one synchronisation of the step
                if (!s[PSD_KR_ST_STOP]) break;
                const int lf = s[PSD_KR_ST_LFAC];
                bool ok = true;
                if (s[PSD_KR_ST_KIND] == 2) {  // null start vector: start over (krylov.jl:298-304, :323-327)
                    PSD_CHECK(reinit(0, 0, ok));
                    again = true;
                    break;
                }
                if (ldef == 0) {
                    ldef = lf + 1;
                    jdef = j;
                }
                if (lf < p - 1) {  // krylov.jl:307-309: a fresh direction for V_{l+1}, then the rest of the step
                    PSD_CHECK(reinit(lf + 1, j - 1, ok));
                    if (!ok) return *info = PSD_INFO_PKSFAIL;
                    l0 = lf + 1;
                    continue;
                }
                // in span at l = p: trivial deflation (krylov.jl:359-363).  After an earlier deflation in the same
                // step the reference would divide by h_{j+1,j} = 0; the column is re-initialised there as well.
                PSD_CHECK(reinit(0, j, ok));
                if (!ok) return *info = PSD_INFO_PKSFAIL;
                if (ldef == p) ldef = 0;
                break;
            }
            if (again) continue;
            if (ldef > 0) {  // krylov.jl:375-407
                PSD_CHECK(download_H());
                std::vector<std::vector<T>> Zs(p, std::vector<T>((size_t)j * j, T(0)));
                for (int l = 0; l < p; ++l)
                    for (int i = 0; i < j; ++i) Zs[l][(size_t)i * j + i] = T(1);
                deflate(jdef, j, Zs);
                PSD_CHECK(basis(0, j, Zs));
                PSD_CHECK(upload_H());
                if (st) st->ndeflate += 1;
                double hn = 0.0;
                for (int q = 1; q <= jdef; ++q)
                    for (int i = 1; i <= jdef; ++i) hn += std::norm(h(p, i, q));
                hn = sqrt(hn);
                if (!(std::abs(h(p, jdef + 1, jdef)) < 100 * 2.220446049250313e-16 * hn)) {
                    singularities += 1;
                    if (singularities > 5) {
                        pa_ok = false;
                        break;
                    }
                    if (jdef < k2) {
                        bool ok = true;
                        PSD_CHECK(reinit(0, jdef + 1, ok));
                        if (!ok) return *info = PSD_INFO_PKSFAIL;
                    }
                }
            }
            kcur = j;
            j += 1;
        }
        PSD_CHECK(download_H());
        if (st) {
            PSD_CHECK(read_state(s));
            st->nreorth = s[PSD_KR_ST_NREORTH];
            st->ms_arnoldi += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return 0;
    }
};

// the projected problem in the form pschur!(H1, Hx; Q) returns (krylov.jl:575-592): 'R' orientation, schurindex 1,
// factor list Hq[0] = T1, Hq[i] = T[i]; Q[i] = Z[i + 1] (1-based Z)
template <bool Z>
struct ProjSchur {
    typedef typename KrylovRun<Z>::T T;
    int m = 0, p = 0;
    std::vector<std::vector<T>> Hq, Q;
    std::vector<std::complex<double>> lam;
};

template <bool Z>
int proj_pschur(psd_ctx* c, ProjSchur<Z>& ps) {
    const int m = ps.m, p = ps.p;
    std::vector<double*> hp(p), qp(p);
    for (int l = 0; l < p; ++l) {
        hp[l] = (double*)ps.Hq[l].data();
        qp[l] = (double*)ps.Q[l].data();
    }
    int info = 0;
    ps.lam.assign(m, 0.0);
    if constexpr (Z) {
        std::vector<double> alpha(2 * m), beta(m);
        std::vector<int32_t> sc(m);
        psd_z_pschur_hess(c, m, p, hp.data(), nullptr, qp.data(), 1, 1, 30, alpha.data(), beta.data(), sc.data(),
                          nullptr, nullptr, 0, &info);
        if (info) return info;
        for (int i = 0; i < m; ++i)
            ps.lam[i] = std::complex<double>(alpha[2 * i], alpha[2 * i + 1]) / beta[i] * std::ldexp(1.0, sc[i]);
    } else {
        std::vector<double> wr(m), wi(m);
        psd_d_pschur_hess(c, m, p, hp.data(), qp.data(), 1, 1, 30, wr.data(), wi.data(), nullptr, nullptr, 0, &info);
        if (info) return info;
        for (int i = 0; i < m; ++i) ps.lam[i] = std::complex<double>(wr[i], wi[i]);
    }
    return 0;
}

// ordschur!(PS, select) on the projected decomposition (values recomputed); 2000 + j: IllConditionedException(j)
template <bool Z>
int proj_ordschur(psd_ctx* c, ProjSchur<Z>& ps, const std::vector<uint8_t>& sel) {
    const int m = ps.m, p = ps.p;
    std::vector<double*> hp(p), qp(p);
    for (int l = 0; l < p; ++l) {
        hp[l] = (double*)ps.Hq[l].data();
        qp[l] = (double*)ps.Q[l].data();
    }
    int info = 0;
    if constexpr (Z) {
        std::vector<double> alpha(2 * m), beta(m);
        std::vector<int32_t> sc(m);
        psd_z_ordschur(c, m, p, hp.data(), qp.data(), 'R', 1, sel.data(), 1, alpha.data(), beta.data(), sc.data(),
                       nullptr, &info);
        if (info) return info;
        for (int i = 0; i < m; ++i)
            ps.lam[i] = std::complex<double>(alpha[2 * i], alpha[2 * i + 1]) / beta[i] * std::ldexp(1.0, sc[i]);
    } else {
        std::vector<double> wr(m), wi(m);
        psd_d_ordschur(c, m, p, hp.data(), qp.data(), 'R', 1, sel.data(), 1, wr.data(), wi.data(), nullptr, &info);
        if (info) return info;
        for (int i = 0; i < m; ++i) ps.lam[i] = std::complex<double>(wr[i], wi[i]);
    }
    return 0;
}

// "better" in the sense of the target (ArnoldiMethod's get_order): LM largest |λ|, LR / SR largest / smallest real
// part, LI / SI largest / smallest imaginary part
inline bool kr_before(char which, std::complex<double> a, std::complex<double> b) {
    switch (which) {
        case 'M': return std::abs(a) > std::abs(b);
        case 'R': return a.real() > b.real();
        case 'r': return a.real() < b.real();
        case 'I': return a.imag() > b.imag();
        default: return a.imag() < b.imag();
    }
}

// _partial_pschur!, krylov.jl:500-798.  dA device [p][n][n], or csr (then dA is not read); results: T host
// (p x maxdim^2), Z device or host.
template <bool Z>
int partial_pschur_run(psd_ctx* c, int n, int p, const double* dA, int nev, char which, int kmin, int kmax,
                       const double* u1, uint64_t seed, double tol, double tol1, int restarts, int purgebuffer,
                       int* nconv_out, double* const* Tout, double* const* Zhost, double* dZout, double* wr, double* wi,
                       psd_krylov_stats* st, int* info, const KrylovCsr* csr = nullptr) {
    typedef typename KrylovRun<Z>::T T;
    typedef std::complex<double> C;
    constexpr int ES = Z ? 2 : 1;
    const double eps = 2.220446049250313e-16;
    KrylovRun<Z> K;
    K.c = c;
    K.n = n;
    K.p = p;
    K.kmin = kmin;
    K.kmax = kmax;
    K.nev = nev;
    K.which = which;
    K.tol = tol;
    K.tol1 = tol1;
    K.seed = seed;
    K.st = st;
    K.dA = dA;
    K.csr = csr;
    if (int rc = K.alloc()) return *info = rc;
    // start vector, krylov.jl:534-544: u1 or a draw of the generator, normalised into V_1[:, 1]
    if (u1) {
        PSD_CHECK(psd_rt_h2d(K.bv.p, u1, sizeof(double) * ES * (size_t)n, c->stream));
    } else {
        PSD_LAUNCH(psd_kr_rand, psd_dim3((n * ES + PSD_KR_NT - 1) / PSD_KR_NT), PSD_KR_NT, 0, c->stream, K.bv.d(),
                   n * ES, seed, K.draw++);
    }
    {
        psd_kr_args a = K.args(K.V(0), 0, nullptr, 0);
        a.tol1 = 0.0;  // (a start vector is only normalised here)
        K.stage(a, 0);
        int s[PSD_KR_ST_WORDS];
        PSD_CHECK(K.read_state(s));
        if (s[PSD_KR_ST_STOP]) return *info = -9;
    }
    bool pa_ok = true;
    if (int rc = K.arnoldi(1, kmin, pa_ok, info)) return rc;
    int64_t nprods = (int64_t)p * kmin;
    int nlock = 0;

    std::vector<C> lam(kmax + 1, 0.0);
    std::vector<double> rs(kmax + 1, 0.0);
    std::vector<int> ord(kmax + 1, 0);
    double Hnorm = 0.0;
    auto isconv = [&](int i) { return rs[i] < std::max(eps * Hnorm, tol * std::abs(lam[i])); };
    auto sort_ord = [&](int a, int b) {  // sort!(ritz.ord, a, b, OrderPerm(λs, ordering)), stable
        if (b > a) std::stable_sort(ord.begin() + a, ord.begin() + b + 1, [&](int x, int y) { return kr_before(which, lam[x], lam[y]); });
    };
    auto include_pair = [&](int k) {  // include_conjugate_pair(T, ritz, k)
        if (Z || k >= kmax) return k;
        const C l = lam[ord[k]];
        if (l.imag() == 0.0) return k;
        for (int i = 1; i < k; ++i)
            if (lam[ord[i]] == std::conj(l)) return k;
        return k + 1;
    };
    int active = 1, k = kmin;
    auto H = [&](int l, int i, int j) -> T& { return K.h(l, i, j); };
    int iter = 0;
    for (iter = 1; iter <= restarts; ++iter) {
        if (iter > 1) {  // _restore_hessenberg!(PK, active, k, ...), krylov.jl:800-831
            const auto t0 = std::chrono::steady_clock::now();
            const int nw = k - active + 1;
            std::vector<T> H1x((size_t)(nw + 1) * nw);
            std::vector<std::vector<T>> Hx(std::max(p - 1, 1), std::vector<T>((size_t)nw * nw));
            std::vector<std::vector<T>> Qs(p, std::vector<T>((size_t)nw * nw, T(0)));
            for (int q = 0; q < nw; ++q)
                for (int i = 0; i <= nw; ++i) H1x[(size_t)q * (nw + 1) + i] = H(p, active + i, active + q);
            for (int l = 1; l < p; ++l)
                for (int q = 0; q < nw; ++q)
                    for (int i = 0; i < nw; ++i) Hx[l - 1][(size_t)q * nw + i] = H(l, active + i, active + q);
            for (int l = 0; l < p; ++l)
                for (int i = 0; i < nw; ++i) Qs[l][(size_t)i * nw + i] = T(1);
            std::vector<double*> hp(std::max(p - 1, 1)), qp(p);
            for (int l = 0; l + 1 < p; ++l) hp[l] = (double*)Hx[l].data();
            for (int l = 0; l < p; ++l) qp[l] = (double*)Qs[l].data();
            int ri = 0;
            if constexpr (Z) psd_z_rphessenberg(c, nw + 1, nw, p, (double*)H1x.data(), hp.data(), qp.data(), nw, nw, &ri);
            else psd_d_rphessenberg(c, nw + 1, nw, p, (double*)H1x.data(), hp.data(), qp.data(), nw, nw, &ri);
            if (ri) return *info = ri;
            for (int q = 0; q < nw; ++q)
                for (int i = 0; i <= nw; ++i) H(p, active + i, active + q) = H1x[(size_t)q * (nw + 1) + i];
            for (int l = 1; l < p; ++l)
                for (int q = 0; q < nw; ++q)
                    for (int i = 0; i < nw; ++i) H(l, active + i, active + q) = Hx[l - 1][(size_t)q * nw + i];
            for (int l = 1; l <= p; ++l)  // locked rows: H_l[1:active-1, active:k] *= Q_l
                for (int i = 1; i < active; ++i) {
                    std::vector<T> row(nw);
                    for (int q = 0; q < nw; ++q) {
                        T s = T(0);
                        for (int r = 0; r < nw; ++r) s += H(l, i, active + r) * Qs[l - 1][(size_t)q * nw + r];
                        row[q] = s;
                    }
                    for (int q = 0; q < nw; ++q) H(l, i, active + q) = row[q];
                }
            if (st) st->ms_proj += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            PSD_CHECK(K.basis(active - 1, nw, Qs));
        }
        if (k + 1 <= kmax) {
            if (int rc = K.arnoldi(k + 1, kmax, pa_ok, info)) return rc;
            nprods += (int64_t)p * (kmax - k);
        }
        if (st) st->restarts = iter;
        const auto tp = std::chrono::steady_clock::now();
        // the projected problem, krylov.jl:577-592
        const int nk = kmax - active + 1;
        ProjSchur<Z> PS;
        PS.m = nk;
        PS.p = p;
        PS.Hq.assign(p, std::vector<T>((size_t)nk * nk, T(0)));
        PS.Q.assign(p, std::vector<T>((size_t)nk * nk, T(0)));
        for (int q = 0; q < nk; ++q)
            for (int i = 0; i < nk; ++i) {
                if (i <= q + 1) PS.Hq[0][(size_t)q * nk + i] = H(p, active + i, active + q);
                for (int l = 1; l < p; ++l)
                    if (i <= q) PS.Hq[l][(size_t)q * nk + i] = H(p - l, active + i, active + q);
            }
        for (int l = 0; l < p; ++l)
            for (int i = 0; i < nk; ++i) PS.Q[l][(size_t)i * nk + i] = T(1);
        if (int rc = proj_pschur<Z>(c, PS)) return *info = rc;
        {
            double s = 0.0;
            for (const T& x : PS.Hq[0]) s += std::norm(x);
            Hnorm = sqrt(s);  // Kressner eq. 22: the one matrix H1
        }
        for (int i = 0; i < nk; ++i) lam[active + i] = PS.lam[i];
        std::vector<T> foot(nk);
        for (int q = 0; q < nk; ++q) foot[q] = H(p, kmax + 1, active + q);
        for (int i = 1; i <= kmax; ++i) ord[i] = i;
        sort_ord(active, kmax);
        const int eff_nev = include_pair(nev);
        const int j0 = active - 1;
        const int zq = (p == 1) ? 0 : 1;  // Qs[p] = Z[2] of the 'R' result (Z[1] for p = 1)
        // _compute_ritz_resids!, krylov.jl:833-917: each Ritz value (conjugate pair) moved to the top on a copy
        {
            for (int jo = active; jo <= kmax; ++jo) rs[ord[jo]] = INFINITY;
            for (int jo = active; jo <= kmax; ++jo) {
                int j = ord[jo];
                const bool inpair = !Z && lam[j].imag() != 0.0;
                if (inpair) {  // the pair is the 2x2 block of T1 that holds j
                    const int jj = j - j0;
                    const bool start = jj < nk && PS.Hq[0][(size_t)(jj - 1) * nk + jj] != T(0);
                    if (!start) j -= 1;
                    if (rs[j] != INFINITY) continue;
                }
                std::vector<uint8_t> sel(nk, 0);
                sel[j - j0 - 1] = 1;
                if (inpair && j - j0 < nk) sel[j - j0] = 1;
                ProjSchur<Z> PX = PS;
                const int rc = proj_ordschur<Z>(c, PX, sel);
                if (rc >= PSD_INFO_ILLCOND && rc < PSD_INFO_SINGULAR) {  // punt: the footer of the current basis
                    double r = 0.0;
                    for (int q = 0; q < j - j0; ++q) {
                        T s = T(0);
                        for (int i = 0; i < nk; ++i) s += foot[i] * PS.Q[zq][(size_t)q * nk + i];
                        r = std::max(r, std::abs(s));
                    }
                    rs[j] = r;
                    if (inpair) rs[j + 1] = r;
                    continue;
                }
                if (rc) return *info = rc;
                T n0 = T(0), n1 = T(0);
                for (int i = 0; i < nk; ++i) {
                    n0 += foot[i] * PX.Q[zq][i];
                    if (nk > 1) n1 += foot[i] * PX.Q[zq][(size_t)nk + i];
                }
                if (inpair) rs[j] = rs[j + 1] = std::max(std::abs(n0), std::abs(n1));
                else rs[j] = std::abs(n0);
            }
        }
        // how many preferred values may have converged (krylov.jl:622-631)
        if (eff_nev >= active)
            std::stable_sort(ord.begin() + active, ord.begin() + eff_nev + 1,
                             [&](int x, int y) { return (isconv(x) ? 0 : 1) < (isconv(y) ? 0 : 1); });
        {
            int first = 0;
            for (int i = 1; i <= kmax; ++i)
                if (!isconv(ord[i])) {
                    first = i;
                    break;
                }
            nlock = first == 0 ? eff_nev : first - 1;
        }
        // _update_ritz!(ritz, PS, select, active, kmax, kgood, ordering), krylov.jl:921-945
        auto update_ritz = [&](const std::vector<uint8_t>& sel) {
            std::vector<double> old(rs.begin() + active, rs.begin() + kmax + 1);
            for (int i = 0; i < nk; ++i) lam[active + i] = PS.lam[i];
            int nsel = 0;
            for (uint8_t x : sel) nsel += x ? 1 : 0;
            int j1 = active, j2 = active + nsel, q = 0;
            for (int i = 0; i < nk; ++i) {
                if (sel[i]) rs[j1++] = old[q++];
                else rs[j2++] = old[q++];
            }
            for (int i = 1; i <= kmax; ++i) ord[i] = i;
            sort_ord(active, kmax);
        };
        if (nlock >= active) {  // lock: move ord[1:nlock] to the top (krylov.jl:637-667)
            std::vector<uint8_t> sel(nk, 0);
            for (int i = 1; i <= nlock; ++i)
                if (ord[i] >= active && ord[i] <= kmax) sel[ord[i] - j0 - 1] = 1;
            if (int rc = proj_ordschur<Z>(c, PS, sel)) return *info = rc;
            update_ritz(sel);
        }
        if (nlock < nev) {  // converged unwanted values go to the end, to be purged (krylov.jl:675-688)
            const int is = nlock + 1 + purgebuffer;
            if (is < kmax)
                std::stable_sort(ord.begin() + is, ord.begin() + kmax + 1,
                                 [&](int x, int y) { return (isconv(x) ? 1 : 0) < (isconv(y) ? 1 : 0); });
        }
        k = include_pair(std::min(nlock + kmin, (kmin + kmax) / 2));
        {  // the values to retain go to the top (krylov.jl:697-724)
            std::vector<uint8_t> sel(nk, 0);
            for (int i = 1; i <= k; ++i)
                if (ord[i] >= active && ord[i] <= kmax) sel[ord[i] - j0 - 1] = 1;
            ProjSchur<Z> PS0 = PS;
            const int rc = proj_ordschur<Z>(c, PS, sel);
            if (rc >= PSD_INFO_ILLCOND && rc < PSD_INFO_SINGULAR) PS = PS0;  // "reordering failed, start praying"
            else if (rc) return *info = rc;
            else update_ritz(sel);
        }
        // stuff PS back into the Krylov decomposition (krylov.jl:731-761): Qs[1] = Z[1], Qs[l] = Z[p + 2 - l]
        std::vector<std::vector<T>> Qs(p);
        Qs[0] = PS.Q[0];
        for (int l = 2; l <= p; ++l) Qs[l - 1] = PS.Q[p + 1 - l];
        for (int q = 0; q < nk; ++q)
            for (int i = 0; i < nk; ++i) H(p, active + i, active + q) = PS.Hq[0][(size_t)q * nk + i];
        {
            std::vector<T> row(nk);
            for (int q = 0; q < nk; ++q) {
                T s = T(0);
                for (int i = 0; i < nk; ++i) s += foot[i] * Qs[p - 1][(size_t)q * nk + i];
                row[q] = s;
            }
            for (int q = 0; q < nk; ++q) H(p, kmax + 1, active + q) = row[q];
        }
        for (int l = 1; l < p; ++l)
            for (int q = 0; q < nk; ++q)
                for (int i = 0; i < nk; ++i) H(l, active + i, active + q) = PS.Hq[p - l][(size_t)q * nk + i];
        for (int l = 1; l <= p; ++l)
            for (int i = 1; i < active; ++i) {
                std::vector<T> row(nk);
                for (int q = 0; q < nk; ++q) {
                    T s = T(0);
                    for (int r = 0; r < nk; ++r) s += H(l, i, active + r) * Qs[l - 1][(size_t)q * nk + r];
                    row[q] = s;
                }
                for (int q = 0; q < nk; ++q) H(l, i, active + q) = row[q];
            }
        if (st) st->ms_proj += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count();
        PSD_CHECK(K.basis(active - 1, nk, Qs));
        // truncate (krylov.jl:763-771)
        PSD_CHECK(psd_rt_d2d(K.V(0) + (size_t)k * n * ES, K.V(0) + (size_t)kmax * n * ES, sizeof(double) * ES * n,
                             c->stream));
        for (int q = active; q <= k; ++q) H(p, k + 1, q) = H(p, kmax + 1, q);
        for (int q = 1; q <= kmax; ++q) {
            for (int i = k + 2; i <= kmax + 1; ++i) H(p, i, q) = T(0);
            for (int l = 1; l < p; ++l)
                for (int i = k + 2; i <= kmax; ++i) H(l, i, q) = T(0);
        }
        K.kcur = k;
        // _verify_locks!(ritz, H_p[1:k+1, 1:k], nlock, isconverged), krylov.jl:949-987 (a pair's residual is the
        // hypot of its two footer entries, for both members)
        {
            double s = 0.0;
            for (int q = 1; q <= k; ++q)
                for (int i = 1; i <= k + 1; ++i) s += std::norm(H(p, i, q));
            Hnorm = sqrt(s);
            for (int i = 1; i <= nlock; ++i) {
                if (!Z && lam[i].imag() != 0.0 && i < nlock) {
                    rs[i] = rs[i + 1] = std::hypot(std::abs(H(p, k + 1, i)), std::abs(H(p, k + 1, i + 1)));
                    ++i;
                } else {
                    rs[i] = std::abs(H(p, k + 1, i));
                }
            }
            int ncv = 0;
            for (int i = 1; i <= nlock; ++i) {
                if (!isconv(i)) break;
                if (!Z && lam[i].imag() != 0.0) ++i;
                ncv = i;
            }
            nlock = ncv;
        }
        if (!pa_ok) break;
        active = nlock + 1;
        if (active > nev) break;
    }
    const int nconv = active - 1;
    if (st) {
        st->nprods = nprods;
        st->nconverged = nconv;
        st->converged = nconv >= nev;
        st->nev = nev;
        st->suspect = pa_ok ? 0 : 1;
    }
    *nconv_out = nconv;
    for (int i = 0; i < kmax; ++i) {
        wr[i] = i < nconv ? lam[i + 1].real() : 0.0;
        wi[i] = i < nconv ? lam[i + 1].imag() : 0.0;
    }
    // T_l = triu(H_l[1:nconv, 1:nconv]) (l < p), T_p = H_p[1:nconv, 1:nconv]; Z_l = V_l[:, 1:nconv]
    for (int l = 1; l <= p; ++l) {
        T* Tl = (T*)Tout[l - 1];
        for (int q = 1; q <= nconv; ++q)
            for (int i = 1; i <= nconv; ++i)
                Tl[(size_t)(q - 1) * nconv + (i - 1)] = (l < p && i > q) ? T(0) : H(l, i, q);
    }
    const size_t zb = sizeof(double) * ES * (size_t)n * nconv;
    for (int l = 0; l < p; ++l) {
        if (Zhost) PSD_CHECK(psd_rt_d2h(Zhost[l], K.V(l), zb, c->stream));
        else PSD_CHECK(psd_rt_d2d(dZout + (size_t)l * n * kmax * ES, K.V(l), zb, c->stream));
    }
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    return *info = 0;
}

// argument checks of krylov.jl:456-470 and of the ABI, before the device is touched
template <bool Z>
int partial_pschur_args(psd_ctx* c, int n, int p, const void* A, int nev, char which, int mindim, int maxdim,
                        const double* u1, double tol, double tol1, int restarts, int purgebuffer, int* nconv,
                        const void* T, const void* Zo, double* wr, double* wi) {
    if (!c) return -1;
    if (n < 1) return -2;
    if (p < 1) return -3;
    if (!A) return -4;
    if (nev < 1) return -5;
    if (which != 'M' && which != 'R' && which != 'r' && which != 'I' && which != 'i') return -6;
    if (!(nev <= mindim && mindim <= maxdim && (int64_t)maxdim <= (int64_t)p * n)) return -7;
    if (maxdim > PSD_KRYLOV_MAXDIM) return -8;
    if (u1) {
        double s = 0.0;
        for (int i = 0; i < n * (Z ? 2 : 1); ++i) s += u1[i] * u1[i];
        if (!(s > 0.0) || !std::isfinite(s)) return -9;
    }
    if (!(tol > 0.0)) return -11;
    if (!(tol1 >= 0.0)) return -12;
    if (restarts < 0) return -13;
    if (purgebuffer < 0) return -14;
    if (!nconv) return -15;
    if (!T) return -16;
    if (!Zo) return -17;
    if (!wr || !wi) return -18;
    return 0;
}

template <bool Z>
int partial_pschur_host(psd_ctx* c, int n, int p, const double* const* A, int nev, char which, int mindim, int maxdim,
                        const double* u1, uint64_t seed, double tol, double tol1, int restarts, int purgebuffer,
                        int* nconv, double* const* T, double* const* Zo, double* wr, double* wi, psd_krylov_stats* st,
                        int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (st) memset(st, 0, sizeof(*st));
    if ((*info = partial_pschur_args<Z>(c, n, p, A, nev, which, mindim, maxdim, u1, tol, tol1, restarts, purgebuffer,
                                        nconv, T, Zo, wr, wi)) != 0)
        return *info;
    for (int l = 0; l < p; ++l)
        if (!A[l] || !T[l] || !Zo[l]) return *info = !A[l] ? -4 : (!T[l] ? -16 : -17);
    const auto t0 = std::chrono::steady_clock::now();
    constexpr int ES = Z ? 2 : 1;
    const size_t nn = (size_t)n * n * ES;
    psd_devbuf bA;
    PSD_CHECK(bA.alloc(nn * p * sizeof(double)));
    for (int l = 0; l < p; ++l) PSD_CHECK(psd_rt_h2d(bA.d() + l * nn, A[l], nn * sizeof(double), c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    int rc = partial_pschur_run<Z>(c, n, p, bA.d(), nev, which, mindim, maxdim, u1, seed, tol, tol1, restarts,
                                   purgebuffer, nconv, T, Zo, nullptr, wr, wi, st, info);
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return *info = rc;
}

template <bool Z>
int partial_pschur_devapi(psd_ctx* c, int n, int p, const double* dA, int nev, char which, int mindim, int maxdim,
                          const double* u1, uint64_t seed, double tol, double tol1, int restarts, int purgebuffer,
                          int* nconv, double* const* T, double* dZ, double* wr, double* wi, psd_krylov_stats* st,
                          int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (st) memset(st, 0, sizeof(*st));
    if ((*info = partial_pschur_args<Z>(c, n, p, dA, nev, which, mindim, maxdim, u1, tol, tol1, restarts, purgebuffer,
                                        nconv, T, dZ, wr, wi)) != 0)
        return *info;
    for (int l = 0; l < p; ++l)
        if (!T[l]) return *info = -16;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = partial_pschur_run<Z>(c, n, p, dA, nev, which, mindim, maxdim, u1, seed, tol, tol1, restarts, purgebuffer,
                                   nconv, T, nullptr, dZ, wr, wi, st, info);
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return *info = rc;
}

// ---- sparse (CSR) factors --------------------------------------------------------------------------------------------
// The checks of psd_kr_csr_check on a host copy (host entries, before anything is copied): 0, -19 or -20.
inline int csr_check_host(int n, const int64_t* rp, const int32_t* ci) {
    if (rp[0] != 0) return -19;
    for (int i = 0; i < n; ++i)
        if (rp[i + 1] < rp[i]) return -19;
    if (rp[n] > PSD_KR_CSR_MAXNNZ) return -19;
    for (int64_t k = 0; k < rp[n]; ++k)
        if (ci[k] < 0 || ci[k] >= n) return -20;
    return 0;
}

inline int csr_log2(int G) {
    int lg = 0;
    while ((1 << lg) < G) ++lg;
    return lg;
}

// Structure check of p device-resident factors, before any of them is gathered through: the counts come from rowptr[n]
// (bounded here), the rest from psd_kr_csr_check, whose flag words are read once.  code: 0, -19 or -20; lg: log2 of the
// automatic group width of every factor.
inline int csr_validate_dev(psd_ctx* c, int n, int p, const int64_t* const* rowptr, const int32_t* const* colind, int* lg,
                            int* code) {
    *code = 0;
    std::vector<int64_t> nnz(p);
    for (int l = 0; l < p; ++l) PSD_CHECK(psd_rt_d2h(&nnz[l], rowptr[l] + n, sizeof(int64_t), c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    for (int l = 0; l < p; ++l)
        if (nnz[l] < 0 || nnz[l] > PSD_KR_CSR_MAXNNZ) {
            *code = -19;
            return 0;
        }
    psd_devbuf bf;
    PSD_CHECK(bf.alloc(sizeof(int) * PSD_KR_CSR_FLAGS));
    PSD_CHECK(psd_rt_memset(bf.p, 0, sizeof(int) * PSD_KR_CSR_FLAGS, c->stream));
    for (int l = 0; l < p; ++l) {
        const int64_t total = std::max<int64_t>(nnz[l], (int64_t)n + 1);
        const int nb = (int)std::min<int64_t>((total + PSD_KR_NT - 1) / PSD_KR_NT, 4096);
        PSD_LAUNCH(psd_kr_csr_check, psd_dim3(nb), PSD_KR_NT, 0, c->stream, rowptr[l], colind[l], n, nnz[l], (int*)bf.p);
        lg[l] = csr_log2(psd_kr_csr_group(n, nnz[l]));
    }
    int f[PSD_KR_CSR_FLAGS];
    PSD_CHECK(psd_rt_d2h(f, bf.p, sizeof(f), c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    if (f[PSD_KR_CSR_BAD_ROWPTR]) *code = -19;
    else if (f[PSD_KR_CSR_BAD_COLIND]) *code = -20;
    return 0;
}

// the array arguments of a CSR entry: NULL arrays and NULL elements are argument 4
inline bool csr_null(int p, const int64_t* const* rowptr, const int32_t* const* colind, const double* const* val) {
    if (!rowptr || !colind || !val) return true;
    for (int l = 0; l < p; ++l)
        if (!rowptr[l] || !colind[l] || !val[l]) return true;
    return false;
}

// p factors already on the device: structure check, then the driver.  Zhost or dZ as in partial_pschur_run.
template <bool Z>
int partial_pschur_csr_dev(psd_ctx* c, int n, int p, const int64_t* const* rowptr, const int32_t* const* colind,
                           const double* const* val, int nev, char which, int mindim, int maxdim, const double* u1,
                           uint64_t seed, double tol, double tol1, int restarts, int purgebuffer, int* nconv,
                           double* const* T, double* const* Zhost, double* dZ, double* wr, double* wi,
                           psd_krylov_stats* st, int* info) {
    std::vector<int> lg(p);
    int code = 0;
    if (int rc = csr_validate_dev(c, n, p, rowptr, colind, lg.data(), &code)) return *info = rc;
    if (code) return *info = code;
    const KrylovCsr op = {rowptr, colind, val, lg.data()};
    return partial_pschur_run<Z>(c, n, p, nullptr, nev, which, mindim, maxdim, u1, seed, tol, tol1, restarts, purgebuffer,
                                 nconv, T, Zhost, dZ, wr, wi, st, info, &op);
}

template <bool Z>
int partial_pschur_csr_host(psd_ctx* c, int n, int p, const int64_t* const* rowptr, const int32_t* const* colind,
                            const double* const* val, int nev, char which, int mindim, int maxdim, const double* u1,
                            uint64_t seed, double tol, double tol1, int restarts, int purgebuffer, int* nconv,
                            double* const* T, double* const* Zo, double* wr, double* wi, psd_krylov_stats* st,
                            int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (st) memset(st, 0, sizeof(*st));
    const void* A = (rowptr && colind && val) ? (const void*)rowptr : nullptr;
    if ((*info = partial_pschur_args<Z>(c, n, p, A, nev, which, mindim, maxdim, u1, tol, tol1, restarts, purgebuffer,
                                        nconv, T, Zo, wr, wi)) != 0)
        return *info;
    if (csr_null(p, rowptr, colind, val)) return *info = -4;
    for (int l = 0; l < p; ++l)
        if (!T[l] || !Zo[l]) return *info = !T[l] ? -16 : -17;
    for (int l = 0; l < p; ++l)
        if (int rc = csr_check_host(n, rowptr[l], colind[l])) return *info = rc;
    const auto t0 = std::chrono::steady_clock::now();
    constexpr int ES = Z ? 2 : 1;
    std::vector<psd_devbuf> buf(3 * (size_t)p);
    std::vector<const int64_t*> drp(p);
    std::vector<const int32_t*> dci(p);
    std::vector<const double*> dvl(p);
    for (int l = 0; l < p; ++l) {
        const size_t nnz = (size_t)rowptr[l][n];
        psd_devbuf &b0 = buf[3 * l], &b1 = buf[3 * l + 1], &b2 = buf[3 * l + 2];
        PSD_CHECK(b0.alloc(sizeof(int64_t) * ((size_t)n + 1)));
        PSD_CHECK(b1.alloc(sizeof(int32_t) * nnz));
        PSD_CHECK(b2.alloc(sizeof(double) * ES * nnz));
        PSD_CHECK(psd_rt_h2d(b0.p, rowptr[l], sizeof(int64_t) * ((size_t)n + 1), c->stream));
        PSD_CHECK(psd_rt_h2d(b1.p, colind[l], sizeof(int32_t) * nnz, c->stream));
        PSD_CHECK(psd_rt_h2d(b2.p, val[l], sizeof(double) * ES * nnz, c->stream));
        drp[l] = (const int64_t*)b0.p;
        dci[l] = (const int32_t*)b1.p;
        dvl[l] = b2.d();
    }
    PSD_CHECK(psd_rt_sync(c->stream));
    int rc = partial_pschur_csr_dev<Z>(c, n, p, drp.data(), dci.data(), dvl.data(), nev, which, mindim, maxdim, u1, seed,
                                       tol, tol1, restarts, purgebuffer, nconv, T, Zo, nullptr, wr, wi, st, info);
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return *info = rc;
}

template <bool Z>
int partial_pschur_csr_devapi(psd_ctx* c, int n, int p, const int64_t* const* rowptr, const int32_t* const* colind,
                              const double* const* val, int nev, char which, int mindim, int maxdim, const double* u1,
                              uint64_t seed, double tol, double tol1, int restarts, int purgebuffer, int* nconv,
                              double* const* T, double* dZ, double* wr, double* wi, psd_krylov_stats* st, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (st) memset(st, 0, sizeof(*st));
    const void* A = (rowptr && colind && val) ? (const void*)rowptr : nullptr;
    if ((*info = partial_pschur_args<Z>(c, n, p, A, nev, which, mindim, maxdim, u1, tol, tol1, restarts, purgebuffer,
                                        nconv, T, dZ, wr, wi)) != 0)
        return *info;
    if (csr_null(p, rowptr, colind, val)) return *info = -4;
    for (int l = 0; l < p; ++l)
        if (!T[l]) return *info = -16;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = partial_pschur_csr_dev<Z>(c, n, p, rowptr, colind, val, nev, which, mindim, maxdim, u1, seed, tol, tol1,
                                       restarts, purgebuffer, nconv, T, nullptr, dZ, wr, wi, st, info);
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return *info = rc;
}

// y = A x through the driver's kernel, once, on host buffers (group 0: the automatic width)
template <bool Z>
int csr_matvec_host(psd_ctx* c, int n, const int64_t* rowptr, const int32_t* colind, const double* val, const double* x,
                    double* y, int group, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (!c) return *info = -1;
    if (n < 1) return *info = -2;
    if (!rowptr || !colind || !val) return *info = -4;
    if (group < 0 || group > 64 || (group & (group - 1)) != 0) return *info = -8;
    if (!x) return *info = -9;
    if (!y) return *info = -17;
    if (int rc = csr_check_host(n, rowptr, colind)) return *info = rc;
    constexpr int ES = Z ? 2 : 1;
    const size_t nnz = (size_t)rowptr[n], e = sizeof(double) * ES;
    const int lg = csr_log2(group ? group : psd_kr_csr_group(n, (int64_t)nnz));
    psd_devbuf b0, b1, b2, bx, by;
    PSD_CHECK(b0.alloc(sizeof(int64_t) * ((size_t)n + 1)));
    PSD_CHECK(b1.alloc(sizeof(int32_t) * nnz));
    PSD_CHECK(b2.alloc(e * nnz));
    PSD_CHECK(bx.alloc(e * n));
    PSD_CHECK(by.alloc(e * n));
    PSD_CHECK(psd_rt_h2d(b0.p, rowptr, sizeof(int64_t) * ((size_t)n + 1), c->stream));
    PSD_CHECK(psd_rt_h2d(b1.p, colind, sizeof(int32_t) * nnz, c->stream));
    PSD_CHECK(psd_rt_h2d(b2.p, val, e * nnz, c->stream));
    PSD_CHECK(psd_rt_h2d(bx.p, x, e * n, c->stream));
    const int rows = PSD_KR_NT >> lg;
    PSD_LAUNCH(psd_kr_csr_mv<Z>, psd_dim3((n + rows - 1) / rows), PSD_KR_NT, PSD_KR_NT * e, c->stream,
               (const int64_t*)b0.p, (const int32_t*)b1.p, b2.d(), bx.d(), by.d(), n, lg, (const int*)nullptr);
    PSD_CHECK(psd_rt_d2h(y, by.p, e * n, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    return *info = 0;
}

// ---- diagnostic entries of the dense kernels (test plumbing; include/psd_mi355x.h) -----------------------------------
// y = A x: psd_kr_mv, then the chunk sum of psd_kr_dots (ncols = 0), on host buffers; A in place when a_dev
template <bool Z>
int dense_matvec_host(psd_ctx* c, int n, const double* A, int a_dev, const double* x, double* y, psd_krylov_geom* geom,
                      int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (!c) return *info = -1;
    if (n < 1) return *info = -2;
    if (!A) return *info = -4;
    if (a_dev != 0 && a_dev != 1) return *info = -8;
    if (!x) return *info = -9;
    if (!y) return *info = -17;
    const size_t e = sizeof(double) * (Z ? 2 : 1);
    psd_devbuf bA, bx, bv, bpart, bpA;
    const double* dA = A;
    if (!a_dev) {
        PSD_CHECK(bA.alloc(e * n * n));
        PSD_CHECK(psd_rt_h2d(bA.p, A, e * n * n, c->stream));
        dA = bA.d();
    }
    const psd_krylov_geom g = kr_geometry<Z>(n, 0, dA);
    if (geom) *geom = g;
    PSD_CHECK(bx.alloc(e * n));
    PSD_CHECK(bv.alloc(e * n));
    PSD_CHECK(bpart.alloc(e * n * g.nchunk));
    PSD_CHECK(bpA.alloc(e * g.nblk * g.ldp));
    PSD_CHECK(psd_rt_h2d(bx.p, x, e * n, c->stream));
    kr_launch_mv<Z>(c, g, dA, bx.d(), bpart.d(), n, nullptr);
    const psd_kr_args a = kr_args(g, n, 0, 0, 0.0, nullptr, bv.d(), bpA.d(), nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr);
    kr_launch_dots<Z>(c, a, bpart.d(), g.nchunk, 0);
    PSD_CHECK(psd_rt_d2h(y, bv.p, e * n, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    return *info = 0;
}

// one stage of the driver on host buffers
template <bool Z>
int kr_orth_host(psd_ctx* c, int n, int ncols, double* U, const double* v, double* h, double* hjj, double* unew,
                 int32_t* state, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (!c) return *info = -1;
    if (n < 1) return *info = -2;
    if (ncols < 0 || ncols > PSD_KRYLOV_MAXDIM) return *info = -3;
    if (!U && ncols > 0) return *info = -4;
    if (!v) return *info = -5;
    if (!h && ncols > 0) return *info = -6;
    if (!hjj) return *info = -7;
    if (!unew) return *info = -8;
    if (!state) return *info = -9;
    constexpr int ES = Z ? 2 : 1;
    const size_t e = sizeof(double) * ES;
    const psd_krylov_geom g = kr_geometry<Z>(n, ncols, nullptr);
    psd_devbuf bU, bv, bpA, bpB, bw1, bw2, bh, bHc, bst;
    PSD_CHECK(bU.alloc(e * n * ((size_t)ncols + 1)));
    PSD_CHECK(bv.alloc(e * n));
    PSD_CHECK(bpA.alloc(e * g.nblk * g.ldp));
    PSD_CHECK(bpB.alloc(e * g.nblk * g.ldp));
    PSD_CHECK(bw1.alloc(sizeof(double) * g.nblk));
    PSD_CHECK(bw2.alloc(sizeof(double) * g.nblk));
    PSD_CHECK(bh.alloc(e * g.ldp));
    PSD_CHECK(bHc.alloc(e * ((size_t)ncols + 1)));
    PSD_CHECK(bst.alloc(sizeof(int) * PSD_KR_ST_WORDS));
    PSD_CHECK(psd_rt_memset(bst.p, 0, sizeof(int) * PSD_KR_ST_WORDS, c->stream));
    PSD_CHECK(psd_rt_memset(bHc.p, 0, e * ((size_t)ncols + 1), c->stream));
    if (ncols > 0) PSD_CHECK(psd_rt_h2d(bU.p, U, e * n * ncols, c->stream));
    double* dnew = bU.d() + (size_t)ncols * n * ES;
    PSD_CHECK(psd_rt_h2d(dnew, unew, e * n, c->stream));
    PSD_CHECK(psd_rt_h2d(bv.p, v, e * n, c->stream));
    const psd_kr_args a = kr_args(g, n, ncols, 0, 100 * 2.220446049250313e-16, bU.d(), bv.d(), bpA.d(), bpB.d(),
                                  bw1.d(), bw2.d(), bh.d(), bHc.d(), (int*)bst.p);
    kr_launch_stage<Z>(c, a, nullptr, 0);
    std::vector<double> hc(((size_t)ncols + 1) * ES);
    int s[PSD_KR_ST_WORDS];
    if (ncols > 0) PSD_CHECK(psd_rt_d2h(U, bU.p, e * n * ncols, c->stream));
    PSD_CHECK(psd_rt_d2h(unew, dnew, e * n, c->stream));
    PSD_CHECK(psd_rt_d2h(hc.data(), bHc.p, e * ((size_t)ncols + 1), c->stream));
    PSD_CHECK(psd_rt_d2h(s, bst.p, sizeof(s), c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    for (size_t i = 0; i < (size_t)ncols * ES; ++i) h[i] = hc[i];
    *hjj = hc[(size_t)ncols * ES];
    state[0] = s[PSD_KR_ST_STOP];
    state[1] = s[PSD_KR_ST_KIND];
    state[2] = s[PSD_KR_ST_NREORTH];
    state[3] = g.nblk;
    return *info = 0;
}

// the basis update on host buffers
template <bool Z>
int kr_basis_host(psd_ctx* c, int n, int p, int ldv_cols, int a0, int m, double* V, const double* Q, int32_t* R,
                  int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (!c) return *info = -1;
    if (n < 1) return *info = -2;
    if (p < 1) return *info = -3;
    if (ldv_cols < 1) return *info = -4;
    if (a0 < 0) return *info = -5;
    if (m < 1 || m > PSD_KRYLOV_MAXDIM || (int64_t)a0 + m > ldv_cols) return *info = -6;
    if (!V) return *info = -7;
    if (!Q) return *info = -8;
    const size_t e = sizeof(double) * (Z ? 2 : 1);
    const size_t vstride = (size_t)n * ldv_cols;
    psd_devbuf bV, bQ;
    PSD_CHECK(bV.alloc(e * vstride * p));
    PSD_CHECK(bQ.alloc(e * m * m * p));
    PSD_CHECK(psd_rt_h2d(bV.p, V, e * vstride * p, c->stream));
    PSD_CHECK(psd_rt_h2d(bQ.p, Q, e * m * m * p, c->stream));
    const int rows = kr_launch_basis<Z>(c, bV.d(), vstride, bQ.d(), n, p, a0, m);
    if (R) *R = rows;
    PSD_CHECK(psd_rt_d2h(V, bV.p, e * vstride * p, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    return *info = 0;
}

}  // namespace

extern "C" {
int psd_d_partial_pschur(psd_ctx* c, int n, int p, const double* const* A, int nev, char which, int mindim, int maxdim,
                         const double* u1, uint64_t seed, double tol, double tol1, int restarts, int purgebuffer,
                         int* nconv, double* const* T, double* const* Z, double* wr, double* wi, psd_krylov_stats* st,
                         int* info) {
    return partial_pschur_host<false>(c, n, p, A, nev, which, mindim, maxdim, u1, seed, tol, tol1, restarts,
                                      purgebuffer, nconv, T, Z, wr, wi, st, info);
}
int psd_z_partial_pschur(psd_ctx* c, int n, int p, const double* const* A, int nev, char which, int mindim, int maxdim,
                         const double* u1, uint64_t seed, double tol, double tol1, int restarts, int purgebuffer,
                         int* nconv, double* const* T, double* const* Z, double* wr, double* wi, psd_krylov_stats* st,
                         int* info) {
    return partial_pschur_host<true>(c, n, p, A, nev, which, mindim, maxdim, u1, seed, tol, tol1, restarts,
                                     purgebuffer, nconv, T, Z, wr, wi, st, info);
}
int psd_d_partial_pschur_dev(psd_ctx* c, int n, int p, const double* dA, int nev, char which, int mindim, int maxdim,
                             const double* u1, uint64_t seed, double tol, double tol1, int restarts, int purgebuffer,
                             int* nconv, double* const* T, double* dZ, double* wr, double* wi, psd_krylov_stats* st,
                             int* info) {
    return partial_pschur_devapi<false>(c, n, p, dA, nev, which, mindim, maxdim, u1, seed, tol, tol1, restarts,
                                        purgebuffer, nconv, T, dZ, wr, wi, st, info);
}
int psd_z_partial_pschur_dev(psd_ctx* c, int n, int p, const double* dA, int nev, char which, int mindim, int maxdim,
                             const double* u1, uint64_t seed, double tol, double tol1, int restarts, int purgebuffer,
                             int* nconv, double* const* T, double* dZ, double* wr, double* wi, psd_krylov_stats* st,
                             int* info) {
    return partial_pschur_devapi<true>(c, n, p, dA, nev, which, mindim, maxdim, u1, seed, tol, tol1, restarts,
                                       purgebuffer, nconv, T, dZ, wr, wi, st, info);
}
#define PSD_KR_CSR_ARGS                                                                                                  \
    psd_ctx *c, int n, int p, const int64_t *const *rowptr, const int32_t *const *colind, const double *const *val,     \
        int nev, char which, int mindim, int maxdim, const double *u1, uint64_t seed, double tol, double tol1,         \
        int restarts, int purgebuffer, int *nconv, double *const *T
#define PSD_KR_CSR_PASS \
    c, n, p, rowptr, colind, val, nev, which, mindim, maxdim, u1, seed, tol, tol1, restarts, purgebuffer, nconv, T
int psd_d_partial_pschur_csr(PSD_KR_CSR_ARGS, double* const* Z, double* wr, double* wi, psd_krylov_stats* st, int* info) {
    return partial_pschur_csr_host<false>(PSD_KR_CSR_PASS, Z, wr, wi, st, info);
}
int psd_z_partial_pschur_csr(PSD_KR_CSR_ARGS, double* const* Z, double* wr, double* wi, psd_krylov_stats* st, int* info) {
    return partial_pschur_csr_host<true>(PSD_KR_CSR_PASS, Z, wr, wi, st, info);
}
int psd_d_partial_pschur_csr_dev(PSD_KR_CSR_ARGS, double* dZ, double* wr, double* wi, psd_krylov_stats* st, int* info) {
    return partial_pschur_csr_devapi<false>(PSD_KR_CSR_PASS, dZ, wr, wi, st, info);
}
int psd_z_partial_pschur_csr_dev(PSD_KR_CSR_ARGS, double* dZ, double* wr, double* wi, psd_krylov_stats* st, int* info) {
    return partial_pschur_csr_devapi<true>(PSD_KR_CSR_PASS, dZ, wr, wi, st, info);
}
#undef PSD_KR_CSR_ARGS
#undef PSD_KR_CSR_PASS
int psd_d_csr_matvec(psd_ctx* c, int n, const int64_t* rowptr, const int32_t* colind, const double* val, const double* x,
                     double* y, int group, int* info) {
    return csr_matvec_host<false>(c, n, rowptr, colind, val, x, y, group, info);
}
int psd_z_csr_matvec(psd_ctx* c, int n, const int64_t* rowptr, const int32_t* colind, const double* val, const double* x,
                     double* y, int group, int* info) {
    return csr_matvec_host<true>(c, n, rowptr, colind, val, x, y, group, info);
}
int psd_d_dense_matvec(psd_ctx* c, int n, const double* A, int a_dev, const double* x, double* y, psd_krylov_geom* geom,
                       int* info) {
    return dense_matvec_host<false>(c, n, A, a_dev, x, y, geom, info);
}
int psd_z_dense_matvec(psd_ctx* c, int n, const double* A, int a_dev, const double* x, double* y, psd_krylov_geom* geom,
                       int* info) {
    return dense_matvec_host<true>(c, n, A, a_dev, x, y, geom, info);
}
int psd_d_kr_orth(psd_ctx* c, int n, int ncols, double* U, const double* v, double* h, double* hjj, double* unew,
                  int32_t* state, int* info) {
    return kr_orth_host<false>(c, n, ncols, U, v, h, hjj, unew, state, info);
}
int psd_z_kr_orth(psd_ctx* c, int n, int ncols, double* U, const double* v, double* h, double* hjj, double* unew,
                  int32_t* state, int* info) {
    return kr_orth_host<true>(c, n, ncols, U, v, h, hjj, unew, state, info);
}
int psd_d_kr_basis(psd_ctx* c, int n, int p, int ldv_cols, int a0, int m, double* V, const double* Q, int32_t* R,
                   int* info) {
    return kr_basis_host<false>(c, n, p, ldv_cols, a0, m, V, Q, R, info);
}
int psd_z_kr_basis(psd_ctx* c, int n, int p, int ldv_cols, int a0, int m, double* V, const double* Q, int32_t* R,
                   int* info) {
    return kr_basis_host<true>(c, n, p, ldv_cols, a0, m, V, Q, R, info);
}
}  // extern "C"
