// Host side of the device verifier (psd_check.h): checkpsd(P, As; thresh, strict), src/diagnostics.jl:190-263.
// Included at the end of psd_engine.cpp (one translation unit).

namespace {

// device allocation freed on every way out of the function that owns it
struct psd_devbuf {
    void* p = nullptr;
    ~psd_devbuf() {
        if (p) psd_rt_free(p);
    }
    int alloc(size_t bytes) { return psd_rt_malloc(&p, bytes); }
    double* d() const { return (double*)p; }
};

// The verdict on one factor from its norms (diagnostics.jl:236-262), for the single and the batched path alike: o =
// ||Z Z' - I||_F, r = ||Z_a T Z_b' - A||_F, t = ||tril(T, .)||_F, anorm = opnorm(A, 1).  *e receives the normalized error.
inline bool checkpsd_verdict(int n, double o, double r, double t, double anorm, double thresh, int strict, double* e) {
    const double eps = PSD_DBL_EPS;
    bool good = true;
    const double cmp = strict ? 0.0 : 10.0 * eps * n;
    if (t > cmp) good = false;
    if (o > 10.0 * eps * n) good = false;
    *e = r / eps / anorm;
    if (!(*e <= thresh)) good = false;
    return good;
}

// T, Z, A: [p][n][n] device blocks in USER order (ES doubles per element).  err[p] (host) receives the normalized
// factorization errors, orth[p] / tri[p] (host, optional) the orthogonality and triangularity norms.
template <bool CPLX>
int checkpsd_dev(psd_ctx* c, int n, int p, const double* dT, const double* dZ, const double* dA, const uint8_t* S,
                 char orient, int schurindex, const double* dwi, double thresh, int strict, double* err, double* orth,
                 double* tri, int* ok) {
    constexpr int E = CPLX ? 2 : 1;
    const size_t nn = (size_t)n * n * E;
    psd_devbuf bW, bacc;
    PSD_CHECK(bW.alloc(nn * sizeof(double)));
    PSD_CHECK(bacc.alloc(sizeof(double) * 5 * (size_t)p));
    double *dW = bW.d(), *dacc = bacc.d();
    PSD_CHECK(psd_rt_memset(dacc, 0, sizeof(double) * 5 * (size_t)p, c->stream));
    const bool left = orient == 'L';
    const int tiles = (n + PSD_CK_TM - 1) / PSD_CK_TM;
    (void)tiles;
    for (int l = 0; l < p; ++l) {
        const int l1 = (l + 1) % p;
        const double* Tl = dT + (size_t)l * nn;
        const double* Al = dA + (size_t)l * nn;
        const int sub = (!CPLX && l == schurindex - 1) ? 1 : 0;  // diagnostics.jl:223-233
        if (CPLX)
            PSD_LAUNCH(psd_ck_small_z, psd_dim3(1), 256, 256 * 8, c->stream, Tl, Al, n, sub, dwi, dacc + 5 * l + 2);
        else
            PSD_LAUNCH(psd_ck_small_d, psd_dim3(1), 256, 256 * 8, c->stream, Tl, Al, n, sub, dwi, dacc + 5 * l + 2);
        const bool sl = S ? (S[l] != 0) : true;
        const int a = (sl != left) ? l : l1, b = (sl != left) ? l1 : l;  // diagnostics.jl:247-251
        psd_ck_args g[3];
        g[0].A = dZ + (size_t)l * nn; g[0].B = dZ + (size_t)l * nn; g[0].C = nullptr; g[0].D = nullptr;
        g[0].acc = dacc + 5 * l + 0; g[0].n = n; g[0].mode = 2; g[0].bconjt = 1;
        g[1].A = Tl; g[1].B = dZ + (size_t)b * nn; g[1].C = dW; g[1].D = nullptr;
        g[1].acc = nullptr; g[1].n = n; g[1].mode = 0; g[1].bconjt = 1;
        g[2].A = dZ + (size_t)a * nn; g[2].B = dW; g[2].C = nullptr; g[2].D = Al;
        g[2].acc = dacc + 5 * l + 1; g[2].n = n; g[2].mode = 1; g[2].bconjt = 0;
        for (int q = 0; q < 3; ++q) {
#ifdef PSD_HOSTSIM
            psd_ck_gemm_sim<CPLX>(g[q]);
#else
            hipLaunchKernelGGL(psd_ck_gemm<CPLX>, dim3(tiles, tiles), dim3(256), 0, c->stream, g[q]);
#endif
        }
    }
    std::vector<double> acc(5 * (size_t)p);
    PSD_CHECK(psd_rt_d2h(acc.data(), dacc, sizeof(double) * 5 * (size_t)p, c->stream));
    PSD_CHECK(psd_rt_sync(c->stream));
    PSD_CHECK(psd_rt_last_error());
    bool good = true;
    for (int l = 0; l < p; ++l) {
        const double o = sqrt(acc[5 * l + 0]), r = sqrt(acc[5 * l + 1]), t = sqrt(acc[5 * l + 2]);
        if (!checkpsd_verdict(n, o, r, t, acc[5 * l + 3], thresh, strict, &err[l])) good = false;
        if (orth) orth[l] = o;
        if (tri) tri[l] = t;
    }
    if (ok) *ok = good ? 1 : 0;
    return 0;
}

template <bool CPLX>
int checkpsd_host(psd_ctx* c, int n, int p, double* const* T, double* const* Z, double* const* A, const uint8_t* S,
                  char orient, int schurindex, const double* wi, double thresh, int strict, double* err, double* orth,
                  double* tri, int* ok, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (!c) return *info = -1;
    if ((*info = check_dims(n, p)) != 0) return *info;
    if (!T || !Z || !A) return *info = -4;
    if (orient != 'R' && orient != 'L') return *info = -8;
    if (schurindex < 1 || schurindex > p) return *info = -9;
    if (!err) return *info = -13;
    constexpr int E = CPLX ? 2 : 1;
    const size_t nn = (size_t)n * n * E;
    psd_devbuf bT, bZ, bA, bwi;
    PSD_CHECK(bT.alloc(nn * p * sizeof(double)));
    PSD_CHECK(bZ.alloc(nn * p * sizeof(double)));
    PSD_CHECK(bA.alloc(nn * p * sizeof(double)));
    double *dT = bT.d(), *dZ = bZ.d(), *dA = bA.d(), *dwi = nullptr;
    for (int l = 0; l < p; ++l) {
        PSD_CHECK(psd_rt_h2d(dT + l * nn, T[l], nn * 8, c->stream));
        PSD_CHECK(psd_rt_h2d(dZ + l * nn, Z[l], nn * 8, c->stream));
        PSD_CHECK(psd_rt_h2d(dA + l * nn, A[l], nn * 8, c->stream));
    }
    if (wi && !CPLX) {
        PSD_CHECK(bwi.alloc(sizeof(double) * (size_t)n));
        dwi = bwi.d();
        PSD_CHECK(psd_rt_h2d(dwi, wi, sizeof(double) * (size_t)n, c->stream));
    }
    const int rc = checkpsd_dev<CPLX>(c, n, p, dT, dZ, dA, S, orient, schurindex, dwi, thresh, strict, err, orth, tri, ok);
    return *info = rc;
}

}  // namespace

extern "C" {

int psd_d_checkpsd(psd_ctx* c, int n, int p, double* const* T, double* const* Z, double* const* A, const uint8_t* S,
                   char orient, int schurindex, const double* wi, double thresh, int strict, double* err, double* orth,
                   double* tri, int* ok, int* info) {
    return checkpsd_host<false>(c, n, p, T, Z, A, S, orient, schurindex, wi, thresh, strict, err, orth, tri, ok, info);
}

int psd_z_checkpsd(psd_ctx* c, int n, int p, double* const* T, double* const* Z, double* const* A, const uint8_t* S,
                   char orient, int schurindex, double thresh, int strict, double* err, double* orth, double* tri, int* ok,
                   int* info) {
    return checkpsd_host<true>(c, n, p, T, Z, A, S, orient, schurindex, nullptr, thresh, strict, err, orth, tri, ok, info);
}

}  // extern "C"

namespace {

// the device entry of either element type: operands already in HBM
template <bool CPLX>
int checkpsd_dev_entry(psd_ctx* c, int n, int p, const double* dT, const double* dZ, const double* dA, const uint8_t* S,
                       char orient, int schurindex, double thresh, int strict, double* err, double* orth, double* tri,
                       int* ok, int* info) {
    int dummy;
    if (!info) info = &dummy;
    if (!c) return *info = -1;
    if ((*info = check_dims(n, p)) != 0) return *info;
    if (!dT || !dZ || !dA) return *info = -4;
    if (orient != 'R' && orient != 'L') return *info = -8;
    if (schurindex < 1 || schurindex > p) return *info = -9;
    if (!err) return *info = -12;
    return *info = checkpsd_dev<CPLX>(c, n, p, dT, dZ, dA, S, orient, schurindex, nullptr, thresh, strict, err, orth, tri, ok);
}

}  // namespace

extern "C" {

int psd_d_checkpsd_dev(psd_ctx* c, int n, int p, const double* dT, const double* dZ, const double* dA, const uint8_t* S,
                       char orient, int schurindex, double thresh, int strict, double* err, double* orth, double* tri,
                       int* ok, int* info) {
    return checkpsd_dev_entry<false>(c, n, p, dT, dZ, dA, S, orient, schurindex, thresh, strict, err, orth, tri, ok, info);
}

int psd_z_checkpsd_dev(psd_ctx* c, int n, int p, const double* dT, const double* dZ, const double* dA, const uint8_t* S,
                       char orient, int schurindex, double thresh, int strict, double* err, double* orth, double* tri,
                       int* ok, int* info) {
    return checkpsd_dev_entry<true>(c, n, p, dT, dZ, dA, S, orient, schurindex, thresh, strict, err, orth, tri, ok, info);
}

}  // extern "C"
