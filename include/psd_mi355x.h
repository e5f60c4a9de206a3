/* libpsd_mi355x — C ABI of the MI355X-native periodic Schur engine.
 *
 * The reference (RalphAS/PeriodicSchurDecompositions.jl v0.1.6) has no FFI layer: its operator API
 * is a set of Julia methods.  Each entry point below is what a thin Julia `ccall` wrapper binds
 * to replace one of those methods (file:line under /root/reference/src); INTEGRATION.md shows the
 * wrapper.  Plain pointers and sizes only; no exceptions cross the boundary.
 *
 * Conventions
 *   - matrices are column-major, ld = n, Float64;
 *   - host entry points take an array of p pointers (Julia's Vector{Matrix{Float64}}); the caller
 *     owns every buffer, results are written back into the same buffers (the reference's
 *     in-place contract, PeriodicSchurDecompositions.jl:120-152);
 *   - `_dev` entry points take one device allocation [p][n][n] (factor-major) already resident
 *     in HBM and leave the result there;
 *   - return value == *info: 0 ok; <0 argument -k invalid; >0 algorithmic:
 *       PSD_INFO_NOCONV + level  convergence failed at level i  (PSD.jl:892 ErrorException)
 *       PSD_INFO_NOTIMPL         not implemented                 (PSD.jl:30 NotImplemented)
 *       PSD_INFO_RUNTIME         HIP runtime failure / no device
 */
#ifndef PSD_MI355X_H
#define PSD_MI355X_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSD_INFO_NOCONV 1000000
#define PSD_INFO_NOTIMPL 2000000
#define PSD_INFO_RUNTIME 3000000

typedef struct psd_ctx psd_ctx;

/* per-call statistics: what bench.py needs to turn time into sweeps/s and algorithmic GB/s */
typedef struct psd_stats {
    int64_t niter;        /* sum of `its` over deflation levels (PSD.jl:1060 `niter`)            */
    int32_t maxits;       /* PSD.jl:1059                                                         */
    int32_t nsweeps;      /* double-shift QR sweeps performed (PSD.jl:806-887)                   */
    int32_t nrqpass;      /* RQ clean-up passes (PSD.jl:602-635)                                 */
    int32_t ndefl1;       /* 1x1 deflations                                                      */
    int32_t ndefl2;       /* 2x2 deflations                                                      */
    int32_t nwindows;     /* diagonal windows chased (= step-kernel launches that did work)      */
    int32_t nlaunch_step; /* step-kernel launches issued                                         */
    int32_t window;       /* window width W used by the chase kernel                             */
    int32_t nlog;         /* entries in the sweep log                                            */
    double ms_hess;       /* periodic Hessenberg-triangular reduction                            */
    double ms_formq;      /* Q formation                                                         */
    double ms_iter;       /* periodic QR iteration                                               */
    double ms_total;      /* device time of the whole call (excludes host<->device copies)       */
    double ms_copy;       /* host<->device copies (host entry points only)                       */
    double bytes_sweeps;  /* algorithmic bytes of all sweeps: sum 2*8*p*w*(2n+1) (wantZ) etc.    */
    double bytes_hess;    /* algorithmic bytes of the reduction: 2*8*p*(5/6)*n^3                 */
    double bytes_formq;   /* 2*8*p*n^3/3                                                         */
    double step_kernel_ms_avg; /* sampled HIP-event duration of the chase kernel (profile mode)  */
    int32_t step_kernel_samples;
    int32_t reserved;
    /* in-kernel cycle accounting of the chase kernel (s_memtime ticks): decide, window load, chase, window
     * store, total; [5] = total in 100 MHz s_memrealtime ticks (shader clock = cyc[4]/cyc[5]*100 MHz) */
    int64_t step_cycles[6];
} psd_stats;

/* context: device selection, stream, workspace cache. One call at a time per context. */
int psd_create(psd_ctx** ctx, int device);
int psd_destroy(psd_ctx* ctx);
/* profile != 0: sample the chase kernel's duration with HIP events (every 16th launch) */
int psd_set_profile(psd_ctx* ctx, int profile);
/* Multishift trains in the real and the complex periodic QR / QZ iteration.  bulges >= 2 (default and maximum 32 — the engines' own defaults: 32 real, 48 complex and real signed, 16 complex signed; PSD_TRAIN in the
 * environment presets it): a sweep of a large active block becomes a train of up to `bulges` double-shift sweeps whose
 * shifts are the eigenvalues of the trailing 2m x 2m block of the product (m <= 8; a longer train runs through the pairs
 * twice), chased as cursors two windows apart by one workgroup each, in windows whose width a cost model picks per train.  0 or 1: the reference's one-shift-one-sweep iteration (PSD.jl:729-763), sweep for sweep.  Same
 * decomposition up to rounding and iteration path; psd_stats.reserved counts the sweeps that ran inside trains. */
int psd_set_train(psd_ctx* ctx, int bulges);
int psd_get_train(psd_ctx* ctx);
/* psd_set_train sets every path (32 or more = every engine's own default); these two address the complex single-shift
 * path alone (its bulges take the eigenvalues of the trailing m x m block of the product as shifts, m <= 16, reused by
 * longer trains; default 48 bulges W positions apart, at most 64) */
int psd_set_train_z(psd_ctx* ctx, int bulges);
int psd_get_train_z(psd_ctx* ctx);
/* the signed paths psd_d_pschur(A, S) / psd_z_pschur(A, S) (double-shift sweeps of rgeneralized.jl:806-1054, single-shift
 * sweeps of generalized.jl:808-852; the complex one takes the eigenvalues of the trailing m x m block of H_1 T): trains with explicit shifts
 * taken from the trailing 2m x 2m block of prod_{l>=2} H_l^{s_l} * H_1 (default 32, the complex one stops at 16; psd_set_train sets this path too,
 * PSD_TRAIN_G presets it alone).  psd_stats.maxits counts the sweeps that ran inside trains.  -2 (test hook): single
 * sweeps started from explicit shifts instead of the implicit _qzrots start. */
int psd_set_train_g(psd_ctx* ctx, int bulges);
int psd_get_train_g(psd_ctx* ctx);
const char* psd_version(void);
/* 1 if the multi-stream periodic Hessenberg reductions of this context (phessenberg!, PSD.jl:213-259, for p >= 32,
 * n >= 512 or when forced) take the pipe form — consecutive chain launches overlapping on two streams —, 0 if they run
 * back to back.  Fixed for the life of the context at psd_create (a context created while no other context of the
 * process is alive gets the pipe form; PSD_H2_PIPE=0 / 2 in the environment forbids / forces it) and forced on by
 * psd_set_shard with world > 1, so that every rank of a period-sharded call runs the same form: the two forms round
 * differently (plain sum of squares against the scaled form of the norm). */
int psd_get_hess_pipe(psd_ctx* ctx);
/* Factor-sliced sweep windows of the real periodic QR iteration (PSD.jl:806-886): `slices` = G >= 2 workgroups chase one
 * window, workgroup g holding the diagonal window blocks of the factors of ITS contiguous slice of the period,
 * (g p/G, (g+1) p/G], and the chain vectors of a position handed from slice to slice as tagged records in the receiver's
 * inbox — the north_star partition (H_j by period, hand-off at slice boundaries) with the G compute
 * units of a slot as the ranks; an inbox is a plain device pointer, across GPUs it would be a peer mapping.  The
 * result does not depend on the number of slices (the reflectors are functions of the vectors handed over: G = 2 and
 * G = 4 agree to the bit) and agrees with slices = 1 to rounding.  1 (default): off.
 * Honoured for p <= 64 and at least two factors per slice, and clamped to what can be resident together (64 x G
 * workgroups, one per compute unit: G <= 4 on the 256 CUs of one MI355X); every wait is bounded, a hand-over that never arrives ends
 * the call with PSD_INFO_RUNTIME.  DESIGN.md section 7c. */
int psd_set_slices(psd_ctx* ctx, int slices);
int psd_get_slices(psd_ctx* ctx);
/* Period sharding over `world` contexts (one per GPU, one process each): every context runs the
 * latency-bound chains (Hessenberg links, window chases) and the updates of the factors H_j they read — identical on
 * all ranks, bit for bit (the tick schedule is reproducible: tests/test_gpu_headline.py, tests/test_gpu_shard.py) — while the
 * Schur vectors, half of all bulk bytes, are split by period: the context forms and updates only the Z_j of its
 * contiguous slice of the period.  No per-tick exchange; the caller all-gathers the slices at the end if it wants every
 * Z_j everywhere (periodicschurdecompositions.jl_amd/sharded.py does, over torch.distributed: RCCL on the GPUs, gloo in
 * the CPU test).  psd_shard_owned: owned[s] = 1 for the user slots s (0-based) of Z this context holds after a call with
 * `orient`.  Honoured by psd_d_pschur / _dev / _hess (Q formation and every Z update), by psd_z_pschur / _dev / _hess
 * (the same: BASELINE configs[2]) and by the iterations of psd_d_gpschur / the signed psd_z_pschur (their Hessenberg
 * stage accumulates Q on every rank); rank 0 of world 1 (default) = everything. */
int psd_set_shard(psd_ctx* ctx, int rank, int world);
int psd_shard_owned(psd_ctx* ctx, int p, char orient, uint8_t* owned);

/* phessenberg!(A)  — PeriodicSchurDecompositions.jl:213-259.
 * A[j] overwritten LAPACK-style (H_j in the upper part, reflectors below), tau is [p][n]
 * (tau[0][n-1] unused, tau[j>=1][n-1] = 0) exactly as the Hessenberg / QR objects the reference
 * returns are laid out. */
int psd_d_phessenberg(psd_ctx* ctx, int n, int p, double* const* A, double* tau, psd_stats* stats, int* info);

/* pschur!(A, lr; wantZ, wantT, maxitfac), Float64 — PeriodicSchurDecompositions.jl:120-152.
 * S must be NULL or all-true here (PSD_INFO_NOTIMPL otherwise): the signed case returns eigenvalues in the scaled
 * (alpha, beta, scale) form and has its own entry, psd_d_gpschur.
 * On exit A[s] holds the user-order factor T_s; the quasi-triangular one is A[*schurindex - 1]
 * (schurindex = 1 for 'R', p for 'L').  Z[s] (p pointers, may be NULL when !wantZ) receive Z_s.
 * wr/wi: n eigenvalues of the product.  sweeplog: optional [3*maxlog] (kind,l,i) per iteration. */
int psd_d_pschur(psd_ctx* ctx, int n, int p, double* const* A, const uint8_t* S, char orient, int wantT, int wantZ,
                 int maxitfac, double* const* Z, double* wr, double* wi, int* schurindex, psd_stats* stats,
                 int32_t* sweeplog, int64_t maxlog, int* info);

/* pschur!(H1, Hs; wantT, wantZ, Q, maxitfac, rev) — PeriodicSchurDecompositions.jl:322-330.
 * H[0] upper Hessenberg, H[1..p-1] upper triangular (internal order).  Q: p pointers holding Q_j
 * on entry (post-multiplied in place and returned as Z_j), or NULL for Z_j = accumulated
 * transformations only (then Zout receives them if wantZ).  With rev != 0 the caller permutes the
 * result as the reference does at :1078-1092 (the kernel work is identical). */
int psd_d_pschur_hess(psd_ctx* ctx, int n, int p, double* const* H, double* const* Q, int wantT, int wantZ,
                      int maxitfac, double* wr, double* wi, psd_stats* stats, int32_t* sweeplog, int64_t maxlog,
                      int* info);

/* nb Hessenberg-triangular problems of the same shape (n, p) in ONE call — what the Krylov driver of the reference issues
 * one by one (krylov.jl:575-592,645,710,800-829: projected problems of order <= 40): pschur!(H1, Hs; wantT, wantZ, Q,
 * maxitfac) for each.  H / Q: nb * p pointers, problem q's factor j at [q * p + j] (H[q * p] upper Hessenberg, the
 * others upper triangular); Q may be NULL when !wantZ, otherwise it holds Q_j on entry and Z_j on exit.  wr / wi: nb * n
 * eigenvalues, problem by problem.  infos[nb] (may be NULL): per-problem info; the return value is the first non-zero
 * one.  nb <= 32.  The problems run side by side on the slot scheduler of the real iteration. */
int psd_d_pschur_hess_batch(psd_ctx* ctx, int nb, int n, int p, double* const* H, double* const* Q, int wantT, int wantZ,
                            int maxitfac, double* wr, double* wi, int* infos, psd_stats* stats, int* info);

/* nb GENERAL (unreduced) problems of the same shape (n, p) in ONE call, Float64, all-true signature: parameter sweeps and
 * multiple-shooting orbits of order 8 ... 64 issue hundreds of them, and one such problem leaves the device launch-bound.
 * phessenberg!(A) (PeriodicSchurDecompositions.jl:213-259) for each: A: nb * p pointers, problem q's factor j at
 * [q * p + j], overwritten LAPACK-style like psd_d_phessenberg; tau is [nb][p][n].  One workgroup reduces one problem, the
 * whole batch in one launch (orders above 128 fall back to the single-problem reduction, problem by problem): H and tau
 * equal, bit for bit, what psd_d_phessenberg's one-launch-per-link form gives.  Any nb >= 1; a batch larger than the
 * device memory is worked through in groups. */
int psd_d_phessenberg_batch(psd_ctx* ctx, int nb, int n, int p, double* const* A, double* tau, psd_stats* stats,
                            int* info);

/* pschur!(A, lr; wantZ, wantT, maxitfac) (PeriodicSchurDecompositions.jl:120-152) for each of nb problems.  A / Z: nb * p
 * pointers in user order, problem q's factor s at [q * p + s]; on exit as psd_d_pschur leaves them (Z may be NULL when
 * !wantZ).  wr / wi: nb * n eigenvalues, problem by problem.  schurindex: 1 for 'R', p for 'L', the same for every
 * problem.  infos[nb] (may be NULL): per-problem info — a problem that exhausts its sweep budget ends alone, the others
 * are complete; the return value is the first non-zero one.  Argument errors and PSD_INFO_RUNTIME codes end the call.
 * The reduction and the Q formation run over the whole batch, the iteration in chunks of 32 problems side by side on the
 * slot scheduler.  stats: the times are sums over the call, the counters sums over the problems. */
int psd_d_pschur_batch(psd_ctx* ctx, int nb, int n, int p, double* const* A, char orient, int wantT, int wantZ,
                       int maxitfac, double* const* Z, double* wr, double* wi, int* infos, int* schurindex,
                       psd_stats* stats, int* info);

/* Device-resident variant of psd_d_pschur_batch: dA, dZ are device pointers to [nb][p][n][n] column-major blocks in
 * user order (dZ may be NULL when !wantZ).  wr / wi / infos are host buffers. */
int psd_d_pschur_batch_dev(psd_ctx* ctx, int nb, int n, int p, double* dA, char orient, int wantT, int wantZ,
                           int maxitfac, double* dZ, double* wr, double* wi, int* infos, int* schurindex,
                           psd_stats* stats, int* info);

/* ---- the same batch entries for ComplexF64, all signatures +1 -----------------------------------------------------
 * Matrices and tau are interleaved (re, im) pairs, column-major; eigenvalues come in the scaled form of psd_z_pschur:
 * alpha (nb * n pairs), beta and ascale (nb * n), problem by problem, lambda = alpha / beta * 2^ascale.  One workgroup
 * reduces one problem and forms one Q_j (as the real entries); the iteration — the single-shift periodic QZ of
 * generalized.jl:166-931 — runs ONE WAVEFRONT PER PROBLEM from the first deflation test to the phase normalisation in a
 * single launch per group, so a problem's result does not depend on its place in the batch.  Orders above 128 run the
 * single call's reduction, Q formation and iteration problem by problem on the batch buffer.  Any nb >= 1; a batch larger
 * than the device memory is worked through in groups.  infos[nb] (may be NULL): per-problem info — PSD_INFO_NOCONV +
 * level for a problem that exhausts its sweep budget, PSD_INFO_RUNTIME + k for one whose in-kernel loop hit its bound;
 * the others are complete.  The return value is the first non-zero per-problem code, or a call-wide code.
 *
 * psd_z_phessenberg_batch: as psd_d_phessenberg_batch; H and tau equal, bit for bit, what psd_z_phessenberg's
 * one-launch-per-link form gives.  info: -1 ctx; -2 nb < 1; -3 n; -4 p; -5 A NULL; -6 tau NULL. */
int psd_z_phessenberg_batch(psd_ctx* ctx, int nb, int n, int p, double* const* A, double* tau, psd_stats* stats,
                            int* info);
/* pschur!(A::Vector{Matrix{ComplexF64}}, lr) for each of nb problems, as psd_d_pschur_batch.  info: -1 ctx; -2 nb < 1;
 * -3 n; -4 p; -5 A NULL; -6 orient; -9 maxitfac < 1; -10 wantZ without Z; -11 alpha, beta or ascale NULL. */
int psd_z_pschur_batch(psd_ctx* ctx, int nb, int n, int p, double* const* A, char orient, int wantT, int wantZ,
                       int maxitfac, double* const* Z, double* alpha, double* beta, int32_t* ascale, int* infos,
                       int* schurindex, psd_stats* stats, int* info);
/* Device-resident variant: dA, dZ device [nb][p][n][n] column-major complex blocks in user order (dZ may be NULL when
 * !wantZ), overwritten; alpha / beta / ascale / infos are host buffers.  Argument codes as psd_z_pschur_batch. */
int psd_z_pschur_batch_dev(psd_ctx* ctx, int nb, int n, int p, double* dA, char orient, int wantT, int wantZ,
                           int maxitfac, double* dZ, double* alpha, double* beta, int32_t* ascale, int* infos,
                           int* schurindex, psd_stats* stats, int* info);
/* nb Hessenberg-triangular ComplexF64 problems (pschur!(H1, Hs, S; wantT, wantZ, Q, maxitfac) with S all true): H / Q
 * as psd_d_pschur_hess_batch (Q may be NULL when !wantZ, otherwise Q_j on entry and Z_j on exit), any nb >= 1.
 * info: -1 ctx; -2 nb < 1; -3 n; -4 p; -5 H NULL; -6 wantZ without Q; -9 maxitfac < 1; -10 alpha, beta or ascale NULL. */
int psd_z_pschur_hess_batch(psd_ctx* ctx, int nb, int n, int p, double* const* H, double* const* Q, int wantT, int wantZ,
                            int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos, psd_stats* stats,
                            int* info);

/* ---- the same batch entries for ComplexF64 with a SIGNED signature ------------------------------------------------
 * pschur!(A, S, lr) of generalized.jl:108-148 — the path behind gpschur(As, Bs), the generalized periodic eigenproblem
 * B_p^-1 A_p ... B_1^-1 A_1 (one pair: the QZ problem of a pencil) — for nb problems of one shape (n, p) and ONE
 * signature S (p bytes, user order, non-zero = +1) per call.  Conventions as the all-true entries above.  One workgroup
 * runs stage 1 of one problem's signed Hessenberg reduction (generalized.jl:988-1033); stage 2 (:1034-1079) and the
 * signed periodic QZ iteration run ONE WAVEFRONT PER PROBLEM, one launch each per group, so a problem's result does not
 * depend on its place in the batch.  Orders above 128 run the single call's reduction and iteration problem by problem
 * on the batch buffer.  An all-true or NULL S takes the all-true entries' path: the results are then theirs, bit for
 * bit.  infos[nb] (may be NULL): PSD_INFO_NOCONV + level for a problem that exhausts its sweep budget,
 * PSD_INFO_RUNTIME + 77 for a rotation list that overflowed, PSD_INFO_RUNTIME + 0xfffe for one whose in-kernel loop hit
 * its bound; the others are complete.  The return value is the first non-zero per-problem code, or a call-wide code.
 * stats: the times are sums over the call, the counters sums over the problems (reserved = ncase2 + 1000 * ncase3,
 * summed as the two counts).
 * info (all four): -1 ctx; -2 nb < 1; -3 n; -4 p; -5 A / H NULL; -6 orient (psd_z_gpschur_hess_batch: wantZ without Q);
 * -7 the entry of S that lands leftmost in working order (S[0] for 'R' and the two Hessenberg entries, S[p-1] for 'L')
 * is false; -9 maxitfac < 1; -10 wantZ without Z; -11 alpha, beta or ascale NULL.
 *
 * psd_z_gphessenberg_batch: _phessenberg!(A, S; wantQ) for each problem, as psd_z_gphessenberg: A (nb * p pointers)
 * overwritten by H_l, Q (nb * p pointers, or NULL) receives Qs[l]. */
int psd_z_gphessenberg_batch(psd_ctx* ctx, int nb, int n, int p, double* const* A, const uint8_t* S, double* const* Q,
                             psd_stats* stats, int* info);
/* pschur!(A::Vector{Matrix{ComplexF64}}, S, lr) for each of nb problems: A / Z nb * p pointers in user order, as
 * psd_z_pschur_batch; schurindex: 1 for 'R', p for 'L'. */
int psd_z_gpschur_batch(psd_ctx* ctx, int nb, int n, int p, double* const* A, const uint8_t* S, char orient, int wantT,
                        int wantZ, int maxitfac, double* const* Z, double* alpha, double* beta, int32_t* ascale, int* infos,
                        int* schurindex, psd_stats* stats, int* info);
/* Device-resident variant: dA, dZ device [nb][p][n][n] column-major complex blocks in user order (dZ may be NULL when
 * !wantZ), overwritten; S, alpha / beta / ascale / infos are host buffers. */
int psd_z_gpschur_batch_dev(psd_ctx* ctx, int nb, int n, int p, double* dA, const uint8_t* S, char orient, int wantT,
                            int wantZ, int maxitfac, double* dZ, double* alpha, double* beta, int32_t* ascale, int* infos,
                            int* schurindex, psd_stats* stats, int* info);
/* nb Hessenberg-triangular ComplexF64 problems with the signature S (internal order): pschur!(H1, Hs, S; wantT, wantZ,
 * Q, maxitfac) for each; H / Q as psd_z_pschur_hess_batch. */
int psd_z_gpschur_hess_batch(psd_ctx* ctx, int nb, int n, int p, double* const* H, const uint8_t* S, double* const* Q,
                             int wantT, int wantZ, int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos,
                             psd_stats* stats, int* info);

/* ---- the same batch entries for Float64 with a signature -----------------------------------------------------------
 * pschur!(A, S, lr) of rgeneralized.jl:3-45 (the MB03BD-type real periodic QZ) — pencils A - lambda B and generalized
 * periodic products B_p^-1 A_p ... B_1^-1 A_1 with real data — for nb problems of one shape (n, p) and ONE signature S
 * per call, without the detour through ComplexF64: the factor at schurindex comes out real quasi-triangular (a 2 x 2
 * block per conjugate pair, a zero sub-diagonal wherever the eigenvalue is real), the others upper triangular, the Z_l
 * real orthogonal, and the alpha of a 2 x 2 block are exact conjugates.  Argument layout (n * n doubles per matrix),
 * info codes (-1 ... -11, as listed above), per-problem infos, return value and stats conventions are those of the four
 * psd_z_g*_batch entries; alpha is nb * n complex pairs, beta and ascale nb * n, eigenvalue = alpha / beta * 2^ascale.
 * stats: reserved = ncase2 + 1000 * ncase3, ndefl2 counts 2 x 2 blocks (of both kinds), nrqpass zero-shift passes, each
 * summed over the problems.  One difference from the complex entries: a NULL or all-true S runs the SAME signed real
 * kernels (as psd_d_gpschur does, and pschur!(A, S, lr) for real element types); it is not sent to psd_d_pschur_batch,
 * whose outputs (wr, wi) have another form.  Stage 1 of the reduction runs one workgroup per problem, stage 2 and the
 * iteration ONE WAVEFRONT PER PROBLEM (single-wave sweep, no trains), one launch each per group; nothing is shared
 * between problems, so a result does not depend on its place in the batch.  Orders above 128 run psd_d_gpschur's
 * reduction and iteration problem by problem on the batch buffer.  A period-sharded context: PSD_INFO_NOTIMPL. */
int psd_d_gphessenberg_batch(psd_ctx* ctx, int nb, int n, int p, double* const* A, const uint8_t* S, double* const* Q,
                             psd_stats* stats, int* info);
int psd_d_gpschur_batch(psd_ctx* ctx, int nb, int n, int p, double* const* A, const uint8_t* S, char orient, int wantT,
                        int wantZ, int maxitfac, double* const* Z, double* alpha, double* beta, int32_t* ascale, int* infos,
                        int* schurindex, psd_stats* stats, int* info);
/* Device-resident variant: dA, dZ device [nb][p][n][n] column-major real blocks in user order (dZ may be NULL when
 * !wantZ), overwritten; S, alpha / beta / ascale / infos are host buffers. */
int psd_d_gpschur_batch_dev(psd_ctx* ctx, int nb, int n, int p, double* dA, const uint8_t* S, char orient, int wantT,
                            int wantZ, int maxitfac, double* dZ, double* alpha, double* beta, int32_t* ascale, int* infos,
                            int* schurindex, psd_stats* stats, int* info);
/* nb Hessenberg-triangular Float64 problems with the signature S (internal order, NULL: all true): pschur!(H1, Hs, S;
 * wantT, wantZ, Q, maxitfac) for each, as psd_d_gpschur_hess; H / Q as psd_d_pschur_hess_batch. */
int psd_d_gpschur_hess_batch(psd_ctx* ctx, int nb, int n, int p, double* const* H, const uint8_t* S, double* const* Q,
                             int wantT, int wantZ, int maxitfac, double* alpha, double* beta, int32_t* ascale, int* infos,
                             psd_stats* stats, int* info);

/* Device-resident variant of psd_d_pschur: dA, dZ are device pointers to [p][n][n] blocks in user
 * order (dZ may be NULL when !wantZ).  wr/wi/sweeplog are host buffers. */
int psd_d_pschur_dev(psd_ctx* ctx, int n, int p, double* dA, char orient, int wantT, int wantZ, int maxitfac,
                     double* dZ, double* wr, double* wi, int* schurindex, psd_stats* stats, int32_t* sweeplog,
                     int64_t maxlog, int* info);

/* ---- ComplexF64 (interleaved re,im; same conventions) ---------------------------------------------
 * Eigenvalues are returned in the reference's scaled form (generalized.jl:40-42,74-76):
 * values[k] = alpha[k] / beta[k] * 2^ascale[k], alpha interleaved complex. */

/* phessenberg!(A) for ComplexF64 — PeriodicSchurDecompositions.jl:213-259; tau is [p][n] complex */
int psd_z_phessenberg(psd_ctx* ctx, int n, int p, double* const* A, double* tau, psd_stats* stats, int* info);

/* pschur!(A::Vector{Matrix{ComplexF64}}, lr; wantZ, wantT) — PeriodicSchurDecompositions.jl:1106-1111, which runs
 * generalized.jl:108-137 with S = trues; with a signed S the signed Hessenberg reduction and the signed periodic QZ of
 * generalized.jl:138-146 run (the leftmost entry of S in working order must be true, info -5). */
int psd_z_pschur(psd_ctx* ctx, int n, int p, double* const* A, const uint8_t* S, char orient, int wantT, int wantZ,
                 int maxitfac, double* const* Z, double* alpha, double* beta, int32_t* ascale, int* schurindex,
                 psd_stats* stats, int32_t* sweeplog, int64_t maxlog, int* info);

/* pschur!(H1, Hs, S; wantT, wantZ, Q, maxitfac, rev) for ComplexF64 — generalized.jl:166-175 */
int psd_z_pschur_hess(psd_ctx* ctx, int n, int p, double* const* H, const uint8_t* S, double* const* Q, int wantT,
                      int wantZ, int maxitfac, double* alpha, double* beta, int32_t* ascale, psd_stats* stats,
                      int32_t* sweeplog, int64_t maxlog, int* info);

/* pschur!(H1, Hs, S; wantT, wantZ, Q, maxitfac) for Float64 with a signature — rgeneralized.jl:49-59 (MB03BD type
 * real periodic QZ).  H[0] Hessenberg, H[1..p-1] upper triangular, S[0] must be true (rgeneralized.jl:73, info -5);
 * Q (p matrices) is accumulated when wantZ; alpha is complex (2n doubles), values = alpha / beta * 2^ascale.
 * stats->reserved = ncase2 + 1000 * ncase3, ndefl2 = 2x2 blocks, nrqpass = zero-shift passes. */
int psd_d_gpschur_hess(psd_ctx* ctx, int n, int p, double* const* H, const uint8_t* S, double* const* Q, int wantT,
                       int wantZ, int maxitfac, double* alpha, double* beta, int32_t* ascale, psd_stats* stats,
                       int32_t* sweeplog, int64_t maxlog, int* info);

/* _phessenberg!(A, S; wantQ) for Float64 — generalized.jl:988-1082: signed periodic Hessenberg-triangular reduction.
 * A[l] is overwritten by H_l (H_1 Hessenberg, the others upper triangular), Q[l] (may be NULL) receives Qs[l]:
 * A_l = Q_l H_l Q_{l+1}' for S[l], A_l = Q_{l+1} H_l Q_l' for !S[l].  S[0] must be true (info -5). */
int psd_d_gphessenberg(psd_ctx* ctx, int n, int p, double* const* A, const uint8_t* S, double* const* Q,
                       psd_stats* stats, int* info);

/* pschur!(A, S, lr; wantZ, wantT) for Float64 — rgeneralized.jl:3-45.  User-order in/out as psd_d_pschur; the entry of
 * S that lands leftmost in the working order (S[0] for 'R', S[p-1] for 'L') must be true (info -5, :37). */
int psd_d_gpschur(psd_ctx* ctx, int n, int p, double* const* A, const uint8_t* S, char orient, int wantT, int wantZ,
                  int maxitfac, double* const* Z, double* alpha, double* beta, int32_t* ascale, int* schurindex,
                  psd_stats* stats, int* info);

/* _phessenberg!(A, S; wantQ) for ComplexF64 — generalized.jl:988-1082 (see psd_d_gphessenberg) */
int psd_z_gphessenberg(psd_ctx* ctx, int n, int p, double* const* A, const uint8_t* S, double* const* Q,
                       psd_stats* stats, int* info);

/* device-resident variant of psd_z_pschur */
int psd_z_pschur_dev(psd_ctx* ctx, int n, int p, double* dA, char orient, int wantT, int wantZ, int maxitfac,
                     double* dZ, double* alpha, double* beta, int32_t* ascale, int* schurindex, psd_stats* stats,
                     int32_t* sweeplog, int64_t maxlog, int* info);

/* LinearAlgebra.ordschur!(P::PeriodicSchur{ComplexF64}, select; wantZ) — ordschur.jl:11-73: move the selected
 * eigenvalues (select[j] != 0) and their subspace to the top by adjacent swaps (sylswap.jl:542-635).
 * T: p pointers, the full user-order factor list with T1 at position `schurindex`; Z: p pointers (or NULL with
 * !wantZ); both updated in place.  schurindex must be 1 or p (info -7 otherwise, ordschur.jl:32); all four
 * alignments of the reference (utils.jl:6-85: _rev_alias, _circshift) are mapped onto the same working form.
 * Eigenvalues are recomputed from the diagonals (ordschur.jl:97-120) in scaled form.
 * info: 0; PSD_INFO_ILLCOND + j  IllConditionedException(j) (ordschur.jl:61); PSD_INFO_SINGULAR (utils.jl:128). */
#define PSD_INFO_ILLCOND 2000
#define PSD_INFO_SINGULAR 3000
int psd_z_ordschur(psd_ctx* ctx, int n, int p, double* const* T, double* const* Z, char orient, int schurindex,
                   const uint8_t* select, int wantZ, double* alpha, double* beta, int32_t* ascale, psd_stats* stats,
                   int* info);

/* LinearAlgebra.ordschur!(P::PeriodicSchur{Float64}, select; wantZ) — rordschur.jl:3-132 (1x1 and 2x2 blocks;
 * a selected member of a conjugate pair takes its partner along, :46-75).  Same conventions as psd_z_ordschur;
 * eigenvalues are returned as wr + i*wi (ordschur.jl:122-204). */
int psd_d_ordschur(psd_ctx* ctx, int n, int p, double* const* T, double* const* Z, char orient, int schurindex,
                   const uint8_t* select, int wantZ, double* wr, double* wi, psd_stats* stats, int* info);

/* LinearAlgebra.ordschur!(P::GeneralizedPeriodicSchur, select; wantZ) by adjacent 1x1 swaps — ordschur.jl:11-96,
 * 323-328, signed swap sylswap.jl:638-764.  T/Z: p matrices in the user order of the decomposition (T1 at
 * `schurindex`), S the user-order signature; eigenvalues are recomputed in the scaled form.  info as psd_z_ordschur.
 * psd_d_gordschur (Float64): rordschur.jl:3-132,141-268 with the signed block swap sylswap.jl:197-538 for 2x2 blocks
 * (conjugate pairs; `select` is completed to pairs) and ordschur.jl:206-314 for the eigenvalues; a decomposition with
 * a real spectrum (T1 triangular) goes through the 1x1 kernel. */
int psd_z_gordschur(psd_ctx* ctx, int n, int p, double* const* T, double* const* Z, const uint8_t* S, char orient,
                    int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta, int32_t* ascale,
                    psd_stats* stats, int* info);
int psd_d_gordschur(psd_ctx* ctx, int n, int p, double* const* T, double* const* Z, const uint8_t* S, char orient,
                    int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta, int32_t* ascale,
                    psd_stats* stats, int* info);

/* _rphessenberg!(Ap, A, Q) — rhessx.jl:55-109 (called by the Krylov driver, krylov.jl:809): row-wise periodic Hessenberg
 * reduction for the left orientation.  Ap: m x n column-major (ld m), m = n or n + 1 (info -2 otherwise, :62), reduced to
 * upper Hessenberg form; A: p-1 pointers to n x n matrices, reduced to upper triangular; Q: p pointers to nq x nqc
 * matrices (nqc >= n), post-multiplied by the accumulated reflectors, or NULL.  All updated in place.
 * psd_z_*: ComplexF64 (interleaved). */
int psd_d_rphessenberg(psd_ctx* ctx, int m, int n, int p, double* Ap, double* const* A, double* const* Q, int nq, int nqc,
                       int* info);
int psd_z_rphessenberg(psd_ctx* ctx, int m, int n, int p, double* Ap, double* const* A, double* const* Q, int nq, int nqc,
                       int* info);

/* checkpsd(P, As; thresh, strict) — diagnostics.jl:190-263 — as a device-side verifier (matrix cores: three n x n x n
 * FP64 products per factor).  T, Z, A: p pointers each, USER order of the decomposition (T[schurindex-1] is the
 * quasi-triangular factor), S the user-order signature (NULL = all true), wi (real variant, may be NULL) the imaginary
 * parts of P.values (non-zero subdiagonals below real eigenvalues are only a warning in the reference, :223-230).
 * err[p]: ||Z_a T_l Z_b' - A_l||_F / eps / opnorm(A_l, 1) with (a, b) by the signature and orientation (:247-252);
 * orth[p] / tri[p] (may be NULL): ||Z_l Z_l' - I||_F and ||tril(T_l, -1 or -2)||_F; *ok: the reference's Bool
 * (tri <= (strict ? 0 : 10 eps n), orth <= 10 eps n, err <= thresh).  psd_z_*: ComplexF64 interleaved.
 * psd_d_checkpsd_dev: operands already in HBM as [p][n][n] blocks in user order. */
int psd_d_checkpsd(psd_ctx* ctx, int n, int p, double* const* T, double* const* Z, double* const* A, const uint8_t* S,
                   char orient, int schurindex, const double* wi, double thresh, int strict, double* err, double* orth,
                   double* tri, int* ok, int* info);
int psd_z_checkpsd(psd_ctx* ctx, int n, int p, double* const* T, double* const* Z, double* const* A, const uint8_t* S,
                   char orient, int schurindex, double thresh, int strict, double* err, double* orth, double* tri, int* ok,
                   int* info);
int psd_d_checkpsd_dev(psd_ctx* ctx, int n, int p, const double* dT, const double* dZ, const double* dA,
                       const uint8_t* S, char orient, int schurindex, double thresh, int strict, double* err,
                       double* orth, double* tri, int* ok, int* info);
/* The ComplexF64 twin of psd_d_checkpsd_dev: [p][n][n] blocks of interleaved (re, im) doubles, same codes. */
int psd_z_checkpsd_dev(psd_ctx* ctx, int n, int p, const double* dT, const double* dZ, const double* dA,
                       const uint8_t* S, char orient, int schurindex, double thresh, int strict, double* err,
                       double* orth, double* tri, int* ok, int* info);

/* ---- partial_pschur: periodic Krylov-Schur for dense factors — src/krylov.jl:446-798 (D. Kressner, Numer. Math. 2006) --
 * A `nev`-order partial periodic Schur decomposition of the product A_p ... A_2 A_1 in the LEFT orientation of the
 * reference (krylov.jl:87-139):  A_l Z_l = Z_{l+1} T_l (l < p),  A_p Z_p = Z_1 T_p,  Z_l n x nconv orthonormal, T_p the
 * quasi-triangular factor (schurindex = p), T_1..T_{p-1} upper triangular.  The factors stay resident on the device; one
 * Krylov step is p matrix-vector products and the orthogonalisation of each result, with the decisions of the
 * Gram-Schmidt rule (re-orthogonalise once when ||w|| < ||r|| / sqrt(2), in span when that still fails) taken on the
 * device and read back once per step.  The projected problems (order <= maxdim) go through the engine's own
 * psd_?_pschur_hess, psd_?_ordschur and psd_?_rphessenberg on the same context.
 *
 * Arguments are the reference's keywords: which = 'M' (LM, largest magnitude), 'R' (LR), 'r' (SR), 'I' (LI), 'i' (SI);
 * mindim / maxdim the kept and the maximal subspace order; tol the convergence tolerance (reference default sqrt(eps));
 * tol1 the null-vector threshold of the start (100 eps); restarts the restart limit (100); purgebuffer (2).  u1 (host, n
 * elements, may be NULL): start vector; without it the start comes from a counter-based generator seeded by `seed` (the
 * reference's `vrand!` cannot cross the ABI), so that a run can be repeated bit for bit.
 *
 * Outputs: *nconv converged Schur vectors (History.nconverged); T: p host buffers of maxdim * maxdim elements, T[l] the
 * nconv x nconv factor T_{l+1} (ld nconv); Z: p buffers of n * maxdim elements, Z[l] the n x nconv block Z_{l+1} (ld n);
 * wr / wi: maxdim entries, the first nconv the eigenvalues (P.values); stats (may be NULL): History and counters.
 *
 * info: 0 (also when not converged: stats->converged = 0, as History.converged); <0 argument -k invalid, checked before
 * the device is touched:
 *   -1 ctx NULL; -2 n < 1; -3 p < 1; -4 A NULL;  -5 nev < 1 (krylov.jl:462); -6 which not one of M R r I i;
 *   -7 not nev <= mindim <= maxdim <= p n (krylov.jl:465-466); -8 maxdim above PSD_KRYLOV_MAXDIM;
 *   -9 u1 zero or not finite; -11 tol not > 0; -12 tol1 < 0; -13 restarts < 0; -14 purgebuffer < 0;
 *   -15 nconv NULL; -16 T NULL; -17 Z NULL; -18 wr or wi NULL;
 * PSD_INFO_PKSFAIL: PKSFailure("Arnoldi reinitialization failed") (krylov.jl:182); PSD_INFO_ILLCOND + j: reordering of
 * the locked Ritz values failed (IllConditionedException(j), which the reference does not catch there, :625);
 * PSD_INFO_RUNTIME + k: HIP runtime failure.
 * ComplexF64 (psd_z_*): A, T, Z, u1 interleaved (re, im); wr / wi still the real and imaginary parts of P.values. */
#define PSD_INFO_PKSFAIL 5000
#define PSD_KRYLOV_MAXDIM 2048

typedef struct psd_krylov_stats {
    int64_t nprods;      /* History.mvproducts: matrix-vector products (p per Krylov step)                    */
    int32_t nconverged;  /* History.nconverged                                                                 */
    int32_t converged;   /* History.converged (nconv >= nev)                                                   */
    int32_t nev;         /* History.nev                                                                        */
    int32_t restarts;    /* restart iterations run                                                             */
    int32_t nreorth;     /* second Gram-Schmidt passes                                                         */
    int32_t nreinit;     /* re-initialised basis vectors (_reinitialize!, krylov.jl:152-182)                   */
    int32_t ndeflate;    /* deflations for a singular factor (_deflate!, krylov.jl:184-226)                    */
    int32_t suspect;     /* 1: the Arnoldi process gave up (> 5 singularities): results suspect (krylov.jl:781)  */
    double ms_arnoldi;   /* Arnoldi extensions: matvecs, orthogonalisation, host reads (host clock)            */
    double ms_proj;      /* projected problems: pschur!, ordschur!, residuals, _rphessenberg! (host clock)      */
    double ms_basis;     /* basis updates V_l <- V_l Q_l (host clock around a synchronise)                     */
    double ms_total;     /* whole call (host entry: including the copies of A and the results)                 */
} psd_krylov_stats;

int psd_d_partial_pschur(psd_ctx* ctx, int n, int p, const double* const* A, int nev, char which, int mindim,
                         int maxdim, const double* u1, uint64_t seed, double tol, double tol1, int restarts,
                         int purgebuffer, int* nconv, double* const* T, double* const* Z, double* wr, double* wi,
                         psd_krylov_stats* stats, int* info);
int psd_z_partial_pschur(psd_ctx* ctx, int n, int p, const double* const* A, int nev, char which, int mindim,
                         int maxdim, const double* u1, uint64_t seed, double tol, double tol1, int restarts,
                         int purgebuffer, int* nconv, double* const* T, double* const* Z, double* wr, double* wi,
                         psd_krylov_stats* stats, int* info);
/* Device-resident variants: dA a device [p][n][n] block (factor-major, not modified), dZ a device [p][n][maxdim] block
 * (Z_{l+1} in the first n * nconv elements of block l, ld n); T, wr, wi, u1 host buffers as above.
 * Alignment: dA may be any 8-byte aligned pointer (a view into a larger allocation at any element offset).  The Float64
 * product reads two rows per lane through 16-byte loads only when n is even AND dA is 16-byte aligned; otherwise it takes
 * the one-row body.  The body decides the column chunking, so the bits of a result depend on n and on that alignment. */
int psd_d_partial_pschur_dev(psd_ctx* ctx, int n, int p, const double* dA, int nev, char which, int mindim, int maxdim,
                             const double* u1, uint64_t seed, double tol, double tol1, int restarts, int purgebuffer,
                             int* nconv, double* const* T, double* dZ, double* wr, double* wi, psd_krylov_stats* stats,
                             int* info);
int psd_z_partial_pschur_dev(psd_ctx* ctx, int n, int p, const double* dA, int nev, char which, int mindim, int maxdim,
                             const double* u1, uint64_t seed, double tol, double tol1, int restarts, int purgebuffer,
                             int* nconv, double* const* T, double* dZ, double* wr, double* wi, psd_krylov_stats* stats,
                             int* info);

/* ---- partial_pschur for sparse factors (CSR) — the reference takes "matrices or any linear maps that implement mul!"
 * (krylov.jl:416-487); the sparse Jacobians of a discretised periodic problem are the linear maps that matter in practice.
 * Factor l is a CSR triple: rowptr[l] (n + 1 entries, int64), colind[l] (rowptr[l][n] entries, int32), both 0-based, and
 * val[l] (as many elements, Float64, or ComplexF64 as interleaved (re, im); the product is plain, not conjugated).  The
 * columns of a row may come in any order and may repeat (repeats add up).  Only the matrix-vector product differs from
 * the dense driver: a device SpMV without floating-point atomics, whose summation order depends on the matrix and on a
 * group width G alone (a row is summed by G consecutive lanes: lane g takes the entries start + g, start + g + G, ... in
 * that order, then a fixed tree runs over the lanes).  G is the smallest power of two >= nnz / n in [1, 64], chosen from
 * n and nnz only, so a run repeats bit for bit on any machine.  A row is never split, so a few very long rows in a very
 * sparse matrix are correct but not fast.  All other arguments, the outputs and the algorithmic info values are those of
 * psd_d_partial_pschur.
 *
 * Argument codes as psd_d_partial_pschur, with: -4 also for a NULL rowptr / colind / val array or a NULL element of one;
 *   -19 rowptr invalid (rowptr[0] != 0, decreasing, or rowptr[n] negative or above 2^40);
 *   -20 a column index outside [0, n).
 * The host entries check the structure on the host before anything is copied.  The `_dev` entries take the same three
 * host arrays, of p DEVICE pointers, and dZ as psd_d_partial_pschur_dev; they read rowptr[n] of every factor and run a
 * structure-check kernel (which reads rowptr and colind and gathers through neither) before any Krylov work, so -19 and
 * -20 come back before an index is ever used as an address. */
int psd_d_partial_pschur_csr(psd_ctx* ctx, int n, int p, const int64_t* const* rowptr, const int32_t* const* colind,
                             const double* const* val, int nev, char which, int mindim, int maxdim, const double* u1,
                             uint64_t seed, double tol, double tol1, int restarts, int purgebuffer, int* nconv,
                             double* const* T, double* const* Z, double* wr, double* wi, psd_krylov_stats* stats,
                             int* info);
int psd_z_partial_pschur_csr(psd_ctx* ctx, int n, int p, const int64_t* const* rowptr, const int32_t* const* colind,
                             const double* const* val, int nev, char which, int mindim, int maxdim, const double* u1,
                             uint64_t seed, double tol, double tol1, int restarts, int purgebuffer, int* nconv,
                             double* const* T, double* const* Z, double* wr, double* wi, psd_krylov_stats* stats,
                             int* info);
int psd_d_partial_pschur_csr_dev(psd_ctx* ctx, int n, int p, const int64_t* const* rowptr, const int32_t* const* colind,
                                 const double* const* val, int nev, char which, int mindim, int maxdim, const double* u1,
                                 uint64_t seed, double tol, double tol1, int restarts, int purgebuffer, int* nconv,
                                 double* const* T, double* dZ, double* wr, double* wi, psd_krylov_stats* stats,
                                 int* info);
int psd_z_partial_pschur_csr_dev(psd_ctx* ctx, int n, int p, const int64_t* const* rowptr, const int32_t* const* colind,
                                 const double* const* val, int nev, char which, int mindim, int maxdim, const double* u1,
                                 uint64_t seed, double tol, double tol1, int restarts, int purgebuffer, int* nconv,
                                 double* const* T, double* dZ, double* wr, double* wi, psd_krylov_stats* stats,
                                 int* info);
/* y = A x for one CSR factor through the driver's own kernel, once: host buffers (x, y: n elements); group = G as above,
 * 0 for the automatic width.  The result has the driver's rounding, so it pins the kernel at a chosen G.
 * info: -1 ctx NULL; -2 n < 1; -4 rowptr, colind or val NULL; -8 group not 0 and not a power of two <= 64; -9 x NULL;
 * -17 y NULL; -19 / -20 as above; PSD_INFO_RUNTIME + k. */
int psd_d_csr_matvec(psd_ctx* ctx, int n, const int64_t* rowptr, const int32_t* colind, const double* val,
                     const double* x, double* y, int group, int* info);
int psd_z_csr_matvec(psd_ctx* ctx, int n, const int64_t* rowptr, const int32_t* colind, const double* val,
                     const double* x, double* y, int group, int* info);

/* ---- diagnostic entries of the dense Krylov kernels -------------------------------------------------------------------
 * TEST PLUMBING, not part of the product's interface and without a Julia binding: each runs kernels of the dense driver
 * once, on host buffers, through the driver's own launch code and launch geometry, so that a test can compare one kernel
 * with a high-precision reference at a chosen shape.  Elements are Float64 (psd_d_*) or ComplexF64 as interleaved (re, im)
 * pairs (psd_z_*); matrices are column-major.  info: <0 argument -k invalid (listed per entry); PSD_INFO_RUNTIME + k.
 *
 * The launch geometry of the driver at order n and subspace order maxdim:
 *   rp      rows per lane of the matvec: 2 for Float64 with n even and a 16-byte aligned factor pointer, else 1;
 *   tiles   = ceil(n / (256 rp)) row tiles of the matvec;
 *   nchunk, ccols: column chunks of the matvec and their width: nchunk0 = max(1, min(ceil(1024 / tiles), ceil(n / 32))),
 *           ccols = ceil(n / nchunk0), nchunk = ceil(n / ccols) (the last chunk holds n - (nchunk - 1) ccols columns);
 *   nblk    = ceil(n / 256) workgroups of the row kernels;  ldp = maxdim + 2, the pitch of their partial sums. */
typedef struct psd_krylov_geom {
    int32_t rp, tiles, nchunk, ccols, nblk, ldp;
} psd_krylov_geom;

/* y = A x as the driver forms it: the chunked product (psd_kr_mv), then the in-order sum of the chunks (psd_kr_dots).
 * A: n x n; a_dev = 0: a host buffer, copied to a fresh (16-byte aligned) device allocation; a_dev = 1: a device pointer,
 * read in place under the alignment rule of psd_d_partial_pschur_dev.  x, y: host, n elements.  geom (may be NULL)
 * receives the geometry used (ldp as for maxdim = 0).
 * info: -1 ctx NULL; -2 n < 1; -4 A NULL; -8 a_dev not 0 or 1; -9 x NULL; -17 y NULL. */
int psd_d_dense_matvec(psd_ctx* ctx, int n, const double* A, int a_dev, const double* x, double* y,
                       psd_krylov_geom* geom, int* info);
int psd_z_dense_matvec(psd_ctx* ctx, int n, const double* A, int a_dev, const double* x, double* y,
                       psd_krylov_geom* geom, int* info);
/* One orthogonalise-normalise-store stage of the driver (geometry of maxdim = ncols, null-vector threshold 100 eps):
 * v against the ncols columns of U (n x ncols, orthonormal), classical Gram-Schmidt with the conditional second pass.
 * h (ncols elements) and *hjj receive the column of the projected factor (its last entry is 0 when the stage stopped);
 * unew (n elements) is uploaded as column ncols of the basis and read back after the stage, and U is read back as well,
 * so a caller sees what the stage wrote and what it left alone.  state[0] = 1 when the stage stopped the step,
 * state[1] = its kind (1: v in the span of U; 2: null vector, ncols = 0 only), state[2] = 1 when the second pass ran,
 * state[3] = nblk.
 * info: -1 ctx NULL; -2 n < 1; -3 ncols < 0 or > PSD_KRYLOV_MAXDIM; -4 U NULL with ncols > 0; -5 v NULL; -6 h NULL with
 * ncols > 0; -7 hjj NULL; -8 unew NULL; -9 state NULL. */
int psd_d_kr_orth(psd_ctx* ctx, int n, int ncols, double* U, const double* v, double* h, double* hjj, double* unew,
                  int32_t* state, int* info);
int psd_z_kr_orth(psd_ctx* ctx, int n, int ncols, double* U, const double* v, double* h, double* hjj, double* unew,
                  int32_t* state, int* info);
/* The in-place basis update V_l[:, a0:a0+m) <- V_l[:, a0:a0+m) Q_l for l = 0..p-1 in one launch.  V: [p][n][ldv_cols]
 * (ld n), Q: [p][m][m].  *R (may be NULL) receives the rows per workgroup: the tile of R x m elements is staged in LDS,
 * R = max(1, min(64, 65536 / (m * element bytes))).
 * info: -1 ctx NULL; -2 n < 1; -3 p < 1; -4 ldv_cols < 1; -5 a0 < 0; -6 m < 1, m > PSD_KRYLOV_MAXDIM or
 * a0 + m > ldv_cols; -7 V NULL; -8 Q NULL. */
int psd_d_kr_basis(psd_ctx* ctx, int n, int p, int ldv_cols, int a0, int m, double* V, const double* Q, int32_t* R,
                   int* info);
int psd_z_kr_basis(psd_ctx* ctx, int n, int p, int ldv_cols, int a0, int m, double* V, const double* Q, int32_t* R,
                   int* info);

/* ---- diagnostic entry of the scalar device routines -------------------------------------------------------------------
 * TEST PLUMBING, not part of the product's interface and without a Julia binding: one kernel runs once, lane t of
 * workgroup t / 64 evaluates case t by calling the routine the engine's chains call (reflectors, Givens rotations, the
 * reflector scalars of the look-ahead Hessenberg reduction, the power-of-two rescaling of the scan chase, and the
 * reciprocal / root forms under them), so that a test can compare each with exact arithmetic one call at a time.
 * in, out: host, ncases rows of 8 doubles; slots an op does not name are ignored on input and zero on output.  The raw
 * forms promise their accuracy only for the arguments their callers' range guards admit; NaN and Inf inputs are outside
 * every routine's contract.  Complex values are (re, im) in consecutive slots.
 * info: -1 ctx NULL; -2 unknown op; -3 ncases < 1; -4 in NULL; -5 out NULL; PSD_INFO_RUNTIME + k. */
typedef enum psd_diag_scalar_op {
    PSD_DS_RCP = 0,              /* psd_rcp_fast:        (x)                  -> (1/x) */
    PSD_DS_SQRT_PAIR = 1,        /* psd_sqrt_pair_fast:  (s)                  -> (sqrt s, 1/sqrt s) */
    PSD_DS_RSQRT2 = 2,           /* psd_rsqrt2_fast:     (a, b)               -> (1/sqrt a, 1/sqrt b) */
    PSD_DS_REFL2 = 3,            /* psd_refl2:           (x0, x1)             -> (beta, v1, tau) */
    PSD_DS_REFL3 = 4,            /* psd_refl3:           (x0, x1, x2)         -> (beta, v1, v2, tau) */
    PSD_DS_REFL2_LEAN = 5,       /* psd_refl2_lean:      as PSD_DS_REFL2 */
    PSD_DS_REFL3_LEAN = 6,       /* psd_refl3_lean:      as PSD_DS_REFL3 */
    PSD_DS_REFL32_PAIR = 7,      /* psd_refl32_pair:     (x0, x1, x2, y0, y1) -> (beta, v1, v2, tau, beta', w1, tau') */
    PSD_DS_REFLECTOR_SMALL = 8,  /* psd_reflector_small: (n, x0, x1, x2), n = 3, anything else runs n = 2
                                                                               -> (beta, v1, v2, tau), v2 = 0 for n = 2 */
    PSD_DS_H2_LARFG = 9,         /* psd_h2_larfg:        (alpha, xnorm)       -> (tau, beta, mult) */
    PSD_DS_ZH2_LARFG = 10,       /* psd_zh2_larfg:       (alpha, xnorm), alpha complex -> (tau, beta, mult), tau and mult complex */
    PSD_DS_GIVENS = 11,          /* psd_givens:          (f, g)               -> (cs, sn, r) */
    PSD_DS_ZGIVENS = 12,         /* psd_zgivens:         (f, g) complex       -> (cs, sn, r), sn and r complex */
    PSD_DS_ZGIVENS_LEAN = 13,    /* psd_zgivens_lean:    as PSD_DS_ZGIVENS */
    PSD_DS_C3_SCALE = 14,        /* (m, x, e, bz, bin), e an integer in [-4096, 4096]
                                    -> (psd_c3_expo(m), psd_c3_ldexp(x, e), psd_c3_beta(bz, bin, e)) */
    PSD_DS_NOPS = 15
} psd_diag_scalar_op;
int psd_diag_scalar(psd_ctx* ctx, int op, int ncases, const double* in, double* out, int* info);

/* ---- eigvecs(ps, select; shifted) by periodic back-substitution — vectors.jl:25-138 without the reordering ----------
 * The selected right eigenvectors of the product and of its circular shifts, from a periodic Schur decomposition, by
 * the periodic form of LAPACK's xTREVC: the triangular factors are solved bottom up (a cyclic recurrence round the period
 * per row block; the updates from the rows below are matrix-core products over panels of columns), then V_l = Z_l X_l on
 * the matrix cores.  The factors are not modified.  Result: A_l v_l = mu v_{l+1} (left orientation; right:
 * A_l v_{l+1} = mu v_l), mu = lambda^(1/p) the principal root of the caller's eigenvalue, ||V_1(:, j)||_2 = 1, the
 * largest-modulus entry of V_1(:, j) real and positive (lowest row on a tie), the same factor applied to every V_l(:, j);
 * for a conjugate pair of a real decomposition the second column is the conjugate of the first.
 *
 * T, Z: p pointers to n x n matrices, the user order of the decomposition (T[schurindex-1] the quasi-triangular factor),
 * any schurindex, orient 'L' or 'R'.  Eigenvalues: wr / wi (Float64, psd_d_*) or alpha / beta / ascale (ComplexF64,
 * psd_z_*: alpha[k] / beta[k] * 2^ascale[k], ascale may be NULL) — the P.values the decomposition reports.  S: NULL or
 * the signature (a signed S: PSD_INFO_NOTIMPL).  select: nsel = n flags, completed to whole conjugate pairs in place
 * (vectors.jl:42-62).  Columns come in the order of the selected eigenvalues from top to bottom.  shifted: V holds p
 * matrices (V_1 .. V_p), else one (V_1, bit-identical to V_1 of the shifted call).  V: p (or 1) pointers to n x maxvec
 * complex interleaved buffers, column-major, ld n; V = NULL: a size query (select completed, stats->nvec set, nothing
 * computed).  An eigenvalue zero (mu = 0) gives a column of NaNs (the reference's formula divides by mu as well) and is
 * counted in stats->nzero.  Near-equal eigenvalues: a pivot below max(eps, tiny) (relative) is replaced by it
 * (stats->nperturbed), so repeated eigenvalues return finite vectors.
 * info: 0; -1 ctx NULL; -2 n < 1; -3 p < 1; -4 T NULL; -5 Z NULL (no Schur vectors, vectors.jl:30-32); -6 eigenvalues
 * NULL; -7 orient; -8 schurindex not in 1..p; -9 select NULL or nsel != n (vectors.jl:34-36); -10 maxvec below the
 * number of columns; PSD_INFO_NOTIMPL signed S; PSD_INFO_RUNTIME + k. */
typedef struct psd_evec_stats {
    int32_t nvec;           /* columns returned (conjugate partners included)                                  */
    int32_t nperturbed;     /* pivots replaced by smin (near-equal eigenvalues)                                */
    int32_t nrescaled;      /* columns scaled by a power of two against overflow                               */
    int32_t nzero;          /* zero-eigenvalue columns (NaN)                                                   */
    double ms_solve;        /* back-substitution: updates and cyclic solves (device events)                   */
    double ms_backtransform;/* V_l = Z_l X_l and the normalisation (device events)                            */
    double ms_kernels;      /* the two together                                                               */
} psd_evec_stats;

int psd_d_eigvecs(psd_ctx* ctx, int n, int p, double* const* T, double* const* Z, const double* wr, const double* wi,
                  const uint8_t* S, char orient, int schurindex, uint8_t* select, int nsel, int shifted,
                  double* const* V, int maxvec, psd_evec_stats* stats, int* info);
int psd_z_eigvecs(psd_ctx* ctx, int n, int p, double* const* T, double* const* Z, const double* alpha,
                  const double* beta, const int32_t* ascale, const uint8_t* S, char orient, int schurindex,
                  uint8_t* select, int nsel, int shifted, double* const* V, int maxvec, psd_evec_stats* stats,
                  int* info);
/* Device-resident variants: dT, dZ device [p][n][n] blocks as psd_?_pschur_dev leaves them (user order), dV a device
 * block of (shifted ? p : 1) matrices n x nvec (complex interleaved, column-major, ld n; block l at 2 l n nvec doubles,
 * nvec = stats->nvec of a size query with dV = NULL).  Eigenvalues, S and select are host arrays. */
int psd_d_eigvecs_dev(psd_ctx* ctx, int n, int p, const double* dT, const double* dZ, const double* wr,
                      const double* wi, const uint8_t* S, char orient, int schurindex, uint8_t* select, int nsel,
                      int shifted, double* dV, int maxvec, psd_evec_stats* stats, int* info);
int psd_z_eigvecs_dev(psd_ctx* ctx, int n, int p, const double* dT, const double* dZ, const double* alpha,
                      const double* beta, const int32_t* ascale, const uint8_t* S, char orient, int schurindex,
                      uint8_t* select, int nsel, int shifted, double* dV, int maxvec, psd_evec_stats* stats,
                      int* info);

/* ---- geigvecs: eigenvectors of signed and singular periodic products (the periodic form of xTGEVC) --------------------
 * The selected right eigenvectors of a (generalized) periodic Schur decomposition with signature S, zero and infinite
 * eigenvalues included, by the back-substitution of psd_?_eigvecs with homogeneous recurrences.  For every column j the
 * vectors v_1 .. v_p (V_l(:, j)) and complex scalars a_1 .. a_p (a[l + p j]) satisfy, l + 1 cyclic,
 *     orient 'L':  S[l] true: A_l v_l = a_l v_{l+1};    S[l] false: A_l v_{l+1} = a_l v_l
 *     orient 'R':  S[l] true: A_l v_{l+1} = a_l v_l;    S[l] false: A_l v_l = a_l v_{l+1}
 * with A_l the factors the decomposition represents.  a_l = T_l(k, k), the diagonal at the eigenvalue's own row k (so a
 * zero a_l is a zero eigenvalue if S[l], an infinite one if not; nothing divides by the eigenvalue).  A conjugate pair
 * of a real decomposition (2x2 block at rows k, k+1): a_l = sqrt|det B_l|, times e^(+-i arg lambda_k) at schurindex (sign
 * from S there), where
 * B_l is the factors' 2x2 block and lambda_k the member with positive imaginary part; the partner column and its scalars
 * are the conjugates.  For finite non-zero eigenvalues the product of a_l^(+-1) (sign from S) is lambda_k.
 * Normalisation, select completion, shifted and V as psd_?_eigvecs.  A cyclic pivot below
 * smin = max(eps max(|A|, |C|), tiny) is replaced by smin (stats->nperturbed): the vectors are always finite.
 *
 * T, Z: p pointers to n x n matrices in user order (T[schurindex-1] quasi-triangular), orient 'L' or 'R', any
 * schurindex.  S: NULL (all true) or p flags.  No eigenvalue arguments: everything comes from T.  a: host, p x maxvec
 * complex interleaved, column-major with ld p, may be NULL.  V = NULL: a size query.  stats: psd_evec_stats, with nzero
 * the number of columns whose eigenvalue is zero or infinite (a zero a_l; these columns are computed).
 * info: 0; -1 ctx NULL; -2 n < 1; -3 p < 1; -4 T NULL; -5 Z NULL; -7 orient; -8 schurindex not in 1..p; -9 select
 * NULL or nsel != n; -13 maxvec below the number of columns; PSD_INFO_RUNTIME + k. */
int psd_d_geigvecs(psd_ctx* ctx, int n, int p, double* const* T, double* const* Z, const uint8_t* S, char orient,
                   int schurindex, uint8_t* select, int nsel, int shifted, double* const* V, int maxvec, double* a,
                   psd_evec_stats* stats, int* info);
int psd_z_geigvecs(psd_ctx* ctx, int n, int p, double* const* T, double* const* Z, const uint8_t* S, char orient,
                   int schurindex, uint8_t* select, int nsel, int shifted, double* const* V, int maxvec, double* a,
                   psd_evec_stats* stats, int* info);
/* Device-resident variants: dT, dZ, dV as psd_?_eigvecs_dev; S, select and a are host arrays. */
int psd_d_geigvecs_dev(psd_ctx* ctx, int n, int p, const double* dT, const double* dZ, const uint8_t* S, char orient,
                       int schurindex, uint8_t* select, int nsel, int shifted, double* dV, int maxvec, double* a,
                       psd_evec_stats* stats, int* info);
int psd_z_geigvecs_dev(psd_ctx* ctx, int n, int p, const double* dT, const double* dZ, const uint8_t* S, char orient,
                       int schurindex, uint8_t* select, int nsel, int shifted, double* dV, int maxvec, double* a,
                       psd_evec_stats* stats, int* info);

/* ---- eigvecs_batch: eigenvectors of many small periodic Schur forms in one call -------------------------------------
 * psd_?_eigvecs (back-substitution) for nb decompositions of one shape (n, p), as psd_d_pschur_batch leaves them:
 * Float64, all-true signature, one orient and schurindex for the whole batch.  Per problem the result contract is that
 * of psd_d_eigvecs: select completed to whole conjugate pairs, columns top to bottom, ||V_1(:, j)|| = 1 with the
 * largest-modulus entry real and positive, the partner of a pair the exact conjugate, a zero eigenvalue a NaN column
 * (counted), small pivots replaced by smin (counted), columns past 2^500 rescaled by a power of two (counted).  A
 * problem's vectors do not depend on its place in the batch or on the grouping (bit for bit).  Up to order 128 the
 * whole back-substitution of a group is one launch (several columns per wavefront for p <= 32) and the call makes the
 * same number of launches whatever nb and n are (stats->nlaunch); above, psd_d_eigvecs_dev runs problem by problem on
 * the slices of the batch buffers.  A batch whose workspace exceeds the free device memory is worked through in groups
 * (PSD_BATCH_GROUP in the environment lowers the group size).
 *
 * T, Z: nb * p pointers to n x n matrices (problem-major, user order).  wr, wi: host [nb][n].  select: host [nb][n],
 * completed in place.  A problem whose row of select is all false costs nothing and gets nvec = 0: that is how a caller
 * skips the problems whose psd_d_pschur_batch info was non-zero.  V: nb * nmat pointers (nmat = shifted ? p : 1) to
 * n x maxvec complex interleaved column-major blocks; the columns at and beyond nvec[q] are written as zeros.  V = NULL:
 * a size query (select completed, nvec filled, nothing computed).  nvec: host [nb], out.  pcnt: host [nb][3] or NULL:
 * perturbed pivots, rescaled columns, zero eigenvalues per problem.
 * info: 0; -1 ctx NULL; -2 n < 1; -3 p < 1; -4 T NULL; -5 Z NULL; -6 wr or wi NULL; -7 orient; -8 schurindex not in
 * 1..p; -9 select NULL; -10 maxvec below the largest nvec; -11 nb < 0; -12 nvec NULL; PSD_INFO_NOTIMPL on a
 * period-sharded context; PSD_INFO_RUNTIME + k.  nb == 0 returns 0 and touches nothing. */
typedef struct psd_bevec_stats {
    int32_t nb;             /* problems of the call                                                            */
    int32_t nvec_total;     /* columns returned over all problems                                              */
    int32_t nperturbed;     /* as psd_evec_stats, summed over the batch                                        */
    int32_t nrescaled;
    int32_t nzero;
    int32_t nlaunch;        /* kernel launches of the call                                                     */
    int32_t ngroups;        /* groups the batch was worked through in                                          */
    int32_t reserved;
    double ms_solve;        /* device events, summed over the groups                                           */
    double ms_backtransform;
    double ms_kernels;
} psd_bevec_stats;

int psd_d_eigvecs_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, double* const* Z, const double* wr,
                        const double* wi, char orient, int schurindex, uint8_t* select, int shifted, double* const* V,
                        int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info);
/* Device-resident variant: dT, dZ device [nb][p][n][n] column-major blocks in user order (what psd_d_pschur_batch_dev
 * leaves), dV a device block [nb][nmat][maxvec][n] of interleaved complex values (each block column-major n x maxvec).
 * wr, wi, select, nvec and pcnt are host arrays.  One kernel and one read-back define the 2x2 row blocks. */
int psd_d_eigvecs_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dT, const double* dZ, const double* wr,
                            const double* wi, char orient, int schurindex, uint8_t* select, int shifted, double* dV,
                            int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info);

/* ---- zeigvecs_batch: eigenvectors of many small ComplexF64 periodic Schur forms in one call -------------------------
 * psd_z_eigvecs (back-substitution) for nb decompositions of one shape (n, p), as psd_z_pschur_batch leaves them:
 * ComplexF64, all-true signature, one orient and schurindex for the whole batch; the conventions of psd_d_eigvecs_batch
 * with interleaved complex matrices.  Per problem the result contract is that of psd_z_eigvecs: one column per selected
 * row, top to bottom, ||V_1(:, j)|| = 1 with the largest-modulus entry real and positive, a zero eigenvalue a NaN column
 * (counted), small pivots replaced by smin (counted), columns past 2^500 rescaled by a power of two (counted).  A
 * problem's vectors do not depend on its place in the batch or on the grouping (bit for bit).  Up to order 128 the whole
 * back-substitution of a group is one launch and the call makes four launches with shifted and p > 1, three otherwise,
 * none when nothing is selected (stats->nlaunch); nothing is read back before the solve, a complex form being triangular
 * in every factor.  Above, psd_z_eigvecs_dev's driver runs problem by problem on the slices of the batch buffers.
 * PSD_BATCH_GROUP acts as for the real entry.
 *
 * T, Z: nb * p pointers to n x n interleaved complex matrices (problem-major, user order).  alpha: host [nb][n] complex
 * pairs, beta: host [nb][n], ascale: host [nb][n] or NULL (zeros) — the eigenvalues alpha / beta * 2^ascale, converted
 * as psd_z_eigvecs converts them.  select: host [nb][n], used as given (there are no conjugate pairs to complete);
 * nvec[q] is the count of its row q, and a problem whose row is all false costs nothing.  V, maxvec, nvec, pcnt, stats
 * and V = NULL (a size query) as for psd_d_eigvecs_batch.
 * info: 0; -1 ctx NULL; -2 n < 1; -3 p < 1; -4 T NULL; -5 Z NULL; -6 alpha or beta NULL; -7 orient; -8 schurindex not in
 * 1..p; -9 select NULL; -10 maxvec below the largest nvec; -11 nb < 0; -12 nvec NULL; PSD_INFO_NOTIMPL on a
 * period-sharded context; PSD_INFO_RUNTIME + k.  nb == 0 returns 0 and touches nothing. */
int psd_z_eigvecs_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, double* const* Z, const double* alpha,
                        const double* beta, const int32_t* ascale, char orient, int schurindex, const uint8_t* select,
                        int shifted, double* const* V, int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats,
                        int* info);
/* Device-resident variant: dT, dZ device [nb][p][n][n] interleaved column-major blocks in user order (what
 * psd_z_pschur_batch_dev leaves), dV a device block [nb][nmat][maxvec][n] of interleaved complex values.  alpha, beta,
 * ascale, select, nvec and pcnt are host arrays. */
int psd_z_eigvecs_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dT, const double* dZ, const double* alpha,
                            const double* beta, const int32_t* ascale, char orient, int schurindex,
                            const uint8_t* select, int shifted, double* dV, int maxvec, int* nvec, int32_t* pcnt,
                            psd_bevec_stats* stats, int* info);

/* ---- leigvecs_batch: LEFT eigenvectors of many small periodic Schur forms in one call ------------------------------
 * The side = 'L' of xTREVC in periodic form, for the decompositions psd_d_eigvecs_batch / psd_z_eigvecs_batch take:
 * W_1 .. W_p (or W_1 alone without shifted) with, mu_j being the principal p-th root of eigenvalue j exactly as the right
 * entries take it and l + 1 cyclic,
 *     orient 'L' (right vectors: A_l v_l = mu v_{l+1}):   w_{l+1}^H A_l = mu w_l^H
 *     orient 'R' (right vectors: A_l v_{l+1} = mu v_l):   w_l^H A_l = mu w_{l+1}^H
 * so that w_l is a left and v_l a right eigenvector of the same cyclic shift of the product, and w_l^H v_l is the same
 * number for every l.  Column j of W belongs to the eigenvalue of column j of V.  Everything else is the right entry's
 * contract, word for word: select completed to conjugate pairs (real), columns top to bottom, ||W_1(:, j)|| = 1 with
 * the largest-modulus entry real and positive and the same factor on every W_l(:, j), the partner of a pair the exact
 * conjugate, a zero eigenvalue a NaN column (counted), small pivots replaced by smin (counted), columns past 2^500
 * rescaled by a power of two (counted), the inputs not modified, the padding columns written as zeros, V = NULL a size
 * query, a problem's bits independent of its place in the batch and of the grouping.
 *
 * No second solver: the adjoints of the left relations are a periodic problem of the opposite orientation whose Schur
 * form is T'_l = J T_l^H J, Z'_l = Z_l J (J the reversal permutation), eigenvalues conjugated and reversed, schurindex
 * unchanged.  One launch writes T' and Z' of a group into workspace, the launches of the right entry run on them with
 * the conjugates of the caller's roots, and one launch turns the columns into the caller's order: stats->nlaunch is the
 * right call's count plus two, whatever nb and n are.  Above order 128 the single driver runs on the flipped slices.
 * Arguments, info codes and stats: those of psd_d_eigvecs_batch[_dev] and psd_z_eigvecs_batch[_dev] respectively. */
int psd_d_leigvecs_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, double* const* Z, const double* wr,
                         const double* wi, char orient, int schurindex, uint8_t* select, int shifted, double* const* V,
                         int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info);
int psd_d_leigvecs_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dT, const double* dZ, const double* wr,
                             const double* wi, char orient, int schurindex, uint8_t* select, int shifted, double* dV,
                             int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info);
int psd_z_leigvecs_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, double* const* Z, const double* alpha,
                         const double* beta, const int32_t* ascale, char orient, int schurindex, const uint8_t* select,
                         int shifted, double* const* V, int maxvec, int* nvec, int32_t* pcnt, psd_bevec_stats* stats,
                         int* info);
int psd_z_leigvecs_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dT, const double* dZ, const double* alpha,
                             const double* beta, const int32_t* ascale, char orient, int schurindex,
                             const uint8_t* select, int shifted, double* dV, int maxvec, int* nvec, int32_t* pcnt,
                             psd_bevec_stats* stats, int* info);

/* ---- eigcond_batch: reciprocal condition numbers of the eigenvalues, per factor -------------------------------------
 * The S of xTRSNA in periodic form (for p = 1 exactly that), from the right and left vectors of EVERY factor as the
 * eigenvector entries write them with shifted (nmat = p; complex interleaved for both families):
 *     orient 'L':   s[l, j] = |w_l^H v_l| / (||w_{l+1}||_2 ||v_l||_2)
 *     orient 'R':   s[l, j] = |w_l^H v_l| / (||w_l||_2 ||v_{l+1}||_2)
 * To first order d lambda_j / lambda_j = (1 / mu_j) sum_l w_{l+1}^H dA_l v_l / (w_1^H v_1) for 'L' (for 'R' the sum runs
 * over w_l^H dA_l v_{l+1}), hence |d lambda_j / lambda_j| <= sum_l ||dA_l||_2 / (|mu_j| s[l, j]).  A NaN column (a zero
 * eigenvalue) gives NaN.  One wavefront per (problem, column), every sum in a fixed order, no atomics: s does not depend
 * on the batch or the grouping, bit for bit.
 *
 * V, W: nb * p pointers to n x maxvec complex interleaved column-major blocks (problem-major).  nvec: host [nb], the
 * columns of every problem.  s: host [nb][maxvec][p], out; the entries of the columns at and beyond nvec[q] are 0.
 * info: 0; -1 ctx NULL; -2 n < 1; -3 p < 1; -4 V NULL; -5 W NULL; -7 orient; -10 maxvec < 1 or an nvec[q] outside
 * 0..maxvec; -11 nb < 0; -12 nvec NULL; -13 s NULL; PSD_INFO_NOTIMPL on a period-sharded context; PSD_INFO_RUNTIME + k.
 * nb == 0 returns 0 and touches nothing. */
int psd_eigcond_batch(psd_ctx* ctx, int nb, int n, int p, double* const* V, double* const* W, char orient, int maxvec,
                      const int* nvec, double* s, int* info);
/* Device-resident variant: dV, dW device blocks [nb][p][maxvec][n] of interleaved complex values, as
 * psd_?_eigvecs_batch_dev and psd_?_leigvecs_batch_dev leave them with shifted.  nvec and s are host arrays. */
int psd_eigcond_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dV, const double* dW, char orient,
                          int maxvec, const int* nvec, double* s, int* info);

/* ---- zgeigvecs_batch: eigenvectors of many small signed ComplexF64 periodic Schur forms in one call ----------------
 * psd_z_geigvecs (homogeneous back-substitution, the periodic form of xTGEVC) for nb generalized decompositions of one
 * shape (n, p) and ONE signature, as psd_z_gpschur_batch / psd_z_gordschur_batch leave them: ComplexF64, one orient and
 * schurindex (any in 1..p) for the whole batch; the conventions of psd_z_eigvecs_batch.  Per problem the result contract
 * is that of psd_z_geigvecs: one column per selected row, top to bottom, the scalars a_l = T_l(k, k) at the column's own
 * row k, the relations of the signature table above, ||V_1(:, j)|| = 1 with the largest-modulus entry real and positive;
 * a zero or infinite eigenvalue (a zero a_l) gives a valid finite column (counted), pivots below smin are replaced
 * (counted), columns past 2^500 are rescaled by a power of two (counted).  A problem's vectors do not depend on its place
 * in the batch or on the grouping (bit for bit).  A NULL or all-true S runs this path too, not psd_z_eigvecs_batch: the
 * contract differs on zero eigenvalues and on a.  Up to order 128 the whole back-substitution of a group is one launch
 * (psd_zgbev_solve: several columns per wavefront for p <= 32, the scalars read from the factors on the device) and the
 * call makes four launches with shifted and p > 1, three otherwise, whatever nb and n are; the device entry makes one
 * more, the gather of the diagonals, when a is not NULL; none when nothing is selected (stats->nlaunch).  Above,
 * psd_z_geigvecs_dev's driver runs problem by problem on the slices of the batch buffers.  PSD_BATCH_GROUP acts as for
 * psd_d_eigvecs_batch.
 *
 * T, Z: nb * p pointers to n x n interleaved complex matrices (problem-major, user order).  S: host [p] flags in user
 * order, or NULL (all true).  select: host [nb][n], used as given; nvec[q] is the count of its row q, and a problem whose
 * row is all false costs nothing.  V, maxvec, nvec and V = NULL (a size query) as for psd_z_eigvecs_batch.  a: host
 * [nb][maxvec][p] complex interleaved — per problem column-major p x maxvec with ld p, as psd_z_geigvecs lays it out, the
 * columns at and beyond nvec[q] zero — or NULL.  pcnt: host [nb][3] or NULL: perturbed pivots, rescaled columns, columns
 * with a zero or infinite eigenvalue per problem; stats->nzero is the sum of the third.
 * info: 0; -1 ctx NULL; -2 n < 1; -3 p < 1; -4 T NULL; -5 Z NULL; (-6 is not used: there are no eigenvalue arguments);
 * -7 orient; -8 schurindex not in 1..p; -9 select NULL; -10 maxvec below the largest nvec; -11 nb < 0; -12 nvec NULL;
 * PSD_INFO_NOTIMPL on a period-sharded context; PSD_INFO_RUNTIME + k.  nb == 0 returns 0 and touches nothing. */
int psd_z_geigvecs_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, double* const* Z, const uint8_t* S,
                         char orient, int schurindex, const uint8_t* select, int shifted, double* const* V, int maxvec,
                         double* a, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info);
/* Device-resident variant: dT, dZ device [nb][p][n][n] interleaved column-major blocks in user order (what
 * psd_z_gpschur_batch_dev / psd_z_gordschur_batch_dev leave), dV a device block [nb][nmat][maxvec][n] of interleaved
 * complex values.  S, select, a, nvec and pcnt are host arrays; a costs one gather kernel and one read-back for the whole
 * batch, skipped when it is NULL. */
int psd_z_geigvecs_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dT, const double* dZ, const uint8_t* S,
                             char orient, int schurindex, const uint8_t* select, int shifted, double* dV, int maxvec,
                             double* a, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info);

/* ---- dgeigvecs_batch: eigenvectors of many small signed Float64 periodic Schur forms in one call -------------------
 * psd_d_geigvecs for nb generalized decompositions of one shape (n, p) and ONE signature, as psd_d_gpschur_batch /
 * psd_d_gordschur_batch leave them: Float64, one orient and schurindex (any in 1..p, the quasi-triangular factor) for the
 * whole batch; the conventions of psd_z_geigvecs_batch, with real T and Z.  Per problem the result contract is that of
 * psd_d_geigvecs: columns top to bottom, a conjugate pair two columns (the partner and its scalars the exact
 * conjugates); a_l = T_l(k, k) on a 1x1 row, sqrt|det B_l| on a pair, times e^(+-i arg lambda) at schurindex;
 * ||V_1(:, j)|| = 1 with the largest-modulus entry real and positive; a zero or infinite eigenvalue gives a valid finite
 * column (counted, never NaN), pivots below smin are replaced (counted), columns past 2^500 are rescaled by a power of
 * two (counted).  A problem's vectors and scalars do not depend on its place in the batch or on the grouping (bit for
 * bit).  A NULL or all-true S runs this path too, not psd_d_eigvecs_batch.  Up to order 128 the whole back-substitution
 * of a group is one launch (psd_gbev_solve: several columns per wavefront for p <= 32, 1x1 and 2x2 row blocks side by
 * side, the scalars uploaded with the tables) and a group makes four launches with shifted and p > 1, three otherwise,
 * whatever nb and n are; the device entry makes one more for the whole call, the gather of the diagonals, sub- and
 * super-diagonals (it defines the row blocks and the scalars); none when nothing is selected (stats->nlaunch).  Above,
 * psd_d_geigvecs_dev's driver runs problem by problem on the slices of the batch buffers.  PSD_BATCH_GROUP acts as for
 * psd_d_eigvecs_batch.
 *
 * T, Z: nb * p pointers to n x n column-major real matrices (problem-major, user order).  S: host [p] flags in user
 * order, or NULL (all true).  select: host [nb][n], completed in place to whole conjugate pairs per problem, as
 * psd_d_eigvecs_batch does; nvec[q] counts the completed row q, and a problem whose row is all false costs nothing.
 * V: nb * nmat pointers to n x maxvec interleaved complex matrices, laid out as for psd_d_eigvecs_batch (the columns at
 * and beyond nvec[q] zero); V = NULL is a size query (select completed, nvec filled).  a: host [nb][maxvec][p] complex
 * interleaved — per problem column-major p x maxvec with ld p, as psd_d_geigvecs lays it out, the columns at and beyond
 * nvec[q] zero — or NULL.  pcnt: host [nb][3] or NULL: perturbed pivots, rescaled columns, columns with a zero or
 * infinite eigenvalue per problem; stats->nzero is the sum of the third.
 * info: as psd_z_geigvecs_batch (-6 not used, -10 maxvec below the largest nvec, -11 nb < 0, -12 nvec NULL,
 * PSD_INFO_NOTIMPL on a period-sharded context).  nb == 0 returns 0 and touches nothing. */
int psd_d_geigvecs_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, double* const* Z, const uint8_t* S,
                         char orient, int schurindex, uint8_t* select, int shifted, double* const* V, int maxvec,
                         double* a, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info);
/* Device-resident variant: dT, dZ device [nb][p][n][n] column-major blocks in user order (what psd_d_gpschur_batch_dev /
 * psd_d_gordschur_batch_dev leave), dV a device block [nb][nmat][maxvec][n] of interleaved complex values.  S, select, a,
 * nvec and pcnt are host arrays.  One gather kernel and one read-back for the whole batch define the row blocks and the
 * scalars (no separate sub-diagonal kernel). */
int psd_d_geigvecs_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dT, const double* dZ, const uint8_t* S,
                             char orient, int schurindex, uint8_t* select, int shifted, double* dV, int maxvec,
                             double* a, int* nvec, int32_t* pcnt, psd_bevec_stats* stats, int* info);

/* ---- ordschur_batch: reorder many small periodic Schur forms in one call ------------------------------------------
 * psd_d_ordschur (rordschur.jl:3-132) for nb decompositions of one shape (n, p), as psd_d_pschur_batch leaves them:
 * Float64, all-true signature, one orient and schurindex (1 or p) for the whole batch.  Per problem the result contract
 * is that of psd_d_ordschur: the selected eigenvalues lead, selecting one member of a conjugate pair takes its partner
 * along, the order inside both groups is kept.  Up to order 128 one wavefront carries one problem through its whole
 * reordering and a group is ONE launch of the swap kernel whatever nb is (stats->nlaunch_step counts them); above, or
 * for a period whose narrowest window does not fit the LDS, the single-problem driver runs problem by problem on the
 * slices of the batch buffers.  A problem's result does not depend on its place in the batch or on the grouping (bit
 * for bit).  A batch that does not fit the free device memory is worked through in groups (PSD_BATCH_GROUP in the
 * environment lowers the group size; PSD_BORD_W narrows the window, PSD_BORD_NMAX lowers the order limit).
 *
 * T, Z: nb * p pointers to n x n matrices (problem-major, user order), reordered in place; Z may be NULL when !wantZ.
 * select: host [nb][n].  wr, wi: host [nb][n], the eigenvalues in their new order; the rows of a failed problem are not
 * written.  infos: host [nb] or NULL, per problem 0, 3000 (singular periodic Sylvester system) or 2000 + row (swap
 * rejected: ill-conditioned), the codes of psd_d_ordschur; a rejected swap ends its problem alone and leaves it a
 * consistent decomposition (the swaps made so far).  nswaps: host [nb] or NULL, the adjacent swaps of every problem.
 * stats: nsweeps = swaps and nwindows = windows over all problems, window = W (at most 25 rows: the longest window whose
 * transform lists cannot overflow), nlaunch_step = launches of the swap
 * kernel (one per group), ms_iter = ms_total = device time of the kernels, ms_copy (host entry) the copies.
 * Returns the first non-zero per-problem code, or a call-wide one: -1 ctx NULL; -2 n < 1; -3 p < 1; -4 T NULL;
 * -5 Z NULL with wantZ; -6 orient; -7 schurindex strictly inside the period; -8 select NULL; -9 wr or wi NULL;
 * -11 nb < 0; PSD_INFO_NOTIMPL on a period-sharded context; PSD_INFO_RUNTIME + k.  nb == 0 returns 0 and touches
 * nothing. */
int psd_d_ordschur_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, double* const* Z, char orient,
                         int schurindex, const uint8_t* select, int wantZ, double* wr, double* wi, int* infos,
                         int* nswaps, psd_stats* stats, int* info);
/* Device-resident variant: dT, dZ device [nb][p][n][n] column-major blocks in user order (what psd_d_pschur_batch_dev
 * leaves), reordered in place; select, wr, wi, infos and nswaps are host arrays.  The blocks are brought to the order
 * the swap kernels work on and back on the device: nothing for 'R' with schurindex 1, block reversals in place for 'L'
 * with schurindex p, a group of problems at a time through a temporary for the two shifted alignments (a group that
 * fits the free device memory, as above). */
int psd_d_ordschur_batch_dev(psd_ctx* ctx, int nb, int n, int p, void* dT, void* dZ, char orient, int schurindex,
                             const uint8_t* select, int wantZ, double* wr, double* wi, int* infos, int* nswaps,
                             psd_stats* stats, int* info);

/* ---- zordschur_batch: reorder many small ComplexF64 periodic Schur forms in one call -------------------------------
 * psd_z_ordschur (ordschur.jl:11-73) for nb decompositions of one shape (n, p), as psd_z_pschur_batch leaves them:
 * ComplexF64, all-true signature, one orient and schurindex (1 or p) for the whole batch; the conventions of
 * psd_d_ordschur_batch with interleaved complex matrices.  Up to order 128 one wavefront carries one problem through its
 * whole reordering — the step and apply bodies of the single driver's serial form, the same windows and the same
 * arithmetic — and a group is ONE launch of the swap kernel (psd_zbord) whatever nb is; above, or for a period whose
 * narrowest window does not fit the LDS, psd_z_ordschur's driver runs problem by problem on the slices of the batch
 * buffers.  A problem's result does not depend on its place in the batch or on the grouping (bit for bit).
 * PSD_BATCH_GROUP, PSD_BORD_W (here from 4) and PSD_BORD_NMAX act as for the real entry.
 *
 * T, Z: nb * p pointers to n x n interleaved complex matrices (problem-major, user order), reordered in place; Z may be
 * NULL when !wantZ.  select: host [nb][n], used as given (there are no conjugate pairs to complete).  alpha: host
 * [nb][n] complex pairs, beta, ascale: host [nb][n] — the eigenvalues alpha / beta * 2^ascale in their new order; the
 * rows of a failed problem are not written.  infos, nswaps, stats and the per-problem codes (0, 3000, 2000 + row) as
 * for psd_d_ordschur_batch; stats->window = W (at most 32).
 * Returns the first non-zero per-problem code, or a call-wide one: -1 ctx NULL; -2 n < 1; -3 p < 1; -4 T NULL;
 * -5 Z NULL with wantZ; -6 orient; -7 schurindex strictly inside the period; -8 select NULL; -9 alpha, beta or ascale
 * NULL; -11 nb < 0; PSD_INFO_NOTIMPL on a period-sharded context; PSD_INFO_RUNTIME + k.  nb == 0 returns 0 and touches
 * nothing. */
int psd_z_ordschur_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, double* const* Z, char orient,
                         int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta, int32_t* ascale,
                         int* infos, int* nswaps, psd_stats* stats, int* info);
/* Device-resident variant: dT, dZ device [nb][p][n][n] column-major interleaved complex blocks in user order (what
 * psd_z_pschur_batch_dev leaves), reordered in place; the other arrays are host arrays.  The blocks are brought to the
 * internal order and back on the device, as psd_d_ordschur_batch_dev does. */
int psd_z_ordschur_batch_dev(psd_ctx* ctx, int nb, int n, int p, void* dT, void* dZ, char orient, int schurindex,
                             const uint8_t* select, int wantZ, double* alpha, double* beta, int32_t* ascale, int* infos,
                             int* nswaps, psd_stats* stats, int* info);

/* ---- zgordschur_batch: reorder many small signed ComplexF64 periodic Schur forms in one call -----------------------
 * psd_z_gordschur (ordschur.jl:11-96, sylswap.jl:638-764) for nb generalized decompositions of one shape (n, p) and ONE
 * signature, as psd_z_gpschur_batch leaves them: ComplexF64, one orient and schurindex (1 or p) for the whole batch; the
 * conventions of psd_z_ordschur_batch.  S: host [p] flags in user order, or NULL (all true).  Up to order 128 one
 * wavefront carries one problem through its whole reordering — the step and apply bodies of psd_z_gordschur's serial
 * form, the same windows and the same arithmetic — and a group is ONE launch of the swap kernel (psd_zgbord) whatever
 * nb is; above, or for a period whose narrowest window does not fit the LDS, psd_z_gordschur's driver runs problem by
 * problem on the slices of the batch buffers.  A problem's result does not depend on its place in the batch or on the
 * grouping (bit for bit).  A NULL or all-true S is the call of psd_z_ordschur_batch (the same bits).  PSD_BATCH_GROUP,
 * PSD_BORD_W (here from 4) and PSD_BORD_NMAX act as for psd_z_ordschur_batch.
 *
 * T, Z, select, alpha, beta, ascale, infos, nswaps, stats and the per-problem codes (0, 3000, 2000 + row) as for
 * psd_z_ordschur_batch; stats->window = W (at most 32).
 * Returns the first non-zero per-problem code, or a call-wide one: -1 ctx NULL; -2 n < 1; -3 p < 1; -4 T NULL;
 * -5 Z NULL with wantZ; -6 orient; -7 schurindex strictly inside the period; -8 select NULL; -9 alpha, beta or ascale
 * NULL; -10 the entry of S that lands first in working order (that of the factor at schurindex) is false; -11 nb < 0;
 * PSD_INFO_NOTIMPL on a period-sharded context; PSD_INFO_RUNTIME + k.  nb == 0 returns 0 and touches nothing. */
int psd_z_gordschur_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, double* const* Z, const uint8_t* S,
                          char orient, int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta,
                          int32_t* ascale, int* infos, int* nswaps, psd_stats* stats, int* info);
/* Device-resident variant: dT, dZ device [nb][p][n][n] column-major interleaved complex blocks in user order (what
 * psd_z_gpschur_batch_dev leaves), reordered in place; S and the other arrays are host arrays.  The blocks are brought
 * to the internal order and back on the device, as psd_d_ordschur_batch_dev does. */
int psd_z_gordschur_batch_dev(psd_ctx* ctx, int nb, int n, int p, void* dT, void* dZ, const uint8_t* S, char orient,
                              int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta,
                              int32_t* ascale, int* infos, int* nswaps, psd_stats* stats, int* info);

/* ---- dgordschur_batch: reorder many small signed Float64 periodic Schur forms in one call --------------------------
 * ordschur!(P::GeneralizedPeriodicSchur{Float64}, select) (rordschur.jl:3-132 with the signed block swaps of
 * sylswap.jl:197-538) for nb real generalized decompositions of one shape (n, p) and ONE signature, as
 * psd_d_gpschur_batch leaves them: quasi-triangular T at schurindex (1 or p), orthogonal Z, one orient for the whole
 * batch; the conventions of psd_z_gordschur_batch.  S: host [p] flags in user order, or NULL (all true).  Up to order
 * 128 one wavefront carries one problem through its whole reordering — the scan, window and swap bodies of the single
 * driver and its off-window update with the sides the signature asks for — and a group is ONE launch of the swap kernel
 * (psd_gbord) whatever nb is; above, or for a period whose narrowest window does not fit the LDS, the real signed single
 * driver runs problem by problem on the slices of the batch buffers (every problem: unlike psd_d_gordschur, a problem
 * with a purely real spectrum is not promoted to the complex kernel).  A problem's result does not depend on its place
 * in the batch or on the grouping (bit for bit).  A NULL or all-true S stays on these kernels: the eigenvalues are
 * always returned in the scaled form.  PSD_BATCH_GROUP, PSD_BORD_W (from 6) and PSD_BORD_NMAX act as for
 * psd_d_ordschur_batch.
 *
 * T, Z: nb * p host matrices of n * n doubles, column-major; select: nb * n flags — one member of a conjugate pair takes
 * its partner along; alpha: nb * n complex pairs (conjugate pairs as exact conjugates), beta, ascale: nb * n; infos,
 * nswaps, stats and the per-problem codes (0, 3000, 2000 + row) as for psd_z_gordschur_batch; stats->window = W (at
 * most 25).
 * Returns the first non-zero per-problem code, or a call-wide one: -1 ctx NULL; -2 n < 1; -3 p < 1; -4 T NULL;
 * -5 Z NULL with wantZ; -6 orient; -7 schurindex strictly inside the period; -8 select NULL; -9 alpha, beta or ascale
 * NULL; -10 the entry of S that lands first in working order (that of the factor at schurindex) is false; -11 nb < 0;
 * PSD_INFO_NOTIMPL on a period-sharded context; PSD_INFO_RUNTIME + k.  nb == 0 returns 0 and touches nothing. */
int psd_d_gordschur_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, double* const* Z, const uint8_t* S,
                          char orient, int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta,
                          int32_t* ascale, int* infos, int* nswaps, psd_stats* stats, int* info);
/* Device-resident variant: dT, dZ device [nb][p][n][n] column-major blocks of doubles in user order (what
 * psd_d_gpschur_batch_dev leaves), reordered in place; S and the other arrays are host arrays.  The blocks are brought
 * to the internal order and back on the device, as psd_d_ordschur_batch_dev does. */
int psd_d_gordschur_batch_dev(psd_ctx* ctx, int nb, int n, int p, void* dT, void* dZ, const uint8_t* S, char orient,
                              int schurindex, const uint8_t* select, int wantZ, double* alpha, double* beta,
                              int32_t* ascale, int* infos, int* nswaps, psd_stats* stats, int* info);

/* ---- checkpsd_batch: verify many small periodic Schur forms in one call ---------------------------------------------
 * checkpsd(P, As; thresh, strict) (diagnostics.jl:190-263) for nb decompositions of one shape (n, p), ONE signature, one
 * orient and one schurindex, as the *_pschur_batch, *_ordschur_batch entries of every family leave them: two entries
 * per element type, the signature an argument (NULL: all true).  Up to order 64 (PSD_BCK_NMAX) a group of problems is
 * ONE launch — a workgroup per (problem, factor) forms || tril(T_l) ||_F, opnorm(A_l, 1), || Z_l Z_l' - I ||_F and
 * || Z_a T_l Z_b' - A_l ||_F on the matrix cores, W = T_l Z_b' staying in LDS — and one read-back of four numbers per
 * factor; every sum has a fixed order and there are no atomics, so up to that order a factor's numbers do not depend on
 * nb, on the problem's place in the batch or on the grouping (bit for bit).  Above it the single verifier
 * (psd_?_checkpsd_dev) runs problem by problem on the slices of the batch buffers, without that promise.  PSD_BATCH_GROUP
 * acts as for the other batch entries; PSD_BCK_NMAX in the environment at psd_create may only lower the order.
 *
 * T, Z, A: nb * p host matrices of n * n elements, column-major, problem-major, USER order (T[q * p + schurindex - 1] is
 * the quasi-triangular factor of problem q); they are only read.  S: host [p] flags in user order, or NULL.  err
 * (required), orth, tri (each may be NULL): host [nb][p], as the single entry defines them; ok (may be NULL): host [nb],
 * the reference's Bool per problem (tri <= (strict ? 0 : 10 eps n), orth <= 10 eps n, err <= thresh; a NaN fails).
 * stats (may be NULL): nfail the problems with ok == 0; nlaunch == ngroups up to order 64.  A failed check is a verdict,
 * not an error: the return value and *info are 0.
 * Returns: -1 ctx NULL; -2 nb < 0; -3 n < 1; -4 p < 1; -5 T, Z or A NULL; -8 orient; -9 schurindex not in 1..p;
 * -13 err NULL; PSD_INFO_NOTIMPL on a period-sharded context; PSD_INFO_RUNTIME + k.  nb == 0 returns 0 and touches
 * nothing. */
typedef struct psd_bcheck_stats {
    int32_t nb;        /* problems of the call */
    int32_t nfail;     /* problems whose verdict is false */
    int32_t nlaunch;   /* kernel launches (one per group up to order 64) */
    int32_t ngroups;   /* groups the batch went to the device in */
    double ms_kernels; /* device time of the kernels and their read-back */
    double ms_copy;    /* host entries: time of the uploads */
} psd_bcheck_stats;
int psd_d_checkpsd_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, double* const* Z, double* const* A,
                         const uint8_t* S, char orient, int schurindex, double thresh, int strict, double* err,
                         double* orth, double* tri, int32_t* ok, psd_bcheck_stats* stats, int* info);
int psd_z_checkpsd_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, double* const* Z, double* const* A,
                         const uint8_t* S, char orient, int schurindex, double thresh, int strict, double* err,
                         double* orth, double* tri, int32_t* ok, psd_bcheck_stats* stats, int* info);
/* Device-resident variants: dT, dZ, dA device [nb][p][n][n] column-major blocks in user order (what the
 * psd_?_*pschur_batch_dev entries leave; psd_z_: interleaved), read only; S and the outputs are host arrays. */
int psd_d_checkpsd_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dT, const double* dZ, const double* dA,
                             const uint8_t* S, char orient, int schurindex, double thresh, int strict, double* err,
                             double* orth, double* tri, int32_t* ok, psd_bcheck_stats* stats, int* info);
int psd_z_checkpsd_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dT, const double* dZ, const double* dA,
                             const uint8_t* S, char orient, int schurindex, double thresh, int strict, double* err,
                             double* orth, double* tri, int32_t* ok, psd_bcheck_stats* stats, int* info);

/* ---- psylv_batch, subcond_batch: periodic Sylvester solves and the condition of an invariant periodic subspace ------
 * nb periodic Schur forms of one shape (n, p), one orient and one schurindex, all-true signature, as the *_pschur_batch
 * and *_ordschur_batch entries leave them; problem q is split at m[q], 0 <= m[q] <= n, k = n - m[q], which must not cut a
 * 2x2 block of the quasi-triangular factor: T_l = [T11_l T12_l; 0 T22_l].  With (a(l), b(l)) = (l + 1, l) cyclically for
 * orient 'L' and (l, l + 1) for 'R' — the factors of the residual Z_a T_l Z_b' - A_l that checkpsd_batch forms — the
 * periodic Sylvester operator on p stacked m x k blocks is
 *     S(X)_l = T11_l X_b(l) - X_a(l) T22_l ,   l = 1..p.
 *
 * psd_?_psylv_batch solves S(X) = C (trans == 0) or S^H(Y) = C (trans != 0; the adjoint under the Frobenius inner product
 * over the stacked blocks).  C: nb * p blocks in user order, problem-major, each of xb elements (xb >= m[q] (n - m[q]) for
 * every q) of which block (q, l) uses the first m[q] (n - m[q]) as an m[q] x k matrix, column-major with leading dimension
 * m[q]; the solution overwrites it.  from_t12 != 0: C is only written and the right-hand side is C_l = -T12_l.  Then
 * T_l [X_b; I] = [X_a; I] T22_l: Y_l = Z_l [X_l; I] spans the complementary periodic invariant subspace.  There is NO
 * scale factor (xTRSYL carries one): a nearly singular problem returns large or non-finite numbers, the latter with the
 * code below.
 *
 * psd_?_subcond_batch is the periodic form of xTRSEN's two numbers for the leading m[q] eigenvalues:
 *     s[q * p + l] = 1 / sqrt(1 + ||X_l||_F^2)   (X of from_t12: the reciprocal of the Frobenius bound on the norm of the
 *                                                 spectral projector of factor l; at p = 1 xTRSEN's S),
 *     sep[q]       = 1 / est,  est the estimate of || S^-1 ||_1 on the p m k stacked unknowns (blocks in user order, each
 *                    column-major) by LAPACK's reverse-communication estimator xLACN2 (real variant for psd_d_, complex
 *                    for psd_z_; iteration limit 5, the final alternating-sign vector); at p = 1 xTRSEN's SEP.
 * X (may be NULL): receives the solution of from_t12, laid out as C above.  m[q] = 0 or n: s = 1, sep = +inf, X untouched,
 * and the problem takes part in no launch.
 *
 * One launch solves a group of problems (one wavefront per problem, Bartels-Stewart over the common block partition, the
 * small cyclic systems by the solvers of the reordering kernels); the condition entry launches per group one solve, one
 * norm kernel and per estimator step one solve and one vector kernel — at most 1 + 11 solves.  Every sum has a fixed
 * order: a problem's numbers do not depend on nb, on its place in the batch or on the grouping, bit for bit.
 * PSD_BATCH_GROUP acts as for the other batch entries.  Orders above 128 (PSD_BSYL_NMAX; PSD_BSYL_NMAX in the environment
 * at psd_create may only lower it) return PSD_INFO_NOTIMPL: the batch entries do not fall back to the single-problem
 * entries psd_?_psylv / psd_?_subcond below, which the caller uses above the cap.  So do
 * periods whose small-block scratch does not fit the LDS (psd_z_: p > 19; psd_d_: p > 136).
 *
 * T: nb * p host matrices (psd_z_: interleaved complex), column-major, USER order, only read; the _dev variants take
 * device [nb][p][n][n] blocks (what the *_pschur_batch_dev / *_ordschur_batch_dev entries leave) and device
 * [nb][p][xb] blocks for C / X; m, s, sep, infos are host arrays.  infos[nb] (may be NULL): PSD_INFO_SINGULAR for a
 * problem whose small solve was rejected (T11 and T22 share an eigenvalue of the product) or whose solution is not
 * finite — its X is NaN, s = 0, sep = 0 — the others are complete; the return value is the first non-zero one.
 * Returns: -1 ctx NULL; -2 nb < 0; -3 n < 1; -4 p < 1; -5 T NULL; -6 orient; -7 schurindex not in 1..p; -8 m NULL, an
 * m[q] outside 0..n or inside a 2x2 block; -9 C NULL (subcond: s or sep NULL); -10 xb below the largest m[q] (n - m[q])
 * (subcond: only with X); PSD_INFO_NOTIMPL above the cap and on a period-sharded context; PSD_INFO_RUNTIME + k.
 * nb == 0 returns 0 and touches nothing. */
typedef struct psd_bsylv_stats {
    int32_t nb;         /* problems of the call */
    int32_t ngroups;    /* groups the batch went to the device in */
    int32_t nsolve;     /* launches of the solve kernel */
    int32_t nnorms;     /* launches of the norm kernel */
    int32_t nest_steps; /* launches of the estimator's vector kernel */
    int32_t nest_iter;  /* most iterations the estimator took on a problem (<= 5) */
    int32_t nsingular;  /* problems that ended with PSD_INFO_SINGULAR */
    int32_t reserved;
    double ms_kernels;  /* device time of the kernels and their read-backs */
    double ms_copy;     /* host entries: time of the copies */
} psd_bsylv_stats;
int psd_d_psylv_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, char orient, int schurindex, const int* m,
                      double* const* C, int64_t xb, int trans, int from_t12, int* infos, psd_bsylv_stats* stats, int* info);
int psd_z_psylv_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, char orient, int schurindex, const int* m,
                      double* const* C, int64_t xb, int trans, int from_t12, int* infos, psd_bsylv_stats* stats, int* info);
int psd_d_psylv_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dT, char orient, int schurindex, const int* m,
                          double* dC, int64_t xb, int trans, int from_t12, int* infos, psd_bsylv_stats* stats, int* info);
int psd_z_psylv_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dT, char orient, int schurindex, const int* m,
                          double* dC, int64_t xb, int trans, int from_t12, int* infos, psd_bsylv_stats* stats, int* info);
int psd_d_subcond_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, char orient, int schurindex, const int* m,
                        double* s, double* sep, double* const* X, int64_t xb, int* infos, psd_bsylv_stats* stats, int* info);
int psd_z_subcond_batch(psd_ctx* ctx, int nb, int n, int p, double* const* T, char orient, int schurindex, const int* m,
                        double* s, double* sep, double* const* X, int64_t xb, int* infos, psd_bsylv_stats* stats, int* info);
int psd_d_subcond_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dT, char orient, int schurindex, const int* m,
                            double* s, double* sep, double* dX, int64_t xb, int* infos, psd_bsylv_stats* stats, int* info);
int psd_z_subcond_batch_dev(psd_ctx* ctx, int nb, int n, int p, const double* dT, char orient, int schurindex, const int* m,
                            double* s, double* sep, double* dX, int64_t xb, int* infos, psd_bsylv_stats* stats, int* info);

/* ---- psylv, subcond: the same for ONE periodic Schur form of any order ----------------------------------------------
 * The single-problem entries of the family above, with its definitions, argument conventions and codes: S, trans,
 * from_t12, s, sep (xLACN2 on the p m k stacked unknowns in user order), m = 0 or n (s = 1, sep = +inf, X untouched, no
 * launch), no scale factor.  The arguments are those of the batch entries without nb, xb and infos: m is one int, and
 * the p blocks of C / X are m x k, column-major, leading dimension m (the _dev variants: one device array [p][m k],
 * dT [p][n][n]).  T is only read.
 *
 * The solve is a tiled Bartels-Stewart walk: the rows of T11 and the columns of T22 are cut at multiples of the tile
 * width (a boundary that would cut a 2x2 block of the quasi-triangular factor moves by one), the tiles of one
 * anti-diagonal are solved in one launch by the body of the batch kernel, one wavefront per tile, and before that their
 * right-hand sides receive the sums over the tiles solved earlier from a matrix-core update kernel (left-looking, K
 * ascending, every tile of C written by one workgroup once: for one tile width the result is the same bits on every
 * run; another width may round differently).  With a tile at least max(m, k) wide the call is one tile, no update, and
 * the arithmetic of the batch kernel.  The tile width is PSD_SYL_TILE of psd_sylv.h; PSD_SYL_TILE in the environment at
 * psd_create sets another one in 2 ... 128 (anything else: the default).  Periods whose small-block scratch does not
 * fit the LDS (psd_z_: p > 19; psd_d_: p > 136) and a period-sharded context return PSD_INFO_NOTIMPL.
 *
 * Returns: -1 ctx NULL; -3 n < 1; -4 p < 1; -5 T NULL; -6 orient; -7 schurindex not in 1..p; -8 m outside 0..n or inside
 * a 2x2 block; -9 C NULL (subcond: s or sep NULL); PSD_INFO_SINGULAR where a small solve was rejected (T11 and T22 share
 * an eigenvalue of the product) or the numbers are not finite — X is NaN, s = 0, sep = 0 —; PSD_INFO_NOTIMPL;
 * PSD_INFO_RUNTIME + k. */
typedef struct psd_sylv_stats {
    int32_t tile;        /* tile width of the call */
    int32_t ntiles;      /* tiles of X */
    int32_t ndiag;       /* anti-diagonals of the tile walk */
    int32_t nsolve;      /* launches of the tile solve kernel */
    int32_t nupdate;     /* launches of the update kernel */
    int32_t nnorms;      /* launches of the norm kernel */
    int32_t nest_steps;  /* launches of the estimator's vector kernel */
    int32_t nest_solves; /* applications of S^-1 or S^-H the estimator took (<= 11) */
    int32_t nest_iter;   /* iterations of the estimator (<= 5) */
    int32_t nsingular;   /* 1: the call ended with PSD_INFO_SINGULAR */
    double ms_solve;     /* device time of the tile solve launches */
    double ms_update;    /* device time of the update launches */
    double ms_est;       /* subcond: device time of the norm and vector kernels and the read-backs between the steps */
    double ms_copy;      /* host entries: time of the copies */
} psd_sylv_stats;
int psd_d_psylv(psd_ctx* ctx, int n, int p, double* const* T, char orient, int schurindex, int m, double* const* C,
                int trans, int from_t12, psd_sylv_stats* stats, int* info);
int psd_z_psylv(psd_ctx* ctx, int n, int p, double* const* T, char orient, int schurindex, int m, double* const* C,
                int trans, int from_t12, psd_sylv_stats* stats, int* info);
int psd_d_psylv_dev(psd_ctx* ctx, int n, int p, const double* dT, char orient, int schurindex, int m, double* dC, int trans,
                    int from_t12, psd_sylv_stats* stats, int* info);
int psd_z_psylv_dev(psd_ctx* ctx, int n, int p, const double* dT, char orient, int schurindex, int m, double* dC, int trans,
                    int from_t12, psd_sylv_stats* stats, int* info);
int psd_d_subcond(psd_ctx* ctx, int n, int p, double* const* T, char orient, int schurindex, int m, double* s, double* sep,
                  double* const* X, psd_sylv_stats* stats, int* info);
int psd_z_subcond(psd_ctx* ctx, int n, int p, double* const* T, char orient, int schurindex, int m, double* s, double* sep,
                  double* const* X, psd_sylv_stats* stats, int* info);
int psd_d_subcond_dev(psd_ctx* ctx, int n, int p, const double* dT, char orient, int schurindex, int m, double* s,
                      double* sep, double* dX, psd_sylv_stats* stats, int* info);
int psd_z_subcond_dev(psd_ctx* ctx, int n, int p, const double* dT, char orient, int schurindex, int m, double* s,
                      double* sep, double* dX, psd_sylv_stats* stats, int* info);

/* ---- diagnostic entry of the walk's update kernel ---------------------------------------------------------------------
 * TEST PLUMBING like the diagnostic entries of the dense Krylov kernels above, without a Julia binding: ONE launch of
 * psd_syl_update through the walk's own checks, partition and launch code, so that a test can compare the kernel with a
 * high-precision reference at a chosen tile width and anti-diagonal.  T, orient, schurindex and m as psd_?_psylv; X: the
 * p blocks m x k (in / out), every entry meaningful: the launch reads the tiles the walk would have solved before
 * anti-diagonal d and adds the two sums of psd_sylv.h to the tiles of d (trans != 0: the sums of S^H; from_t12 != 0: the
 * tiles of d start from -T12 and not from what X holds).  Nothing else of X is written, no tile is solved.
 * tile: the tile width of this call, 2 ... 128 (the context's width and PSD_SYL_TILE are not consulted).
 * d: 1 ... nI + nJ - 2 (anti-diagonal 0 has no update; the walk numbers them as psd_sylv.h says).
 * geom (may be NULL): the partition and the grid; bounds (may be NULL): n + 2 ints, receives the row boundaries of T11
 * rb[0 .. nI] = 0 ... m followed by the local column boundaries of T22 cb[0 .. nJ] = 0 ... k.
 * info: the codes -1 ... -9 of psd_?_psylv; -10 tile outside 2 ... 128; -11 d outside 1 ... nI + nJ - 2 (geom is set,
 * nothing is launched, X is untouched; m = 0 or n has no anti-diagonal); PSD_INFO_NOTIMPL; PSD_INFO_RUNTIME + k. */
typedef struct psd_syl_geom {
    int32_t nI, nJ;  /* tiles per column and per row of X */
    int32_t nsb;     /* 32 x 32 sub-blocks per tile and dimension: ceil((tile + 1) / 32) */
    int32_t ndtiles; /* tiles on anti-diagonal d: the grid is (ndtiles nsb nsb, p) */
} psd_syl_geom;
int psd_d_syl_update(psd_ctx* ctx, int n, int p, double* const* T, char orient, int schurindex, int m, double* const* X,
                     int tile, int d, int trans, int from_t12, psd_syl_geom* geom, int32_t* bounds, int* info);
int psd_z_syl_update(psd_ctx* ctx, int n, int p, double* const* T, char orient, int schurindex, int m, double* const* X,
                     int tile, int d, int trans, int from_t12, psd_syl_geom* geom, int32_t* bounds, int* info);

#ifdef __cplusplus
}
#endif
#endif
