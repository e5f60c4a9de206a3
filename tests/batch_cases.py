"""Cases for the batched entries (Engine.phessenberg_batch_ / pschur_batch_ / pschur_batch): many small general problems
of one shape in one call.  Each case takes an engine; tests/test_hostsim_pschur_batch.py runs them on the serial
simulation, tests/test_gpu_pschur_batch.py on the device.  Factors come from pt.bench_factors."""
import numpy as np
import pytest

import psd_amd
import psdtest as pt

# (nb, n, p).  (2, 33, 2) crosses the 8-row strip and the 4-column block of the update bodies and goes past one wavefront.
HESS_SHAPES = [(3, 2, 1), (3, 5, 1), (4, 9, 2), (2, 33, 2)]
# p >= 3: the single call of the device build takes the look-ahead form (other rounding); the simulation the one-stream form
HESS_SHAPES_P3 = [(3, 12, 3), (2, 17, 5)]
# (33, 6, 3) crosses the 32-problem chunk of the iteration
FULL_SHAPES = [(33, 6, 3), (5, 1, 4), (4, 2, 2), (3, 24, 1), (6, 20, 3), (2, 40, 8)]

_cache = {}


def problems(nb, n, p):
    """The factors of a shape: built once, shared, never written to."""
    key = (nb, n, p)
    if key not in _cache:
        probs = [pt.bench_factors(n, p, seed=7000 + 131 * q + 7 * n + p) for q in range(nb)]
        for A in probs:
            for a in A:
                a.setflags(write=False)
        _cache[key] = probs
    return _cache[key]


def work(A):
    return [np.array(a, order="F", copy=True) for a in A]


def shape_id(s):
    return "nb%d_n%d_p%d" % s


# ------------------------------------------------------------------------------------------------
# 1. reduction
def case_reduction_bits(eng, shape):
    """phessenberg_batch_ against phessenberg_ problem by problem: the same bodies in the same order, so the packed H
    (reflectors below the diagonal included) and tau are equal bit for bit."""
    nb, n, p = shape
    probs = problems(*shape)
    Wb = [work(A) for A in probs]
    out, st = eng.phessenberg_batch_(Wb)
    assert len(out) == nb
    for q in range(nb):
        W1 = work(probs[q])
        H1, tau1, _ = eng.phessenberg_(W1)
        for j in range(p):
            assert np.array_equal(W1[j], Wb[q][j]), (shape, q, j)
            assert np.array_equal(H1[j], out[q][0][j]), (shape, q, j)
        assert np.array_equal(tau1, out[q][1]), (shape, q)


def _q_from_reflectors(Apacked, tau, first):
    """Q = H_1 ... H_{n-1} from LAPACK-style storage: the reflector of column c acts on rows c + first ... n - 1
    (first = 1 for the Hessenberg factor, 0 for the triangular ones)."""
    n = Apacked.shape[0]
    Q = np.eye(n)
    for c in range(n - 2, -1, -1):
        r0 = c + first
        if r0 > n - 2:
            continue
        v = np.zeros(n)
        v[r0] = 1.0
        v[r0 + 1:] = Apacked[r0 + 1:, c]
        Q -= tau[c] * np.outer(v, v @ Q)
    return Q


def case_reduction_close(eng, shape):
    """For shapes whose single call rounds differently (look-ahead form): triu parts equal to 1e-13 ||A||, the Q_j of the
    batched reduction orthogonal, and Q_j' A_j Q_{j+1} = H_j.

    Bounds: orthogonality 10 eps n as pt.pschur_check demands of Z; residual 10 n eps ||A_j||_F — n - 1 reflectors from
    either side, each a backward error of a few eps ||A_j||_F (Higham, Accuracy and Stability, Lemma 19.3)."""
    nb, n, p = shape
    probs = problems(*shape)
    Wb = [work(A) for A in probs]
    out, st = eng.phessenberg_batch_(Wb)
    for q in range(nb):
        A = probs[q]
        W1 = work(A)
        H1, tau1, _ = eng.phessenberg_(W1)
        anorm = max(np.linalg.norm(a, 2) for a in A)
        Hb, taub = out[q]
        for j in range(p):
            d = np.abs(Hb[j] - H1[j]).max()
            print(f"{shape} q={q} j={j}: |H_batch - H_single| = {d:.3e} (bound {1e-13 * anorm:.3e})")
            assert d <= 1e-13 * anorm, (shape, q, j, d)
        Qs = [_q_from_reflectors(Wb[q][j], taub[j], 1 if j == 0 else 0) for j in range(p)]
        for j in range(p):
            orth = np.linalg.norm(Qs[j].T @ Qs[j] - np.eye(n))
            assert orth < 10 * pt.EPS * n, (shape, q, j, orth)
            res = np.linalg.norm(Qs[j].T @ A[j] @ Qs[(j + 1) % p] - Hb[j])
            assert res < 10 * n * pt.EPS * np.linalg.norm(A[j]), (shape, q, j, res)


# ------------------------------------------------------------------------------------------------
# 2. full decomposition
def check_problem(A, ps, lr, single_values=None):
    """The checks of engine_cases.case_pschur_hess_batch, for a general problem in orientation lr."""
    n = A[0].shape[0]
    pt.pschur_check(A, ps, tol=100 * max(1.0, np.sqrt(n / 32)), check_lam=False)
    P = pt.product(A, lr == "L")
    sc = np.linalg.norm(P, 2)
    assert pt.match_eigs(np.linalg.eigvals(P), ps.values) <= 1e-10 * sc * max(1.0, np.linalg.cond(P) * 1e-6)
    if single_values is not None:
        assert pt.match_eigs(single_values, ps.values) <= 1e-10 * sc
    return sc


def case_full(eng, shape, lr):
    nb, n, p = shape
    probs = problems(*shape)
    batch = eng.pschur_batch(probs, lr)
    assert len(batch) == nb
    for q in range(nb):
        assert batch[q].orientation == lr and batch[q].schurindex == (p if lr == "L" else 1)
        single = eng.pschur(work(probs[q]), lr)
        check_problem(probs[q], batch[q], lr, single.values)
    # a problem does not depend on its neighbours: alone in a batch of one it gives the same spectrum
    for q in sorted({0, nb - 2, nb - 1} & set(range(nb))):
        alone = eng.pschur_batch([probs[q]], lr)
        sc = np.linalg.norm(pt.product(probs[q], lr == "L"), 2)
        assert pt.match_eigs(alone[0].values, batch[q].values) <= 1e-10 * sc, (shape, lr, q)


# ------------------------------------------------------------------------------------------------
# 3. flags
def case_flags(eng, shape=(5, 12, 3)):
    nb, n, p = shape
    probs = problems(*shape)
    for lr in ("R", "L"):
        full = eng.pschur_batch(probs, lr)
        noz = eng.pschur_batch(probs, lr, wantZ=False)
        not_ = eng.pschur_batch(probs, lr, wantZ=False, wantT=False)
        for q in range(nb):
            sc = np.linalg.norm(pt.product(probs[q], lr == "L"), 2)
            assert noz[q].Z == [] and not_[q].Z == []
            assert pt.match_eigs(full[q].values, noz[q].values) <= 1e-10 * sc
            assert pt.match_eigs(full[q].values, not_[q].values) <= 1e-10 * sc
            for ps in (full[q], noz[q], not_[q]):
                assert ps.schurindex == (1 if lr == "R" else p) and ps.orientation == lr
        # a batch of one equals the plain call
        W = work(probs[0])
        b1 = eng.pschur_batch_([W], lr)
        assert b1[0].Ts[0] is W[0]  # in place
        s1 = eng.pschur(probs[0], lr)
        check_problem(probs[0], b1[0], lr, s1.values)
    # the copying form leaves its input alone (the shared factors are read-only: a write would have raised)
    assert all(not a.flags.writeable for A in probs for a in A)


# ------------------------------------------------------------------------------------------------
# 4. one failing problem
def one_fails_problems(n=24, p=3):
    """Three problems whose product needs a handful of sweeps — triangular factors with one 3 x 3 block in A_1 (already
    Hessenberg-triangular: every reflector of the reduction is the identity) — around one full random problem."""
    def easy(seed):
        A = [np.triu(a) for a in pt.bench_factors(n, p, seed=seed)]
        full = pt.bench_factors(n, 1, seed=seed + 977)[0]
        for k in (9, 10):
            A[0][k + 1, k] = full[k + 1, k]
        return [np.asfortranarray(a) for a in A]
    return [easy(41), pt.bench_factors(n, p, seed=42), easy(43), easy(44)]


def case_one_fails(eng, single_pattern=True):
    """maxitfac = 2 (2 n sweeps, PSD.jl:471,891-893): the full problem exhausts its budget and ends alone; the other
    three are complete and correct.  single_pattern: the single call with the same maxitfac fails for exactly that one."""
    probs = one_fails_problems()
    if single_pattern:
        for q, A in enumerate(probs):
            if q == 1:
                with pytest.raises(psd_amd.ConvergenceError):
                    eng.pschur(A, "R", maxitfac=2)
            else:
                eng.pschur(A, "R", maxitfac=2)
    infos = []
    out = eng.pschur_batch(probs, "R", maxitfac=2, infos_out=infos)
    assert len(infos) == 4 and infos[0] == 0 and infos[2] == 0 and infos[3] == 0, infos
    assert psd_amd.INFO_NOCONV <= infos[1] < psd_amd.INFO_NOTIMPL, infos
    for q in (0, 2, 3):
        check_problem(probs[q], out[q], "R")
    Ws = [work(A) for A in probs]
    with pytest.raises(psd_amd.ConvergenceError):  # raised after all four have run
        eng.pschur_batch_(Ws, "R", maxitfac=2)
    for q in (0, 2, 3):  # ... so the in-place factors of the others are their T factors
        assert np.all(np.tril(Ws[q][0], -2) == 0) and all(np.all(np.tril(w, -1) == 0) for w in Ws[q][1:])
        assert pt.match_eigs(out[q].values, np.linalg.eigvals(pt.product(Ws[q]))) <= 1e-10 * np.linalg.norm(pt.product(probs[q]), 2)


# ------------------------------------------------------------------------------------------------
# 5. argument errors
def case_argument_errors(eng):
    A = problems(3, 5, 1)
    B = problems(4, 9, 2)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.pschur_batch([A[0], B[0][:1]])  # unequal order
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.pschur_batch([B[0], B[1][:1]])  # unequal period
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.phessenberg_batch_([work(B[0]), work(A[0])])
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.pschur_batch([[a.astype(np.complex128) for a in A[0]]])
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.pschur_batch_([[np.asfortranarray(a.astype(np.complex128)) for a in A[0]]])
    with pytest.raises(TypeError):
        eng.pschur_batch_([[np.ascontiguousarray(a) for a in B[0]]])  # in place needs Fortran order
    with pytest.raises(ValueError):
        eng.pschur_batch(A, "X")
    assert eng.pschur_batch([]) == [] and eng.pschur_batch_([], "L") == []
    infos = [7]
    assert eng.pschur_batch([], infos_out=infos) == [] and infos == []


def case_abi_codes(eng, shape=(5, 12, 3)):
    """The argument codes of the four C entries of the real family, as zbatch_cases.case_abi_codes: the return value and
    *info agree, code by code.  Every call ends in the argument checks, so the pointers are never followed (the packed
    host block stands in for a device buffer)."""
    import ctypes as C

    nb, n, p = shape
    probs = problems(*shape)
    lib, ctx = eng.lib, eng.ctx
    dp = C.POINTER(C.c_double)
    A = work(probs[0])
    ptrs = eng._ptrs(A)
    dA = np.ascontiguousarray(np.array([pt.pack(A)]))
    buf = C.c_void_p(dA.ctypes.data)
    tau, w = np.zeros((p, n)), np.zeros(n)
    wp, tp = w.ctypes.data_as(dp), tau.ctypes.data_as(dp)

    def both(call):
        """the code of a call, returned and stored alike"""
        info = C.c_int(12345)
        rc = call(C.byref(info))
        assert rc == info.value, (rc, info.value)
        return rc

    def hess(c=ctx, nb_=1, n_=n, p_=p, A_=ptrs, tau_=tp):
        return both(lambda ip: lib.psd_d_phessenberg_batch(c, nb_, n_, p_, A_, tau_, None, ip))

    def host_(c=ctx, nb_=1, n_=n, p_=p, A_=ptrs, o=b"R", mi=30, wz=0, Z_=None, wr_=wp, wi_=wp):
        return both(lambda ip: lib.psd_d_pschur_batch(c, nb_, n_, p_, A_, o, 1, wz, mi, Z_, wr_, wi_, None, None, None, ip))

    def dev_(c=ctx, nb_=1, n_=n, p_=p, A_=buf, o=b"R", mi=30, wz=0, Z_=None, wr_=wp, wi_=wp):
        return both(lambda ip: lib.psd_d_pschur_batch_dev(c, nb_, n_, p_, A_, o, 1, wz, mi, Z_, wr_, wi_, None, None, None, ip))

    def hb_(c=ctx, nb_=1, n_=n, p_=p, H_=ptrs, mi=30, wz=0, Q_=None, wr_=wp, wi_=wp):
        return both(lambda ip: lib.psd_d_pschur_hess_batch(c, nb_, n_, p_, H_, Q_, 1, wz, mi, wr_, wi_, None, None, ip))

    assert hess(c=None) == -1 and hess(nb_=0) == -2 and hess(n_=0) == -3 and hess(p_=0) == -4
    assert hess(A_=None) == -5 and hess(tau_=None) == -6
    for f in (host_, dev_):
        assert f(c=None) == -1 and f(nb_=0) == -2 and f(nb_=-3) == -2 and f(n_=0) == -3 and f(p_=0) == -4
        assert f(A_=None) == -5 and f(o=b"X") == -6 and f(mi=0) == -9 and f(wz=1) == -10
        assert f(wr_=None) == -11 and f(wi_=None) == -11
    assert hb_(c=None) == -1 and hb_(nb_=0) == -2 and hb_(nb_=33) == -2  # (at most 32 problems side by side)
    assert hb_(n_=0) == -3 and hb_(p_=0) == -4  # (returned and stored alike: the codes of psd_z_pschur_hess_batch)
    assert hb_(H_=None) == -5 and hb_(wz=1) == -6 and hb_(mi=0) == -9 and hb_(wr_=None) == -10 and hb_(wi_=None) == -10
    # the first bad argument decides
    assert hb_(nb_=33, n_=0) == -2 and hb_(n_=0, p_=0) == -3 and host_(nb_=0, n_=0) == -2 and dev_(p_=0, A_=None) == -4
    # a null info is allowed
    assert lib.psd_d_pschur_hess_batch(ctx, 1, 0, p, ptrs, None, 1, 0, 30, wp, wp, None, None, None) == -3
    assert lib.psd_d_pschur_batch(ctx, 0, n, p, ptrs, b"R", 1, 0, 30, None, wp, wp, None, None, None, None) == -2


def _same_bits(whole, parts, p, withZ=True):
    for q in range(len(whole)):
        assert np.array_equal(whole[q].values, parts[q].values), q
        for j in range(p):
            assert np.array_equal(whole[q].Ts[j], parts[q].Ts[j]), (q, j)
            if withZ:
                assert np.array_equal(whole[q].Z[j], parts[q].Z[j]), (q, j)


def case_groups(make_engine, shape=(6, 20, 3)):
    """A host entry whose batch does not fit the device at once works through it in groups (PSD_BATCH_GROUP lowers the
    group size): the same results as in one group, problem by problem."""
    nb, n, p = shape
    probs = problems(*shape)
    ref = make_engine({})
    eng = make_engine({"PSD_BATCH_GROUP": "4"})
    # one list of matrices through the loop (no Z), bit for bit
    _same_bits(ref.pschur_batch(probs, "L", wantZ=False), eng.pschur_batch(probs, "L", wantZ=False), p, withZ=False)
    whole = ref.pschur_batch(probs, "L")
    parts = eng.pschur_batch(probs, "L")
    for q in range(nb):
        assert np.array_equal(whole[q].values, parts[q].values)
        for j in range(p):
            assert np.array_equal(whole[q].Ts[j], parts[q].Ts[j]) and np.array_equal(whole[q].Z[j], parts[q].Z[j])
    Wb, Wp = [work(A) for A in probs], [work(A) for A in probs]
    ob, _ = ref.phessenberg_batch_(Wb)
    op, _ = eng.phessenberg_batch_(Wp)
    for q in range(nb):
        assert np.array_equal(ob[q][1], op[q][1]) and all(np.array_equal(Wb[q][j], Wp[q][j]) for j in range(p))
    # the reduced factors through pschur_hess_batch_, bit for bit: H and Q both go up and come down (Q_j on entry: any
    # orthogonal matrices, the same for both engines)
    rng = np.random.default_rng(20)
    Qs = [[np.asfortranarray(np.linalg.qr(rng.standard_normal((n, n)))[0]) for _ in range(p)] for _ in range(nb)]
    infos_w, infos_p = [], []
    hw = ref.pschur_hess_batch_([(H[0], H[1:], Q) for H, Q in zip([work(o[0]) for o in ob], [work(Q) for Q in Qs])],
                                infos_out=infos_w)
    hp = eng.pschur_hess_batch_([(H[0], H[1:], Q) for H, Q in zip([work(o[0]) for o in op], [work(Q) for Q in Qs])],
                                infos_out=infos_p)
    assert infos_w == infos_p == [0] * nb
    _same_bits(hw, hp, p)
    assert hw[0].stats.nsweeps > 0 and hp[0].stats.nsweeps > 0


# ------------------------------------------------------------------------------------------------
# device-resident entry
def case_device_resident(eng, shape=(5, 12, 3)):
    """One torch [nb, p, n, n] tensor through psd_d_pschur_batch_dev: T, Z and the values equal the host entry's to 1e-12
    relative (the same kernels on the same data; the entries differ in the copies alone)."""
    import torch

    nb, n, p = shape
    probs = problems(*shape)
    for lr in ("R", "L"):
        host = eng.pschur_batch(probs, lr)
        dA = torch.from_numpy(np.array([[np.array(a) for a in A] for A in probs])).cuda()
        keep = dA.clone()
        T, Z, values, st = eng.pschur_batch(dA, lr)
        assert isinstance(T, torch.Tensor) and T.is_cuda and Z.is_cuda and tuple(T.shape) == (nb, p, n, n)
        assert torch.equal(dA, keep)  # the input stays as it was
        Th, Zh = T.cpu().numpy(), Z.cpu().numpy()
        for q in range(nb):
            sc = max(np.linalg.norm(a, 2) for a in probs[q])
            assert np.abs(values[q] - host[q].values).max() <= 1e-12 * np.abs(host[q].values).max()
            for j in range(p):
                assert np.abs(Th[q, j] - host[q].Ts[j]).max() <= 1e-12 * sc, (lr, q, j)
                assert np.abs(Zh[q, j] - host[q].Z[j]).max() <= 1e-12, (lr, q, j)
            ps = psd_amd.PeriodicSchur([np.asfortranarray(Th[q, j]) for j in range(p)],
                                       [np.asfortranarray(Zh[q, j]) for j in range(p)], values[q], lr,
                                       p if lr == "L" else 1)
            check_problem(probs[q], ps, lr)
    Tn, Zn, vn, _ = eng.pschur_batch(dA, "R", wantZ=False)
    assert Zn is None
    for q in range(nb):
        assert pt.match_eigs(eng.pschur(probs[q], "R").values, vn[q]) <= 1e-10 * np.linalg.norm(pt.product(probs[q]), 2)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.pschur_batch(dA[:, :, :, :5])
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.pschur_batch(dA.to(torch.complex128))


def case_dev_abi(eng, shape=(5, 12, 3)):
    """psd_d_pschur_batch_dev through the C ABI on packed [nb][p][n][n] column-major blocks (in the simulation device
    memory is host memory): the same bits as the host entry, and the argument codes of all three entries."""
    import ctypes as C

    nb, n, p = shape
    probs = problems(*shape)
    dp = C.POINTER(C.c_double)
    for lr in ("R", "L"):
        host = eng.pschur_batch(probs, lr)
        dA = np.ascontiguousarray(np.array([pt.pack(A) for A in probs]))
        dZ = np.zeros_like(dA)
        wr, wi = np.zeros((nb, n)), np.zeros((nb, n))
        infos = (C.c_int * nb)()
        si, info = C.c_int(0), C.c_int(0)
        st = psd_amd.Stats()
        rc = eng.lib.psd_d_pschur_batch_dev(eng.ctx, nb, n, p, C.c_void_p(dA.ctypes.data), lr.encode(), 1, 1, 30,
                                            C.c_void_p(dZ.ctypes.data), wr.ctypes.data_as(dp), wi.ctypes.data_as(dp),
                                            infos, C.byref(si), C.byref(st), C.byref(info))
        assert rc == 0 and info.value == 0 and si.value == (p if lr == "L" else 1) and not any(infos)
        assert st.ms_total >= st.ms_hess >= 0 and st.nsweeps > 0
        for q in range(nb):
            assert np.array_equal(wr[q] + 1j * wi[q], host[q].values)
            for j in range(p):
                assert np.array_equal(dA[q, j].T, host[q].Ts[j]) and np.array_equal(dZ[q, j].T, host[q].Z[j])
    lib, ctx = eng.lib, eng.ctx
    A = work(probs[0])
    ptrs = eng._ptrs(A)
    tau = np.zeros((p, n))
    w = np.zeros(n)
    wp, tp = w.ctypes.data_as(dp), tau.ctypes.data_as(dp)
    buf = C.c_void_p(dA.ctypes.data)

    def hess(nb_=1, n_=n, p_=p, A_=ptrs, tau_=tp):
        return lib.psd_d_phessenberg_batch(ctx, nb_, n_, p_, A_, tau_, None, None)

    def host_(nb_=1, n_=n, p_=p, A_=ptrs, o=b"R", mi=30, wz=0, Z_=None, wr_=wp):
        return lib.psd_d_pschur_batch(ctx, nb_, n_, p_, A_, o, 1, wz, mi, Z_, wr_, wp, None, None, None, None)

    def dev_(nb_=1, n_=n, p_=p, A_=buf, o=b"R", mi=30, wz=0, Z_=None, wr_=wp):
        return lib.psd_d_pschur_batch_dev(ctx, nb_, n_, p_, A_, o, 1, wz, mi, Z_, wr_, wp, None, None, None, None)

    assert hess(nb_=0) == -2 and hess(n_=0) == -3 and hess(p_=0) == -4 and hess(A_=None) == -5 and hess(tau_=None) == -6
    for f in (host_, dev_):
        assert f(nb_=0) == -2 and f(n_=0) == -3 and f(p_=0) == -4 and f(A_=None) == -5 and f(o=b"X") == -6
        assert f(mi=0) == -9 and f(wz=1) == -10 and f(wr_=None) == -11
    assert lib.psd_d_pschur_batch(None, 1, n, p, ptrs, b"R", 1, 0, 30, None, wp, wp, None, None, None, None) == -1
