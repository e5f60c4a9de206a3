"""CPU tier: partial_pschur (periodic Krylov-Schur, src/krylov.jl:446-798) on the TEST-ONLY serial simulation of the
device code (tests/hostsim): the kernels of psd_krylov.h and the host driver, against the reference's test problem
(test/krylov.jl) and the CPU oracle's full spectrum."""
import ctypes as C

import numpy as np
import pytest

import krylov_cases as kc


@pytest.fixture(scope="module")
def real_problem():
    As = kc.mkmats1(30, 3, seed=11)
    return As, kc.full_values(As)


@pytest.fixture(scope="module")
def cplx_problem():
    As = kc.mkmats1(30, 3, cplx=True, seed=12)
    return As, kc.full_values(As)


@pytest.mark.parametrize("which", ["LM", "SR", "LR"])
def test_real_targets(sim_engine, real_problem, which):
    As, vfull = real_problem
    kc.pkstest(sim_engine, As, which, vfull)


@pytest.mark.parametrize("which", ["LM", "SR", "LR", "LI", "SI"])
def test_complex_targets(sim_engine, cplx_problem, which):
    As, vfull = cplx_problem
    kc.pkstest(sim_engine, As, which, vfull)


def test_larger_n200_p8(sim_engine):
    As = kc.mkmats1(200, 8, xpnd=1.05, seed=13, unit=True)
    kc.pkstest(sim_engine, As, "LM", kc.full_values(As))


@pytest.mark.parametrize("cplx", [False, True])
def test_period_one(sim_engine, cplx):
    As = kc.mkmats1(30, 1, cplx=cplx, seed=14)
    kc.pkstest(sim_engine, As, "LM", kc.full_values(As))


def test_defaults_and_history(sim_engine, real_problem):
    As, vfull = real_problem
    P, h = sim_engine.partial_pschur(As, 3)  # the reference's defaults: LM, mindim 10, maxdim 20, tol sqrt(eps)
    assert h.converged and h.nconverged == P.Z[0].shape[1] >= 3
    assert P.stats.restarts >= 1 and P.stats.nprods == h.mvproducts
    kc.check(P, As, np.sqrt(kc.EPS))
    for lam in P.values:  # (with the larger default subspace more values converge than were asked for)
        assert np.min(np.abs(vfull - lam) / np.abs(vfull)) < 1e-5


def test_argument_errors(sim_engine, real_problem):
    As, _ = real_problem
    eng = sim_engine
    with pytest.raises(ValueError):
        eng.partial_pschur(As, 0)
    with pytest.raises(ValueError):
        eng.partial_pschur(As, 4, "XX")
    with pytest.raises(ValueError):
        eng.partial_pschur(As, 4, mindim=3, maxdim=12)
    with pytest.raises(ValueError):
        eng.partial_pschur(As, 4, mindim=8, maxdim=6)
    with pytest.raises(ValueError):
        eng.partial_pschur(As, 4, mindim=6, maxdim=91)  # > p n
    with pytest.raises(ValueError):
        eng.partial_pschur(As, 4, u1=np.ones(29))
    with pytest.raises(ValueError):
        eng.partial_pschur([As[0], As[1][:5, :5]], 2)


def _abi_call(eng, n, p, nev=2, which=b"M", mindim=4, maxdim=6, u1=None, tol=1e-8, tol1=1e-14, restarts=10,
              purgebuffer=2, A="ok", T="ok", Z="ok", wr="ok", nconv="ok"):
    mats = [np.asfortranarray(np.eye(n)) for _ in range(p)]
    Ts = [np.zeros((maxdim, maxdim)) for _ in range(p)]
    Zs = [np.zeros((n, maxdim)) for _ in range(p)]
    w = np.zeros(max(maxdim, 1))
    dp = C.POINTER(C.c_double)
    info = C.c_int(0)
    k = C.c_int(0)
    up = u1.ctypes.data_as(dp) if u1 is not None else None
    rc = eng.lib.psd_d_partial_pschur(eng.ctx, n, p, eng._ptrs(mats) if A == "ok" else None, nev, which, mindim,
                                      maxdim, up, 0, tol, tol1, restarts, purgebuffer,
                                      C.byref(k) if nconv == "ok" else None, eng._ptrs(Ts) if T == "ok" else None,
                                      eng._ptrs(Zs) if Z == "ok" else None, w.ctypes.data_as(dp) if wr == "ok" else None,
                                      w.ctypes.data_as(dp), None, C.byref(info))
    assert rc == info.value
    return rc


def test_abi_argument_codes(sim_engine):
    """krylov.jl:456-470 and the ABI's own checks map to the negative info values documented in psd_mi355x.h."""
    eng = sim_engine
    n, p = 8, 2
    assert _abi_call(eng, 0, p) == -2
    assert _abi_call(eng, n, 0) == -3
    assert _abi_call(eng, n, p, A=None) == -4
    assert _abi_call(eng, n, p, nev=0) == -5
    assert _abi_call(eng, n, p, which=b"X") == -6
    assert _abi_call(eng, n, p, nev=5, mindim=4) == -7
    assert _abi_call(eng, n, p, mindim=7, maxdim=6) == -7
    assert _abi_call(eng, n, p, maxdim=17) == -7
    assert _abi_call(eng, 3000, 2, maxdim=2049) == -8
    assert _abi_call(eng, n, p, u1=np.zeros(n)) == -9
    assert _abi_call(eng, n, p, tol=0.0) == -11
    assert _abi_call(eng, n, p, tol1=-1.0) == -12
    assert _abi_call(eng, n, p, restarts=-1) == -13
    assert _abi_call(eng, n, p, purgebuffer=-1) == -14
    assert _abi_call(eng, n, p, nconv=None) == -15
    assert _abi_call(eng, n, p, T=None) == -16
    assert _abi_call(eng, n, p, Z=None) == -17
    assert _abi_call(eng, n, p, wr=None) == -18


def test_reproducible_u1_and_seed(sim_engine, real_problem):
    As, _ = real_problem
    u1 = np.random.default_rng(3).standard_normal(30)
    kw = dict(mindim=6, maxdim=12, tol=1e-10, restarts=60)
    a = sim_engine.partial_pschur(As, 4, "LM", u1=u1, **kw)
    b = sim_engine.partial_pschur(As, 4, "LM", u1=u1, **kw)
    kc.same_bits(*a, *b)
    c = sim_engine.partial_pschur(As, 4, "LM", seed=77, **kw)
    d = sim_engine.partial_pschur(As, 4, "LM", seed=77, **kw)
    kc.same_bits(*c, *d)
    e = sim_engine.partial_pschur(As, 4, "LM", seed=78, **kw)
    assert not np.array_equal(np.asarray(c[0].Z[0]), np.asarray(e[0].Z[0]))


def test_rank_deficient_reinitialises(sim_engine):
    """A factor of rank 3: the vector of step 4 lies in the span of the next basis, so the device flags the step, the
    host re-initialises (krylov.jl:152-182) and deflates (:184-226); the result is still a partial decomposition."""
    As = kc.rank_deficient(30, 3, 3)
    P, h = sim_engine.partial_pschur(As, 2, "LM", mindim=6, maxdim=12, tol=1e-10, restarts=60, seed=5)
    st = P.stats
    assert st.nreinit > 0 and st.ndeflate > 0, st.asdict()
    assert P.Z[0].shape[1] >= 1
    kc.check(P, As, 1e-10)
    vfull = kc.full_values(As)
    scale = np.max(np.abs(vfull))
    for lam in P.values:  # (the zero eigenvalues of the singular product are valid answers too)
        assert np.min(np.abs(vfull - lam)) <= 1e-5 * scale


@pytest.mark.parametrize("n,p,kw", [(31, 3, {}), (257, 2, dict(xpnd=1.05, unit=True)), (513, 2, dict(xpnd=1.02, unit=True))])
def test_odd_real_orders(sim_engine, n, p, kw):
    """Odd orders take the one-row body psd_kr_mv<false, 1> of the Float64 matvec through the whole driver (one row
    either side of a tile at 257 and 513)."""
    As = kc.mkmats1(n, p, **kw)
    kc.pkstest(sim_engine, As, "LM", kc.full_values(As))


@pytest.mark.parametrize("cplx", [False, True])
def test_wide_subspace(sim_engine, cplx):
    """maxdim = 300 > 256: see krylov_cases.wide_subspace."""
    P, h = kc.wide_subspace(sim_engine, cplx)
    assert P.stats.restarts >= 1


def test_bit_identical_runs_odd_order(sim_engine):
    As = kc.mkmats1(257, 2, xpnd=1.05, seed=23, unit=True)
    kw = dict(mindim=6, maxdim=12, tol=1e-10, restarts=60, seed=9)
    kc.same_bits(*sim_engine.partial_pschur(As, 4, "LM", **kw), *sim_engine.partial_pschur(As, 4, "LM", **kw))
