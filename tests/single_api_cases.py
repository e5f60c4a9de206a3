"""Cases of the single-problem entries of the C ABI (psd_{d,z}_{phessenberg, gphessenberg, pschur, gpschur, pschur_hess,
gpschur_hess, pschur_dev, ordschur, gordschur, rphessenberg}), shared by the simulated-device tier and the GPU tier.  They
call `eng.lib` with raw ctypes, so that the return value and *info are both seen — the Python mirror validates before it
calls and reads only *info.  Three groups: the argument codes of every entry (those of include/psd_mi355x.h), the
plumbing on tiny problems (slots, switches, signatures, orientation) and the statistics block."""
import ctypes as C

import numpy as np

import psd_amd
import psdtest as pt

NOTIMPL = psd_amd.INFO_NOTIMPL
DP, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int32)
_STATS, _INFO = object(), object()
SENTINEL = -7777

# (family, complex): psd_{d|z}_{family}
ENTRIES = [("phessenberg", False), ("phessenberg", True), ("gphessenberg", False), ("gphessenberg", True),
           ("pschur", False), ("pschur", True), ("gpschur", False), ("pschur_hess", False), ("pschur_hess", True),
           ("gpschur_hess", False), ("pschur_dev", False), ("pschur_dev", True), ("ordschur", False), ("ordschur", True),
           ("gordschur", False), ("gordschur", True), ("rphessenberg", False), ("rphessenberg", True)]
# the four entries that time their copies into ms_copy
TIMES_COPIES = {("phessenberg", False), ("pschur", False), ("pschur", True), ("gpschur", False)}


def _u8(v):
    return None if v is None else (C.c_uint8 * max(len(v), 1))(*[1 if x else 0 for x in v])


def _ptr(a, t=DP):
    return a.ctypes.data_as(t)


def _on_device(eng):
    return b"hostsim" not in eng.lib.psd_version()


class _DevBlocks:
    """[p][n][n] column-major blocks where psd_?_pschur_dev wants them: host memory for the serial simulation, HBM (torch
    is only the allocator) for the product library."""

    def __init__(self, eng, mats, dt):
        self.host = pt.pack(mats, dt)
        self.t = None
        if _on_device(eng):
            import torch

            self.t = torch.from_numpy(self.host).cuda()
            torch.cuda.synchronize()

    def ptr(self):
        return C.c_void_p(self.t.data_ptr() if self.t is not None else self.host.ctypes.data)

    def fetch(self):
        return pt.unpack(self.t.cpu().numpy() if self.t is not None else self.host)


class Raw:
    """One raw call of a single-problem entry.  The statistics block and *info start from garbage, so that a call that
    leaves them alone shows."""

    def __init__(self, eng, name, argv, **keep):
        self.eng, self.name, self.argv = eng, name, argv
        self.has_stats = any(a is _STATS for a in argv)
        self.__dict__.update(keep)

    def __call__(self, info=True, stats=True):
        self.st = psd_amd.Stats()
        C.memset(C.byref(self.st), 0x55, C.sizeof(self.st))
        self.info = C.c_int(-99)
        sub = {id(_STATS): C.byref(self.st) if stats else None, id(_INFO): C.byref(self.info) if info else None}
        self.rc = getattr(self.eng.lib, self.name)(*[sub.get(id(a), a) for a in self.argv])
        return self.rc

    def matrices(self):
        """every matrix the call may write, as the caller sees them after it"""
        out = []
        for m in (self.mats, self.zs):
            if isinstance(m, _DevBlocks):
                out += m.fetch()
            elif m is not None:
                out += list(m)
        return out + ([self.ap] if self.ap is not None else [])

    def values(self):
        if len(self.eig) == 2:
            return self.eig[0] + 1j * self.eig[1]
        return psd_amd._scaled_values(*self.eig)


def _factors(cplx, n, p, seed=11, triu=False):
    A = pt.rand_uniform_zfactors(n, p, seed) if cplx else pt.rand_uniform_factors(n, p, seed)
    if triu:
        A = [np.asfortranarray(np.triu(a, -1 if j == 0 else 0)) for j, a in enumerate(A)]
    return A


def build(eng, fam, cplx, n=4, p=3, mats=None, zs=None, ctx="ok", A="ok", Z="ok", tau="ok", S=None, orient=b"R", wantT=1,
          wantZ=1, maxitfac=30, eig="ok", schurindex=1, select="ok", sel=None, maxlog=0, m=None, nq=None, nqc=None):
    """The call of entry (fam, cplx) with every argument valid, except those overridden: None for a pointer stands for
    NULL.  mats / zs: the caller's factors and transformations (made up when absent: the argument checks return before
    anything is read)."""
    t = "z" if cplx else "d"
    dt = np.complex128 if cplx else np.float64
    n1, p1 = max(n, 1), max(p, 1)
    ident = lambda k: [np.asfortranarray(np.eye(n1, dtype=dt)) for _ in range(k)]  # noqa: E731
    ap = None
    if fam == "rphessenberg":
        m = n1 if m is None else m
        ap = np.asfortranarray(_factors(cplx, max(m, n1), 1, 5)[0][:max(m, 1), :n1])
        mats = _factors(cplx, n1, max(p1 - 1, 1), 6)[:p1 - 1] if mats is None else mats
        nq, nqc = (n1 if nq is None else nq), (n1 if nqc is None else nqc)
        zs = [np.asfortranarray(np.eye(max(nq, 1), max(nqc, 1), dtype=dt)) for _ in range(p1)] if zs is None else zs
    else:
        mats = _factors(cplx, n1, p1, triu=True) if mats is None else mats
        zs = ident(p1) if zs is None else zs
    if fam == "pschur_dev":
        mats, zs = _DevBlocks(eng, mats, dt), _DevBlocks(eng, zs, dt)
        pA, pZ = mats.ptr(), zs.ptr()
    else:
        pA, pZ = (eng._ptrs(mats) if mats else None), eng._ptrs(zs)
    pA, pZ = (pA if A == "ok" else None), (pZ if Z == "ok" else None)
    real_eig = not cplx and fam in ("pschur", "pschur_hess", "pschur_dev", "ordschur")
    eigs = [np.zeros(n1), np.zeros(n1)] if real_eig else [np.zeros(n1, dtype=np.complex128), np.zeros(n1),
                                                           np.zeros(n1, dtype=np.int32)]
    pe = [_ptr(e, I32P if e.dtype == np.int32 else DP) if eig == "ok" else None for e in eigs]
    tauv = np.zeros((p1, n1), dtype=dt)
    si = C.c_int(0)
    log = np.full(3 * max(maxlog, 0) + 6, SENTINEL, dtype=np.int32) if maxlog >= 0 else None
    plog = [_ptr(log, I32P) if maxlog > 0 else None, maxlog]
    Sarr = _u8(S)
    if sel is None:
        sel = [1] + [0] * (n1 - 1)
    selarr = _u8(sel) if select == "ok" else None
    head = [eng.ctx if ctx == "ok" else None, n, p]
    sw = [wantT, wantZ, maxitfac]
    if fam == "phessenberg":
        argv = head + [pA, _ptr(tauv) if tau == "ok" else None, _STATS, _INFO]
    elif fam == "gphessenberg":
        argv = head + [pA, Sarr, pZ, _STATS, _INFO]
    elif fam == "pschur":
        argv = head + [pA, Sarr, orient] + sw + [pZ] + pe + [C.byref(si), _STATS] + plog + [_INFO]
    elif fam == "gpschur":
        argv = head + [pA, Sarr, orient] + sw + [pZ] + pe + [C.byref(si), _STATS, _INFO]
    elif fam == "pschur_hess" and not cplx:
        argv = head + [pA, pZ] + sw + pe + [_STATS] + plog + [_INFO]
    elif fam in ("pschur_hess", "gpschur_hess"):
        argv = head + [pA, Sarr, pZ] + sw + pe + [_STATS] + plog + [_INFO]
    elif fam == "pschur_dev":
        argv = head + [pA, orient] + sw + [pZ] + pe + [C.byref(si), _STATS] + plog + [_INFO]
    elif fam == "ordschur":
        argv = head + [pA, pZ, orient, schurindex, selarr, wantZ] + pe + [_STATS, _INFO]
    elif fam == "gordschur":
        argv = head + [pA, pZ, Sarr, orient, schurindex, selarr, wantZ] + pe + [_STATS, _INFO]
    elif fam == "rphessenberg":
        argv = [head[0], m, n, p, C.c_void_p(ap.ctypes.data) if A == "ok" else None,
                pA if tau == "ok" else None, pZ, nq, nqc, _INFO]
    else:
        raise KeyError(fam)
    return Raw(eng, f"psd_{t}_{fam}", argv, mats=mats, zs=zs, ap=ap, eig=eigs, tau=tauv, si=si, log=log,
               keep=(Sarr, selarr, pA, pZ))


# ------------------------------------------------------------------------------------------------
# argument codes
def arg_cases(fam, cplx):
    """(overrides, code) of entry (fam, cplx): each bad argument alone, then pairs that pin the order of the checks.
    p = 3 by default; a signed S is (1, 0, 1)."""
    sg = (1, 0, 1)
    out = [(dict(ctx=None), -1), (dict(n=0), -2), (dict(p=0), -3), (dict(A=None), -4)]
    if fam == "phessenberg":
        out += [(dict(tau=None), -4)]
    elif fam == "gphessenberg":
        out += [(dict(S=(0, 1, 1)), -5), (dict(A=None, S=(0, 1, 1)), -4)]
    elif fam == "pschur" and not cplx:
        out += [(dict(S=sg), NOTIMPL), (dict(orient=b"X"), -6), (dict(Z=None), -10), (dict(maxitfac=0), -8),
                (dict(eig=None), -10),
                (dict(S=sg, orient=b"X"), NOTIMPL), (dict(orient=b"X", Z=None), -6), (dict(Z=None, maxitfac=0), -10)]
    elif fam == "pschur":
        out += [(dict(orient=b"X"), -6), (dict(Z=None), -10), (dict(maxitfac=0), -8), (dict(eig=None), -10),
                (dict(S=sg, maxitfac=0), -9), (dict(S=(0, 1, 1)), -5), (dict(S=(1, 1, 0), orient=b"L"), -5),
                (dict(orient=b"X", Z=None), -6), (dict(S=sg, Z=None, maxitfac=0), -10),
                (dict(S=(0, 1, 1), maxitfac=0), -9)]
    elif fam == "gpschur":
        out += [(dict(S=sg, orient=b"X"), -6), (dict(S=sg, Z=None), -10), (dict(S=sg, maxitfac=0), -9),
                (dict(S=(0, 1, 1)), -5), (dict(S=(1, 1, 0), orient=b"L"), -5),
                (dict(S=sg, orient=b"X", Z=None), -6), (dict(S=sg, Z=None, maxitfac=0), -10),
                (dict(S=(0, 1, 1), maxitfac=0), -9)]
    elif fam == "pschur_hess" and not cplx:
        out += [(dict(Z=None), -5), (dict(maxitfac=0), -8), (dict(Z=None, maxitfac=0), -5)]
    elif fam in ("pschur_hess", "gpschur_hess"):
        out += [(dict(S=(0, 1, 1)), -5), (dict(S=sg, Z=None), -6), (dict(S=sg, maxitfac=0), -9), (dict(Z=None), -6),
                (dict(maxitfac=0), -9), (dict(S=(0, 1, 1), Z=None), -5), (dict(S=sg, Z=None, maxitfac=0), -6)]
    elif fam == "pschur_dev":
        out += [(dict(orient=b"X"), -5), (dict(maxitfac=0), -8), (dict(Z=None), -9), (dict(eig=None), -10),
                (dict(orient=b"X", maxitfac=0), -5), (dict(maxitfac=0, Z=None), -8), (dict(Z=None, eig=None), -9)]
    elif fam in ("ordschur", "gordschur"):
        g = dict(S=sg) if fam == "gordschur" else {}
        out = [(dict(o, **g), c) for o, c in out]
        out += [(dict(Z=None, **g), -5), (dict(orient=b"X", **g), -6), (dict(select=None, **g), -8),
                (dict(schurindex=0, **g), -7), (dict(schurindex=4, **g), -7), (dict(schurindex=2, **g), -7),
                (dict(orient=b"L", schurindex=2, **g), -7), (dict(select=None, schurindex=2, **g), -8),
                (dict(orient=b"X", select=None, **g), -6)]
        if fam == "gordschur":
            out += [(dict(S=None), -5), (dict(S=(0, 1, 1)), -5), (dict(S=(1, 1, 0), orient=b"L", schurindex=3), -5),
                    (dict(S=None, orient=b"X"), -5), (dict(S=(0, 1, 1), schurindex=2), -7)]
    elif fam == "rphessenberg":
        out += [(dict(m=6), -2), (dict(m=3), -2), (dict(tau=None), -5), (dict(nq=0), -8), (dict(nqc=3), -8),
                (dict(m=6, p=0), -2), (dict(A=None, tau=None), -4), (dict(tau=None, nqc=3), -5)]
    return out


def case_arg_codes(eng, fam, cplx):
    """Every bad argument of entry (fam, cplx): the code of the header, return value == *info, a statistics block that
    comes back all zero, untouched matrices, and the same code from the same call with info = NULL."""
    for over, code in arg_cases(fam, cplx):
        r = build(eng, fam, cplx, **over)
        before = [m.copy() for m in r.matrices()]
        assert r() == code, (fam, cplx, over, r.rc, code)
        assert r.info.value == r.rc, (fam, cplx, over, r.rc, r.info.value)
        if r.has_stats:
            assert bytes(r.st) == bytes(C.sizeof(r.st)), (fam, cplx, over)
        for a, b in zip(before, r.matrices()):
            assert np.array_equal(a, b), (fam, cplx, over)
        r2 = build(eng, fam, cplx, **over)
        assert r2(info=False) == code, (fam, cplx, over, r2.rc)
        assert r2(stats=False) == code and r2.info.value == code


# ------------------------------------------------------------------------------------------------
# plumbing on tiny problems
SIZES = [(n, p) for n in (1, 2, 5, 33) for p in (1, 2, 3)]


def signed_S(p, lr):
    """[1,0] / [1,0,1] in user order for 'R' and their 'L' counterparts (the leftmost entry, S[p-1] for 'L', is true)"""
    S = [True, False, True][:p]
    return S[::-1] if lr == "L" else S


def _copies(mats):
    return [np.array(a, order="F", copy=True) for a in mats]


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b, equal_nan=True), (what, k, np.abs(np.asarray(a) - np.asarray(b)).max())


def _bytes_hess(E, n, p):
    return 2.0 * E * p * (5.0 / 6.0) * float(n) * n * n


def _bytes_formq(E, n, p):
    return 2.0 * E * p * float(n) * n * n / 3.0


def check_stats(r, fam, cplx):
    st = r.st
    if (fam, cplx) in TIMES_COPIES:
        assert st.ms_copy >= 0.0
    else:
        assert st.ms_copy == 0.0
    assert st.ms_total >= st.ms_iter >= 0.0, (st.ms_total, st.ms_iter)


def check_log(r, maxlog):
    """nlog rows reached a large enough sweeplog, and nothing behind them was written"""
    rows = r.log[:3 * maxlog].reshape(-1, 3)
    written = int(np.sum(np.any(rows != SENTINEL, axis=1)))
    assert r.st.nlog <= maxlog
    assert written == r.st.nlog, (written, r.st.nlog)
    assert np.all(rows[:written] != SENTINEL) and np.all(r.log[3 * written:] == SENTINEL)


def _rows(log, k):
    """the first k rows of a sweep log as a sorted list: windows that are under way together log in the order in which
    they finish, so two calls agree in the rows and not in their order"""
    return sorted(map(tuple, np.asarray(log).reshape(-1)[:3 * k].reshape(-1, 3).tolist()))


def check_clipped(c, r, m):
    """call c got room for m rows of the log that call r received in full"""
    import collections

    assert c.st.nlog == r.st.nlog
    assert np.all(c.log[:3 * m] != SENTINEL) and np.all(c.log[3 * m:] == SENTINEL)
    assert not collections.Counter(_rows(c.log, m)) - collections.Counter(_rows(r.log, r.st.nlog))


def case_pschur(eng, cplx, n, p):
    """psd_?_pschur with S null and all-true, both orientations, and psd_?_pschur_dev on the same factors: codes,
    schurindex, the reference's invariants, every slot as eng.pschur returns it, the statistics block and the sweep log;
    then wantZ = 0 with a null Z and wantT = 0."""
    E = 16 if cplx else 8
    A = _factors(cplx, n, p, seed=100 * n + p) if cplx else pt.synth_factors(n, p, seed=100 * n + p)
    maxlog = 2 * 30 * n + n + 16
    for lr in "RL":
        ref = eng.pschur(A, lr)
        pt.pschur_check(A, ref, check_lam=not cplx, real=not cplx)
        if cplx:  # (compare_reigvals pairs conjugates: the unordered match with its bound instead)
            lam = np.linalg.eigvals(pt.product(A, lr == "L"))
            assert pt.match_eigs(lam, ref.values) < 1000 * pt.EPS * abs(lam).max()
        for fam, S in (("pschur", None), ("pschur", [True] * p), ("pschur_dev", None)):
            r = build(eng, fam, cplx, n, p, mats=_copies(A), zs=[np.zeros_like(a) for a in A], S=S, orient=lr.encode(),
                      maxlog=maxlog)
            assert r() == 0 and r.info.value == 0, (fam, lr, r.rc, r.info.value)
            assert r.si.value == (p if lr == "L" else 1)
            _same(r.matrices(), ref.Ts + ref.Z, (fam, lr))
            assert np.array_equal(r.values(), ref.values)
            check_stats(r, fam, cplx)
            assert r.st.bytes_hess == _bytes_hess(E, n, p) and r.st.bytes_formq == _bytes_formq(E, n, p)
            check_log(r, maxlog)
            assert r.st.nlog == ref.stats.nlog
            assert _rows(r.log, r.st.nlog) == _rows(ref.sweeplog, r.st.nlog), (fam, lr, r.log[:3 * r.st.nlog], ref.sweeplog)
            if r.st.nlog >= 2:  # a sweeplog shorter than the log is clipped at 3 * maxlog_user ints
                m = r.st.nlog // 2
                c = build(eng, fam, cplx, n, p, mats=_copies(A), zs=[np.zeros_like(a) for a in A], S=S,
                          orient=lr.encode(), maxlog=m)
                assert c() == 0
                check_clipped(c, r, m)
            # no Schur vectors: Z null; then no T either
            z = build(eng, fam, cplx, n, p, mats=_copies(A), Z=None, wantZ=0, S=S, orient=lr.encode())
            assert z() == 0 and z.info.value == 0
            assert z.st.bytes_formq == 0.0 and z.st.bytes_hess == _bytes_hess(E, n, p)
            scale = max(abs(ref.values).max(), 1e-300)
            assert pt.match_eigs(ref.values, z.values()) < 1000 * pt.EPS * scale
            mz = z.matrices()[:p]
            for j in range(p):
                assert np.all(np.tril(mz[j], -2 if j == r.si.value - 1 and not cplx else -1) == 0)
            t = build(eng, fam, cplx, n, p, mats=_copies(A), Z=None, wantZ=0, wantT=0, S=S, orient=lr.encode())
            assert t() == 0 and t.info.value == 0
            assert pt.match_eigs(ref.values, t.values()) < 1000 * pt.EPS * scale


def _gps(S, r, p, lr):
    m = r.matrices()
    return psd_amd.GeneralizedPeriodicSchur(list(S), m[:p], m[p:2 * p], *r.eig, lr, r.si.value)


def case_signed(eng, cplx, n, p):
    """psd_z_pschur with a signed S and psd_d_gpschur (signed and all-true), both orientations, on well conditioned
    factors (the signature inverts some of them): codes, schurindex, the reference's invariants, every slot as
    eng.pschur(A, lr, S=S) returns it, the statistics block."""
    E = 16 if cplx else 8
    fam = "pschur" if cplx else "gpschur"
    mf = 30 if cplx else 120
    A = pt.bench_factors(n, p, seed=200 * n + p, dtype=np.complex128 if cplx else np.float64)
    check = pt.gpschur_check if cplx else pt.rgpschur_check
    assert p > 1 or not cplx  # (ComplexF64, p = 1: no signed signature, and all-true is psd_z_pschur's plain path)
    for lr in "RL":
        for S in ([signed_S(p, lr)] if p > 1 else []) + ([] if cplx else [[True] * p]):
            ref = eng.pschur(A, lr, S=S)
            check(A, S, ref)
            r = build(eng, fam, cplx, n, p, mats=_copies(A), zs=[np.zeros_like(a) for a in A], S=S, orient=lr.encode(),
                      maxitfac=mf)
            assert r() == 0 and r.info.value == 0, (lr, S, r.rc, r.info.value)
            assert r.si.value == (p if lr == "L" else 1)
            _same(r.matrices(), ref.Ts + ref.Z, (fam, lr, S))
            _same(r.eig, [ref.alpha, ref.beta, ref.alphascale], (fam, lr, S, "eigenvalues"))
            check(A, S, _gps(S, r, p, lr))
            check_stats(r, fam, cplx)
            if not all(S):
                assert r.st.bytes_hess == 2.0 * E * p * float(n) * n * n and r.st.bytes_formq == 0.0
                assert r.st.ms_hess >= r.st.ms_formq >= 0.0
            z = build(eng, fam, cplx, n, p, mats=_copies(A), Z=None, wantZ=0, S=S, orient=lr.encode(), maxitfac=mf)
            assert z() == 0 and z.info.value == 0
            _same(z.eig[1:], [ref.beta, ref.alphascale], (fam, lr, S, "no Z"))
            t = build(eng, fam, cplx, n, p, mats=_copies(A), Z=None, wantZ=0, wantT=0, S=S, orient=lr.encode(),
                      maxitfac=mf)
            assert t() == 0 and t.info.value == 0


def case_hess(eng, fam, cplx, n, p):
    """psd_d_pschur_hess, psd_z_pschur_hess and psd_d_gpschur_hess on Hessenberg-triangular factors with Q = I: S null (where
    there is one), all-true and signed; every slot as the Python mirror of the same entry returns it (these entries keep
    the caller's order), the reference's invariants, the statistics block and the sweep log."""
    dt = np.complex128 if cplx else np.float64
    H = [np.asfortranarray(np.triu(a, -1 if j == 0 else 0)) for j, a in
         enumerate(pt.bench_factors(n, p, seed=300 * n + p, dtype=dt))]
    eye = lambda: [np.asfortranarray(np.eye(n, dtype=dt)) for _ in range(p)]  # noqa: E731
    mf = 120 if fam == "gpschur_hess" else 30
    maxlog = 2 * mf * n + n + 16
    sigs = [None] if fam == "pschur_hess" and not cplx else [None, [True] * p] + ([signed_S(p, "R")] if p > 1 else [])
    if fam == "gpschur_hess":
        sigs = sigs[1:]
    for S in sigs:
        W = _copies(H)
        if fam == "pschur_hess" and not cplx:
            ref = eng.pschur_hess_(W[0], W[1:], Q=eye())
            pt.pschur_check(H, ref)
        else:
            fn = eng.zpschur_hess_ if cplx else eng.gpschur_hess_
            ref = fn(W[0], W[1:], S if S is not None else [True] * p, Q=eye())
            (pt.gpschur_check if cplx else pt.rgpschur_check)(H, ref.S, ref)
        r = build(eng, fam, cplx, n, p, mats=_copies(H), zs=eye(), S=S, maxitfac=mf, maxlog=maxlog)
        assert r() == 0 and r.info.value == 0, (fam, S, r.rc, r.info.value)
        _same(r.matrices(), ref.Ts + ref.Z, (fam, S))
        assert np.array_equal(r.values(), ref.values, equal_nan=True)
        check_stats(r, fam, cplx)
        assert r.st.ms_total == r.st.ms_iter and r.st.bytes_hess == 0.0 and r.st.bytes_formq == 0.0
        z = build(eng, fam, cplx, n, p, mats=_copies(H), Z=None, wantZ=0, S=S, maxitfac=mf)
        assert z() == 0 and z.info.value == 0
        t = build(eng, fam, cplx, n, p, mats=_copies(H), Z=None, wantZ=0, wantT=0, S=S, maxitfac=mf)
        assert t() == 0 and t.info.value == 0
        assert r.st.nlog == ref.stats.nlog
        if cplx and S is not None and not all(S):  # (the complex signed engine hands no sweep log to the caller)
            assert np.all(r.log == SENTINEL)
            continue
        check_log(r, maxlog)
        assert _rows(r.log, r.st.nlog) == _rows(ref.sweeplog, r.st.nlog), (fam, S, r.log[:3 * r.st.nlog], ref.sweeplog)
        if r.st.nlog >= 2:
            m = r.st.nlog // 2
            c = build(eng, fam, cplx, n, p, mats=_copies(H), zs=eye(), S=S, maxitfac=mf, maxlog=m)
            assert c() == 0
            check_clipped(c, r, m)


def case_phessenberg(eng, cplx, n, p):
    """psd_?_phessenberg and psd_?_gphessenberg (S null, all-true, signed; with and without Q)."""
    E = 16 if cplx else 8
    A = _factors(cplx, n, p, seed=400 * n + p)
    ref, tau, _ = eng.phessenberg_(_copies(A))
    r = build(eng, "phessenberg", cplx, n, p, mats=_copies(A))
    assert r() == 0 and r.info.value == 0
    for j in range(p):
        assert np.array_equal(np.triu(r.mats[j], -1 if j == 0 else 0), ref[j])
    assert np.array_equal(r.tau, tau)
    check_stats(r, "phessenberg", cplx)
    assert r.st.bytes_hess == _bytes_hess(E, n, p) and r.st.ms_total == r.st.ms_hess >= 0.0
    B = pt.bench_factors(n, p, seed=410 * n + p, dtype=np.complex128 if cplx else np.float64)
    for S in [None, [True] * p] + ([signed_S(p, "R")] if p > 1 else []):
        Sx = [True] * p if S is None else S
        g = build(eng, "gphessenberg", cplx, n, p, mats=_copies(B), zs=[np.zeros_like(a) for a in B], S=S)
        assert g() == 0 and g.info.value == 0
        pt.sg_hess_check(B, Sx, g.mats, g.zs)
        Hr, Qr = eng.gphessenberg_(_copies(B), Sx)
        _same(g.mats + g.zs, Hr + Qr, ("gphessenberg", S))
        check_stats(g, "gphessenberg", cplx)
        assert g.st.bytes_hess == 2.0 * E * p * float(n) * n * n and g.st.ms_hess >= g.st.ms_formq >= 0.0
        q = build(eng, "gphessenberg", cplx, n, p, mats=_copies(B), Z=None, S=S)
        assert q() == 0 and q.info.value == 0
        _same(q.mats, g.mats, ("gphessenberg without Q", S))


def case_rphessenberg(eng, cplx, n, p):
    """psd_?_rphessenberg with m = n and m = n + 1, Q = I and Q null."""
    dt = np.complex128 if cplx else np.float64
    for m in (n, n + 1):
        Ap = np.asfortranarray(_factors(cplx, m, 1, seed=500 * n + p)[0][:, :n])
        As = _factors(cplx, n, p, seed=510 * n + p)[:p - 1]
        r = build(eng, "rphessenberg", cplx, n, p, m=m, mats=_copies(As),
                  zs=[np.asfortranarray(np.eye(n, dtype=dt)) for _ in range(p)])
        r.ap[...] = Ap
        assert r() == 0 and r.info.value == 0, (m, r.rc, r.info.value)
        pt.rphess_check(Ap, As, r.ap, r.mats, r.zs)
        q = build(eng, "rphessenberg", cplx, n, p, m=m, mats=_copies(As), Z=None)
        q.ap[...] = Ap
        assert q(info=False) == 0
        _same([q.ap] + q.mats, [r.ap] + r.mats, ("rphessenberg without Q", m))


def _clone(ps, S=None):
    Ts, Zs = _copies(ps.Ts), _copies(ps.Z)
    if S is None:
        return psd_amd.PeriodicSchur(Ts, Zs, ps.values.copy(), ps.orientation, ps.schurindex)
    return psd_amd.GeneralizedPeriodicSchur(list(S), Ts, Zs, ps.alpha.copy(), ps.beta.copy(), ps.alphascale.copy(),
                                            ps.orientation, ps.schurindex)


ORD_N = (1, 2, 5, 7, 33)


def _smaller_half(lam):
    """the eigenvalues of smaller modulus (conjugates stay together); all of them for n = 1"""
    return np.abs(lam) <= np.sort(np.abs(lam))[max(len(lam) // 2 - 1, 0)]


def case_ordschur(eng, cplx, n, p):
    """psd_?_ordschur, both orientations (schurindex 1 and p), the smaller half of the spectrum selected: at n = 7 the
    reference's constructed spectrum 4^j, else a generic decomposition (Float64: with conjugate pairs; n = 33 is wider
    than a window).  Codes, swap count and eigenvalues of the oracle, every slot as eng.ordschur_ returns it, the
    invariants; then wantZ = 0 with a null Z."""
    dt = np.complex128 if cplx else np.float64
    A0 = pt.ord_test_factors(n, p, seed=4000 + p, dtype=dt) if n == 7 else pt.bench_factors(n, p, seed=90 + n + p, dtype=dt)
    for lr in "RL":
        A = A0[::-1] if lr == "R" else A0
        ps0 = eng.pschur(A, lr)
        select = _smaller_half(ps0.values)
        ref = eng.ordschur_(_clone(ps0), select)
        po = pt.oracle_ordschur(pt.PSD(ps0.Ts, ps0.Z, ps0.values.copy(), lr, ps0.schurindex), select)
        r = build(eng, "ordschur", cplx, n, p, mats=_copies(ps0.Ts), zs=_copies(ps0.Z), orient=lr.encode(),
                  schurindex=ps0.schurindex, sel=select)
        assert r() == 0 and r.info.value == 0, (lr, r.rc, r.info.value)
        assert po.info == 0 and r.st.nsweeps == po.nswaps
        assert pt.match_eigs(po.values, r.values()) < 1e-9 * abs(po.values).max()
        _same(r.matrices(), ref.Ts + ref.Z, ("ordschur", lr))
        assert np.array_equal(r.values(), ref.values)
        ok, err = pt.checkpsd(psd_amd.PeriodicSchur(r.mats, r.zs, r.values(), lr, ps0.schurindex), A,
                              thresh=100 * np.sqrt(max(n / 32, 1)))
        assert ok, (n, p, lr, err)
        check_stats(r, "ordschur", cplx)
        z = build(eng, "ordschur", cplx, n, p, mats=_copies(ps0.Ts), Z=None, wantZ=0, orient=lr.encode(),
                  schurindex=ps0.schurindex, sel=select)
        assert z() == 0 and z.info.value == 0 and z.st.nsweeps == po.nswaps


def case_gordschur(eng, cplx, n, p):
    """psd_?_gordschur with the signatures [1,0] / [1,0,1] ('R') and their 'L' counterparts (p = 1 has no signed
    signature): at n = 7 the constructed real spectrum (Float64: the promoted path), else a generic signed decomposition
    (Float64: conjugate pairs, the 2x2 branch).  As case_ordschur."""
    dt = np.complex128 if cplx else np.float64
    grow = max(1.0, np.sqrt(n / 32))
    for lr in "RL":
        S = signed_S(p, lr)
        A = pt.gord_test_factors(n, p, S, seed=31 + p, cplx=cplx) if n == 7 else pt.bench_factors(n, p, seed=40 + n + p, dtype=dt)
        ps0 = eng.pschur_(_copies(A), lr, S=S)
        if n == 33 and not cplx:
            assert np.any(ps0.values.imag != 0)
        select = _smaller_half(ps0.values)
        ref = eng.ordschur_(_clone(ps0, S), select)
        r = build(eng, "gordschur", cplx, n, p, mats=_copies(ps0.Ts), zs=_copies(ps0.Z), S=S, orient=lr.encode(),
                  schurindex=ps0.schurindex, sel=select)
        assert r() == 0 and r.info.value == 0, (lr, n, r.rc, r.info.value)
        _same(r.matrices(), ref.Ts + ref.Z, ("gordschur", lr, n))
        _same(r.eig, [ref.alpha, ref.beta, ref.alphascale], ("gordschur", lr, n, "eigenvalues"))
        r.si.value = ps0.schurindex
        if cplx:
            pt.gpschur_check(A, S, _gps(S, r, p, lr), tol=100 * grow, qtol=10 * grow)
        else:
            pt.rgpschur_check(A, S, _gps(S, r, p, lr), tol=(100 if n == 7 else 400) * grow, qtol=10 * grow)
        po = pt.oracle_gordschur(pt.GPSD(S, _copies(ps0.Ts), _copies(ps0.Z), ps0.alpha, ps0.beta, ps0.alphascale,
                                         lr, ps0.schurindex), select)
        assert po.info == 0 and po.nswaps == r.st.nsweeps
        assert pt.match_eigs(po.values, r.values()) < 1e-9 * abs(po.values).max()
        check_stats(r, "gordschur", cplx)
        z = build(eng, "gordschur", cplx, n, p, mats=_copies(ps0.Ts), Z=None, wantZ=0, S=S, orient=lr.encode(),
                  schurindex=ps0.schurindex, sel=select)
        assert z() == 0 and z.info.value == 0 and z.st.nsweeps == po.nswaps


def case_repeat_calls(eng, fam, cplx, signed):
    """A smaller and then a larger (n, p) on one context, then the smaller again: the same bits as a context that has
    seen nothing else (the workspace is reserved, then staged into, per call)."""
    dt = np.complex128 if cplx else np.float64

    def run(e, n, p):
        A = pt.bench_factors(n, p, seed=7 * n + p, dtype=dt)
        r = build(e, fam, cplx, n, p, mats=A, zs=[np.zeros_like(a) for a in A], S=signed_S(p, "L") if signed else None,
                  orient=b"L", maxitfac=120 if fam == "gpschur" else 30)
        assert r() == 0 and r.info.value == 0
        return r.matrices() + list(r.eig)

    shapes = [(5, 2), (33, 3), (5, 2)]
    seen = [run(eng, n, p) for n, p in shapes]
    for (n, p), got in list(zip(shapes, seen))[1:]:
        fresh = psd_amd.Engine(libpath=eng.lib._name)
        try:
            _same(got, run(fresh, n, p), (fam, cplx, n, p))
        finally:
            fresh.close()
