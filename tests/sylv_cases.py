"""Engine.psylvester and Engine.subspacecond (psd_?_psylv[_dev], psd_?_subcond[_dev], csrc/psd_sylv.h): the periodic
Sylvester solve and the periodic form of xTRSEN's S and SEP for ONE form of any order, by the tiled walk — the cases shared
by the simulated tier (test_hostsim_psylvester.py) and the device tier (test_gpu_psylvester.py).

The reference is that of bsylv_cases.py: the dense Kronecker matrix (kron_matrix), numpy.linalg.solve for X, the exact
||K^-1||_1 and the restated xLACN2 (lacn2).  Gates: relation ratios <= evec_cases.GATE; forward errors of X, s and sep
<= n eps kappa, kappa = max_l(||T11_l||_F + ||T22_l||_F) / sigma_min(K); the adjoint identity to n eps.

INPUTS: every one has kappa <= 1e6 and the restated estimator within a factor 3 of the norm (test_reference_inputs
checks both on the CPU).  The product diagonals come in groups, so that the split separates two of them:
  d20    Float64 n = 20, p = 3, m = 10: 10 in [1, 1.5], 10 in [3, 3.5]; 2x2 blocks at rows 3, 7, 13 ('R': 15, 11, 5) —
         with tile width 4 the boundaries 4 and 8 of T11 and the local boundary 4 of T22 would cut one and move
  d130a  Float64 n = 130, p = 2: 3 in [1, 1.5], 127 in [3, 3.5], a block at row 64; 'L' m = 3, 'R' (the flip) m = 127
  d130b  the same seed and block: 127 in [1, 1.5], 3 in [8, 9]; 'L' m = 127, 'R' m = 3
  z20    ComplexF64 n = 20, p = 3, m = 10: the moduli of d20 times the phases of bevec_cases.zdiag
  z130   ComplexF64 n = 130, p = 2, m = 3: 3 in [1, 1.5], 124 in [2.1, 2.4], 3 in [3, 3.5]
The n = 130 inputs are above the cap of the batch entries (128): psylvester_batch raises NotImplementedPSD on them.
Wide tiles (case_wide_tiles: the update kernel beyond one 16 x 16 fragment, `partition` restates the driver's boundaries):
  d100   Float64 n = 100, p = 1, m = 50: 50 in [1, 1.5], 50 in [3, 3.5]; 2x2 blocks at rows 15, 31, 47 of T11 and at the
         same local rows of T22 (65, 81, 97).  In 'L' the tiles are 17 | 16 | 16 | 1 wide at tile width 16 (three moved
         boundaries: the second fragment row and column of a workgroup hold one row or column), 33 | 17 at 32 (a second
         sub-block of one row, nsb = 2) and 49 | 1 at 48 (sub-blocks 32 + 17); 24 and 40 cut fragments inside
  z100   ComplexF64, the same order, split and groups: no boundary moves, the widths 16 ... 48 are full fragments and
         sub-blocks (48 = 32 + 16, 40 = 32 + 8, 24 = 16 + 8) with the ragged rest of 50
  d133   Float64 n = 133, p = 2: 130 in [1, 1.5], 3 in [8, 9], a block at row 127; 'L' m = 130, 'R' m = 3.  At tile width
         128 the boundary 128 of 'L' moves: tiles 129 | 1, above the cap of the batch kernel, nsb = 5, one update
  the order-70 problems of bsylv_cases.PROBLEMS at tile widths 17, 24 and 32: 33 = 17 + 16 = 24 + 9 = 32 + 1 rows,
         37 = 17 + 17 + 3 = 24 + 13 = 32 + 5 columns (d: the blocks at rows 10 and 40 move no boundary)
Kernel cases (sylv_kernel_cases.py: one update launch against an extended-precision reference):
  d140   Float64 n = 140, p = 2, m = 70: 2x2 blocks at rows 15, 31, 47, 63 of T11, the same local rows of T22, and at the
         mirrored rows n - 2 - r, so that 'L' and the flip-adjoint 'R' both move the boundaries 16, 32, 48 and 64
  z140   ComplexF64, the same order and split"""
import numpy as np
import pytest

import bevec_cases as bc
import bsylv_cases as sc
import evec_cases as vc
import lbevec_cases as lc
import psd_amd
from batch_common import cached

EPS = sc.EPS
GATE = vc.GATE
KNOBS = ("PSD_SYL_TILE", "PSD_BSYL_NMAX", "PSD_BATCH_GROUP")
LIB_TILE = 16  # PSD_SYL_TILE of csrc/psd_sylv.h


def _groups(*spec):
    return np.concatenate([np.linspace(lo, hi, cnt) for cnt, lo, hi in spec])


def _ddiag(d, p):
    return [d ** (1.0 / p) for _ in range(p)]


def _zdiag(d, p, seed):
    rs = np.random.RandomState(1000 + seed)  # (the phases rule of bevec_cases.zdiag)
    return [d ** (1.0 / p) * np.exp(1j * rs.uniform(-np.pi, np.pi, len(d))) for _ in range(p)]


TWO20 = ((10, 1.0, 1.5), (10, 3.0, 3.5))
_PAIRS140 = (15, 31, 47, 63, 85, 101, 117, 133)
# name: (ComplexF64, n, p, seed, pair rows, the groups of the product diagonals, m in 'L', m in 'R')
INPUTS = {
    "d20": (False, 20, 3, 23, (3, 7, 13), TWO20, 10, 10),
    "d130a": (False, 130, 2, 7, (64,), ((3, 1.0, 1.5), (127, 3.0, 3.5)), 3, 127),
    "d130b": (False, 130, 2, 7, (64,), ((127, 1.0, 1.5), (3, 8.0, 9.0)), 127, 3),
    "z20": (True, 20, 3, 5, (), TWO20, 10, 10),
    "z130": (True, 130, 2, 9, (), ((3, 1.0, 1.5), (124, 2.1, 2.4), (3, 3.0, 3.5)), 3, 3),
    # residual only (the Kronecker matrix would have order 12800): GPU tier
    "d160": (False, 160, 2, 11, (30, 77, 120), ((80, 1.0, 1.5), (80, 3.0, 3.5)), 80, 80),
    "z160": (True, 160, 2, 11, (), ((80, 1.0, 1.5), (80, 3.0, 3.5)), 80, 80),
    # wide tiles
    "d100": (False, 100, 1, 17, (15, 31, 47, 65, 81, 97), ((50, 1.0, 1.5), (50, 3.0, 3.5)), 50, 50),
    "z100": (True, 100, 1, 13, (), ((50, 1.0, 1.5), (50, 3.0, 3.5)), 50, 50),
    "d133": (False, 133, 2, 7, (127,), ((130, 1.0, 1.5), (3, 8.0, 9.0)), 130, 3),
    # one update launch (sylv_kernel_cases.py): no Kronecker reference
    "d140": (False, 140, 2, 19, _PAIRS140 + tuple(sorted(138 - r for r in _PAIRS140)), ((70, 1.0, 1.5), (70, 3.0, 3.5)), 70, 70),
    "z140": (True, 140, 2, 19, (), ((70, 1.0, 1.5), (70, 3.0, 3.5)), 70, 70),
}
SMALL = ("d20", "z20")
BIG = ("d130a", "d130b", "z130")
RESID = ("d160", "z160")
WIDE = ("d100", "z100", "d133")
WIDE_TILES = {"d100": (16, 24, 32, 40, 48), "z100": (16, 24, 32, 40, 48), "d133": (128,)}
WIDE_BATCH = tuple(sc.IDS.index(i) for i in ("d_n70_p2_m33", "z_n70_p2_m33"))  # at the tile widths WIDE_BATCH_TILES
WIDE_BATCH_TILES = (17, 24, 32)
WIDTHS_L = {("d100", 16): [17, 16, 16, 1], ("d100", 32): [33, 17], ("d100", 48): [49, 1], ("d133", 128): [129, 1]}


def problem(name, lr):
    """(ps, As, m) of an input in orientation lr, read-only"""
    def make():
        cplx, n, p, seed, pairs, groups, mL, mR = INPUTS[name]
        d = _groups(*groups)
        assert len(d) == n
        pr = bc.zform(n, p, seed, diag=_zdiag(d, p, seed)) if cplx else bc.plain_form(n, p, seed, pairs, diag=_ddiag(d, p))
        if lr == "R":
            pr = lc.as_right(pr)
        ps, As = pr
        m = mL if lr == "L" else mR
        for a in list(ps.Ts) + list(ps.Z) + list(As):
            a.setflags(write=False)
        assert ps.orientation == lr and ps.Ts[ps.schurindex - 1][m, m - 1] == 0  # the split cuts no block
        return ps, As, m
    return cached(("sylv", name, lr), make)


def reference_of(ps, m):
    p, n = len(ps.Ts), ps.Ts[0].shape[0]
    T11, T12, T22 = sc.parts(ps, m)
    K = sc.kron_matrix(ps, m)
    Kinv = np.linalg.inv(K)
    smin = 1.0 / np.linalg.norm(Kinv, 2)
    kappa = max(np.linalg.norm(a) + np.linalg.norm(b) for a, b in zip(T11, T22)) / smin
    X = sc.unstack(np.linalg.solve(K, sc.stack([-c for c in T12])), p, m, n - m)
    s = np.array([1.0 / np.sqrt(1.0 + np.linalg.norm(x) ** 2) for x in X])
    est, solves, it = sc.lacn2(Kinv, np.iscomplexobj(K))
    return dict(K=K, Kinv=Kinv, kappa=kappa, X=X, s=s, norm1=np.linalg.norm(Kinv, 1), est=est, solves=solves, it=it)


def reference(name, lr):
    """K, K^-1, kappa, X of C = -T12, s, ||K^-1||_1 and the restated estimator of an input: computed once"""
    return cached(("sylv-ref", name, lr), lambda: reference_of(*problem(name, lr)[::2]))


def case_reference_inputs(name, lr):
    ref = reference(name, lr)
    print("input", name, lr, "kappa %.3e est / norm %.3f" % (ref["kappa"], ref["est"] / ref["norm1"]))
    assert ref["kappa"] <= sc.KAPPA_MAX, ref["kappa"]
    assert 1.0 / 3.0 <= ref["est"] / ref["norm1"] <= 1.0 + 1e-12, ref["est"] / ref["norm1"]
    assert ref["solves"] <= 11


# ------------------------------------------------------------------------------------------------
# the checks of one form
def check_solves(eng, tag, ps, m, ref, seed, adjoint_gate):
    """X of C = -T12 against the Kronecker solve, the relation ratios of both forms of the operator with -T12 and with
    random right-hand sides, and the adjoint identity"""
    p, n = len(ps.Ts), ps.Ts[0].shape[0]
    keep = [a.copy() for a in list(ps.Ts) + list(ps.Z)]
    _, T12, _ = sc.parts(ps, m)
    K = ref["K"]
    KH = K.conj().T
    bound = n * EPS * ref["kappa"]
    X = eng.psylvester(ps, m)
    assert len(X) == p and all(x.shape == (m, n - m) for x in X)
    ex = np.linalg.norm(sc.stack(X) - sc.stack(ref["X"])) / np.linalg.norm(sc.stack(ref["X"]))
    r = sc.residual_ratio(ps, m, X, [-c for c in T12])
    print(tag, "X error %.3e bound %.3e residual %.3e" % (ex, bound, r), eng.psylvester_stats.asdict())
    assert ex <= bound, (ex, bound)
    assert r <= GATE, r
    Cs = sc.random_blocks(ps, m, seed)
    keepC = [c.copy() for c in Cs]
    r = sc.residual_ratio(ps, m, eng.psylvester(ps, m, C=Cs), Cs)
    Y = eng.psylvester(ps, m, C=Cs, trans=True)
    rt = sc.residual_ratio(ps, m, Y, Cs, Kop=KH)
    ey = np.linalg.norm(sc.stack(Y) - np.linalg.solve(KH, sc.stack(Cs))) / np.linalg.norm(sc.stack(Y))
    print(tag, "random: residual %.3e transposed %.3e, its X error %.3e" % (r, rt, ey))
    assert r <= GATE and rt <= GATE, (r, rt)
    assert ey <= bound, (ey, bound)
    # <Y, S X> = <S^H Y, X>: S X from numpy, Y recovered by the entry from S^H Y
    X0, Y0 = sc.random_blocks(ps, m, seed + 1), sc.random_blocks(ps, m, seed + 2)
    SHY = sc.unstack(KH @ sc.stack(Y0), p, m, n - m)
    Y1 = eng.psylvester(ps, m, C=SHY, trans=True)
    lhs, rhs = np.vdot(sc.stack(Y1), K @ sc.stack(X0)), np.vdot(sc.stack(SHY), sc.stack(X0))
    gap = abs(lhs - rhs) / (np.linalg.norm(sc.stack(X0)) * np.linalg.norm(sc.stack(Y1)) * np.linalg.norm(K))
    print(tag, "adjoint identity %.3e bound %.3e" % (gap, adjoint_gate))
    assert gap <= adjoint_gate, gap
    assert sc.untouched(ps, keep) and all(np.array_equal(a, b) for a, b in zip(Cs, keepC))


def check_cond(eng, tag, ps, m, ref):
    """s, X and sep against the reference (the gates of bsylv_cases.case_reference)"""
    n = ps.Ts[0].shape[0]
    bound = n * EPS * ref["kappa"]
    s, sep, X = eng.subspacecond(ps, m, want_x=True)
    st = eng.subspacecond_stats
    es = np.abs(s - ref["s"]) / ref["s"]
    ex = np.linalg.norm(sc.stack(X) - sc.stack(ref["X"])) / np.linalg.norm(sc.stack(ref["X"]))
    est = 1.0 / sep
    print(tag, "kappa %.3e s %.3e X %.3e bound %.3e est / norm %.4f solves %d (numpy %d) iterations %d (numpy %d)"
          % (ref["kappa"], es.max(), ex, bound, est / ref["norm1"], st.nest_solves, ref["solves"], st.nest_iter, ref["it"]),
          st.asdict())
    assert np.all(es <= bound), (es.max(), bound)
    assert ex <= bound, (ex, bound)
    assert est <= ref["norm1"] * (1.0 + bound), (est, ref["norm1"])
    assert est >= ref["norm1"] / 3.0, (est, ref["norm1"])
    if st.nest_solves == ref["solves"] and st.nest_iter == ref["it"]:  # the same path
        assert abs(est - ref["est"]) <= bound * ref["est"], (est, ref["est"])
    s2, sep2 = eng.subspacecond(ps, m)
    assert np.array_equal(s, s2) and sep == sep2


# ------------------------------------------------------------------------------------------------
# 1. small tiles: several anti-diagonals, boundaries that move, ragged fragments
def case_small_tiles(eng, name, lr, tile):
    ps, As, m = problem(name, lr)
    ref = reference(name, lr)
    check_solves(eng, "tile %d %s %s" % (tile, name, lr), ps, m, ref, 700, ps.Ts[0].shape[0] * EPS)
    st = eng.psylvester_stats
    assert st.tile == tile and st.ndiag > 1 and st.nupdate == st.ndiag - 1 and st.nsolve == st.ndiag
    if tile == 4 and name == "d20":  # the boundaries 4 and 8 of T11 and the local 4 of T22 have moved
        assert st.ntiles == 9
    check_cond(eng, "tile %d %s %s" % (tile, name, lr), ps, m, ref)


def bounds_of(length, t, sub, off):
    """The driver's partition restated: boundaries at multiples of t; one that would cut a 2x2 block (sub[off + x - 1]
    != 0) moves to x + 1, and is dropped if that is the end."""
    b = [0]
    for x in range(t, length, t):
        y = x + 1 if sub is not None and sub[off + x - 1] != 0 else x
        if y < length:
            b.append(y)
    return b + [length]


def partition(ps, m, t):
    """(rb, cb) of the form at tile width t: the rows of T11 and the local columns of T22, cut along the sub-diagonal of
    the quasi-triangular factor"""
    Tq = ps.Ts[ps.schurindex - 1]
    sub = None if np.iscomplexobj(Tq) else np.diag(Tq, -1)
    return bounds_of(m, t, sub, 0), bounds_of(Tq.shape[0] - m, t, sub, m)


def case_wide_tiles(eng, key, lr, tile):
    """eng: PSD_SYL_TILE=tile.  key: an input of WIDE, or an index of bsylv_cases.PROBLEMS (gates and seeds as
    case_small_tiles and case_batch_problems have them).  The update kernel runs with tiles wider than one fragment; the
    number of tiles is that of the restated partition."""
    if isinstance(key, str):
        (ps, As, m), ref, tag, seed, gate = problem(key, lr), reference(key, lr), key, 700, None
    else:
        (ps, As, m), ref, tag, seed, gate = sc.problem(key, lr), sc.reference(key, lr), sc.IDS[key], 800 + key, GATE
    tag = "tile %d %s %s" % (tile, tag, lr)
    rb, cb = partition(ps, m, tile)
    widths = [b - a for a, b in zip(rb, rb[1:])]
    print(tag, "tile rows", widths, "tile columns", [b - a for a, b in zip(cb, cb[1:])])
    if lr == "L" and (key, tile) in WIDTHS_L:
        assert widths == WIDTHS_L[(key, tile)], widths
    check_solves(eng, tag, ps, m, ref, seed, ps.Ts[0].shape[0] * EPS if gate is None else gate)
    check_cond(eng, tag, ps, m, ref)
    for st in (eng.psylvester_stats, eng.subspacecond_stats):
        assert st.tile == tile and st.ntiles == (len(rb) - 1) * (len(cb) - 1), (st.asdict(), rb, cb)
    st = eng.psylvester_stats
    assert st.nupdate == st.ndiag - 1 > 0 and st.nsolve == st.ndiag, st.asdict()
    if key == "d133":
        assert st.ntiles == 2 and st.nupdate == 1, st.asdict()


def case_batch_problems(eng, k, lr):
    """bsylv_cases.PROBLEMS through the single entries, with the gates they have in bsylv_cases (the adjoint identity
    there: GATE; n eps at n = 2 is two units of the last place of one inner product)"""
    ps, As, m = sc.problem(k, lr)
    ref = sc.reference(k, lr)
    check_solves(eng, "tile 4 %s %s" % (sc.IDS[k], lr), ps, m, ref, 800 + k, GATE)
    check_cond(eng, "tile 4 %s %s" % (sc.IDS[k], lr), ps, m, ref)


# 2. above the cap of the batch entries, at the default tile
def case_above_cap(eng, name, lr):
    ps, As, m = problem(name, lr)
    with pytest.raises(psd_amd.NotImplementedPSD):  # (the batch entries keep their cap)
        eng.psylvester_batch([ps], m)
    ref = reference(name, lr)
    check_cond(eng, "default %s %s" % (name, lr), ps, m, ref)
    assert eng.subspacecond_stats.tile == LIB_TILE
    _, T12, _ = sc.parts(ps, m)
    X = eng.psylvester(ps, m)
    r = sc.residual_ratio(ps, m, X, [-c for c in T12])
    assert r <= GATE, r


# 3. one tile is the batch kernel
def one_tile_problems():
    return ([("batch", k, lr) for k in range(len(sc.PROBLEMS)) for lr in "LR"]
            + [("input", name, lr) for name in SMALL for lr in "LR"])


def case_one_tile(eng, exact):
    """eng: PSD_SYL_TILE=128.  exact: bit for bit (the simulation); otherwise within 1e-12 of the scale, the project's
    allowance for two instantiations of one body, and the number of entries that differ is printed"""
    differ = total = 0
    for kind, key, lr in one_tile_problems():
        ps, As, m = sc.problem(key, lr) if kind == "batch" else problem(key, lr)
        Cs = sc.random_blocks(ps, m, 900)
        pairs = []
        for trans in (False, True):
            pairs += list(zip(eng.psylvester(ps, m, C=Cs, trans=trans), eng.psylvester_batch([ps], m, C=[Cs], trans=trans)[0]))
            assert eng.psylvester_stats.ntiles == 1 and eng.psylvester_stats.nupdate == 0
        s, sep, X = eng.subspacecond(ps, m, want_x=True)
        sb, sepb, Xb = eng.subspacecond_batch([ps], m, want_x=True)
        pairs += list(zip(X, Xb[0])) + [(s, sb[0]), (np.array([sep]), np.array([sepb[0]]))]
        for a, b in pairs:
            differ += int(np.sum(a != b))
            total += a.size
            if exact:
                assert np.array_equal(a, b), (kind, key, lr)
            else:
                assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b).max()), (kind, key, lr, np.abs(a - b).max())
    print("one tile against the batch kernel: %d of %d entries differ" % (differ, total))


# 4. repeatability
def case_repeat(eng, name, lr):
    ps, As, m = problem(name, lr)
    a = eng.subspacecond(ps, m, want_x=True)
    b = eng.subspacecond(ps, m, want_x=True)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    Cs = sc.random_blocks(ps, m, 950)
    for trans in (False, True):
        x1, x2 = eng.psylvester(ps, m, C=Cs, trans=trans), eng.psylvester(ps, m, C=Cs, trans=trans)
        assert all(np.array_equal(x, y) for x, y in zip(x1, x2))
    return ps, m, a, Cs


def case_device_equals_host(eng, name, lr):
    import torch

    ps, m, host, Cs = case_repeat(eng, name, lr)
    T = torch.from_numpy(np.array([np.array(t) for t in ps.Ts])).cuda()
    keep = T.clone()
    s, sep, X = eng.subspacecond_dev(T, m, want_x=True, lr=lr, schurindex=ps.schurindex)
    assert X.is_cuda and torch.equal(T, keep)
    assert np.array_equal(s, host[0]) and sep == host[1]
    assert all(np.array_equal(X[l].cpu().numpy(), host[2][l]) for l in range(len(ps.Ts)))
    assert torch.equal(eng.psylvester_dev(T, m, lr=lr, schurindex=ps.schurindex), X)
    Cd = torch.from_numpy(np.array(Cs)).cuda()
    Y = eng.psylvester_dev(T, m, C=Cd, trans=True, lr=lr, schurindex=ps.schurindex)
    Y0 = eng.psylvester(ps, m, C=Cs, trans=True)
    assert all(np.array_equal(Y[l].cpu().numpy(), Y0[l]) for l in range(len(ps.Ts)))
    assert torch.equal(Cd, torch.from_numpy(np.array(Cs)).cuda())


# 5. residual only
def case_residual_only(eng, name, lr):
    ps, As, m = problem(name, lr)
    p, n = len(ps.Ts), ps.Ts[0].shape[0]
    _, T12, T22 = sc.parts(ps, m)
    s, sep, X = eng.subspacecond(ps, m, want_x=True)
    r = sc.residual_ratio(ps, m, X, [-c for c in T12])
    worst = 0.0  # T_l [X_b; I] = [X_a; I] T22_l
    Y = [np.vstack([X[l], np.eye(n - m)]) for l in range(p)]
    for l in range(p):
        a, b = sc.ab(l, p, lr == "L")
        worst = max(worst, np.linalg.norm(ps.Ts[l] @ Y[b] - Y[a] @ T22[l])
                    / (np.linalg.norm(ps.Ts[l]) * max(np.linalg.norm(Y[a]), np.linalg.norm(Y[b]))))
    s0 = np.array([1.0 / np.sqrt(1.0 + np.linalg.norm(x) ** 2) for x in X])
    print("residual only", name, lr, "S(X) + T12 %.3e block diagonalisation %.3e s %.3e sep %.3e"
          % (r, worst, np.abs(s - s0).max() / s0.min(), sep), eng.subspacecond_stats.asdict())
    assert r <= GATE and worst <= GATE, (r, worst)
    assert np.all(np.abs(s - s0) <= 4 * EPS * s0), np.abs(s / s0 - 1).max()
    assert 0 < sep < np.inf


# 6. a singular form: the equal products in the tile the walk reaches last
def singular_problem(name):
    def make():
        ps, _, m = problem(name, "L")
        Ts = [t.copy(order="F") for t in ps.Ts]
        for t in Ts:
            t[18, 18] = t[1, 1]  # (row 1: the first block row of T11; row 18: the last block column of T22)
        return psd_amd.PeriodicSchur(Ts, ps.Z, np.array(ps.values), ps.orientation, ps.schurindex), m
    return cached(("sylv-singular", name), make)


def case_singular(eng, name):
    """eng: PSD_SYL_TILE=4"""
    ps, m = singular_problem(name)
    p = len(ps.Ts)
    code = []
    s, sep, X = eng.subspacecond(ps, m, want_x=True, info_out=code)
    assert code == [3000] and eng.subspacecond_stats.nsingular == 1 and eng.subspacecond_stats.ndiag > 1
    assert np.all(s == 0.0) and sep == 0.0 and len(X) == p and all(np.isnan(x).all() for x in X)
    code = []
    X = eng.psylvester(ps, m, info_out=code)
    assert code == [3000] and all(np.isnan(x).all() for x in X)
    code = []
    X = eng.psylvester(ps, m, C=sc.random_blocks(ps, m, 5), trans=True, info_out=code)
    assert code == [3000] and all(np.isnan(x).all() for x in X)
    with pytest.raises(psd_amd.SingularException):
        eng.subspacecond(ps, m)
    with pytest.raises(psd_amd.SingularException):
        eng.psylvester(ps, m)
    good, _, _ = problem(name, "L")  # the engine goes on
    s, sep = eng.subspacecond(good, m)
    assert np.all(s > 0) and sep > 0


# 7. arguments
def case_arguments(eng, make_engine):
    ps, As, m = problem("d20", "L")
    zs = problem("z20", "L")[0]
    n, p = 20, 3
    for call in (eng.subspacecond, eng.psylvester):
        with pytest.raises(ValueError, match="argument 8"):  # inside the 2 x 2 block at rows 3, 4
            call(ps, 4)
        for bad in (-1, n + 1):
            with pytest.raises(ValueError, match="argument 8"):
                call(ps, bad)
        with pytest.raises(psd_amd.DimensionMismatch):
            call(ps, 2.5)
        with pytest.raises(psd_amd.DimensionMismatch):
            call(ps, [10])
        g = psd_amd.GeneralizedPeriodicSchur([True, False, True], ps.Ts, ps.Z, np.array(ps.values), np.ones(n),
                                             np.zeros(n, dtype=np.int32), "L", p)
        with pytest.raises(psd_amd.NotImplementedPSD):
            call(g, m)
    for form in (ps, zs):  # the trivial splits: no launch
        for mm in (0, n):
            s, sep, X = eng.subspacecond(form, mm, want_x=True)
            st = eng.subspacecond_stats
            assert np.all(s == 1.0) and sep == np.inf and all(x.shape == (mm, n - mm) for x in X)
            assert st.nsolve == 0 and st.nupdate == 0 and st.nnorms == 0 and st.nest_steps == 0
            X = eng.psylvester(form, mm)
            assert all(x.shape == (mm, n - mm) for x in X) and eng.psylvester_stats.nsolve == 0
    with pytest.raises(psd_amd.DimensionMismatch):  # right-hand sides of the wrong shape
        eng.psylvester(ps, m, C=[np.zeros((m, m + 1))] * p)
    with pytest.raises(psd_amd.DimensionMismatch):
        eng.psylvester(ps, m, C=[np.zeros((m, n - m))] * (p - 1))
    with pytest.raises(TypeError):
        eng.psylvester(ps, m, C=[np.zeros((m, n - m), dtype=complex)] * p)
    # the periods whose small-block scratch does not fit the LDS
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.subspacecond(bc.zform(4, 20, 5)[0], 2)
    with pytest.raises(psd_amd.NotImplementedPSD):
        eng.psylvester(bc.plain_form(4, 137, 5)[0], 2)
    s, sep = eng.subspacecond(bc.zform(4, 19, 5)[0], 2)
    assert np.all(s > 0) and sep > 0
    sharded = make_engine({})
    sharded.set_shard(0, 2)
    for call in (sharded.subspacecond, sharded.psylvester):
        with pytest.raises(psd_amd.NotImplementedPSD):
            call(ps, m)
    # PSD_SYL_TILE out of range: the default
    for bad in ("1", "129", "0", "-4", "x"):
        e = make_engine({"PSD_SYL_TILE": bad})
        e.psylvester(ps, m)
        assert e.psylvester_stats.tile == LIB_TILE, bad
    for good in (2, 128):
        e = make_engine({"PSD_SYL_TILE": str(good)})
        e.psylvester(ps, m)
        assert e.psylvester_stats.tile == good
    # the cap of the batch entries does not bind the single ones
    low = make_engine({"PSD_BSYL_NMAX": "6"})
    with pytest.raises(psd_amd.NotImplementedPSD):
        low.psylvester_batch([ps], m)
    assert all(np.isfinite(x).all() for x in low.psylvester(ps, m))
