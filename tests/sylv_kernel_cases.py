"""Kernel-level cases of the tiled periodic Sylvester walk (csrc/psd_sylv.h), shared by the CPU tier (serial simulation)
and the GPU tier: ONE launch of psd_syl_update through the diagnostic entry Engine.syl_update (psd_?_syl_update,
include/psd_mi355x.h) at a chosen tile width and anti-diagonal, against a plain numpy reference in extended precision
(np.longdouble / np.clongdouble) written here from the formula in the header comment of psd_sylv.h over the boundaries
the entry returns:
    S:    C_e[I, J] += - sum_{I' after I} A_e[I, I'] Xa[I', J]  + sum_{J' before J} Xb[I, J'] B_e[J', J]
    S^H:  C_e[I, J] += - sum_{I' before I} A_e[I', I]^H Xa[I', J] + sum_{J' after J} Xb[I, J'] B_e[J, J']^H
for the tiles (I, J) of anti-diagonal d, (nI - 1 - I) + J = d (S^H: I + (nJ - 1 - J) = d), A_e = T11 and B_e = T22 of the
factor, Xa and Xb the unknowns that `equation` names (restated from the comment block of psd_bsylv.h).  X is random
everywhere: the kernel only reads tiles the walk would have solved, and what they hold is arbitrary.

Gate, per entry: |got - ref| <= 8 (K + 2) eps (|C| + sum |L| |R|), K the number of terms of both sums, C what the target
starts from (X, or -T12 with from_t12) — the form of krylov_kernel_cases.matvec_bound: any summation order, fused or not;
complex products add 2 sqrt(2) < 4.  Everything outside the tiles of d, and T, must keep its bits, and a second call must
give the bits of the first.  Every check returns the worst err / bound ratio it saw (profiles/sylv/README.md records them).

INPUTS (sylv_cases.INPUTS): d140 and z140, n = 140, p = 2, m = 70.  d140 has 2x2 blocks at rows 15, 31, 47, 63 of T11 and
at the same local rows of T22 and, so that the flip-adjoint 'R' form has the same, at the mirrored rows n - 2 - r: the
boundaries 16, 32, 48 and 64 all move, in both orientations.  TILES: the 32 x 32 sub-block of a workgroup and the 16 x 16
fragment of a wavefront from both sides, 17 for a fragment of one row or column in ComplexF64 too; `coverage` says which
classes of sub-block the sweep must contain."""
import numpy as np

import bsylv_cases as sc
import sylv_cases as yc
from batch_common import cached
from krylov_kernel_cases import EPS, TINY, ld, randn

UB = 32   # PSD_SYL_UB: edge of a workgroup's sub-block
FR = 16   # edge of a wavefront's fragment, and the K step (PSD_SYL_UK)
TILES = (4, 16, 17, 24, 31, 32, 33, 40, 48, 64)
INPUT = {False: "d140", True: "z140"}


def equation(e, p, left, trans):
    """(fa, fb, ua, ub) of equation e: the factor of T11, the factor of T22, the unknown beside T11, the unknown beside
    T22.  S(X)_l = T11_l X_b(l) - X_a(l) T22_l;  S^H(Y)_j = T11_l^H Y_l - Y_l' T22_l'^H with b(l) = j, a(l') = j."""
    if not trans:
        a, b = sc.ab(e, p, left)
        return e, e, b, a
    l = [x for x in range(p) if sc.ab(x, p, left)[1] == e][0]
    l2 = [x for x in range(p) if sc.ab(x, p, left)[0] == e][0]
    return l, l2, l, l2


def tiles_on(d, nI, nJ, trans):
    if trans:
        return [(I, J) for I in range(nI) for J in range(nJ) if I + (nJ - 1 - J) == d]
    return [(I, J) for I in range(nI) for J in range(nJ) if (nI - 1 - I) + J == d]


def kernel_x(name, lr):
    """the random X of an input, read-only"""
    def make():
        ps, _, m = yc.problem(name, lr)
        n, p = ps.Ts[0].shape[0], len(ps.Ts)
        rng = np.random.default_rng(8100 + n + (lr == "R"))
        X = [np.asfortranarray(randn(rng, (m, n - m), np.iscomplexobj(ps.Ts[0]))) for _ in range(p)]
        for x in X:
            x.setflags(write=False)
        return X
    return cached(("sylv-kernel-x", name, lr), make)


def update_sums(ps, m, X, rb, cb, d, trans):
    """per tile of anti-diagonal d and equation: ((I, J), e, rows, columns, the two sums in extended precision, their
    sum of |L| |R|, the number of terms)"""
    p, n = len(ps.Ts), ps.Ts[0].shape[0]
    k = n - m
    T11, _, T22 = sc.parts(ps, m)
    out = []
    for I, J in tiles_on(d, len(rb) - 1, len(cb) - 1, trans):
        i0, i1, j0, j1 = rb[I], rb[I + 1], cb[J], cb[J + 1]
        for e in range(p):
            fa, fb, ua, ub = equation(e, p, ps.orientation == "L", trans)
            if not trans:
                L1, R1 = T11[fa][i0:i1, i1:m], X[ua][i1:m, j0:j1]
                L2, R2 = X[ub][i0:i1, 0:j0], T22[fb][0:j0, j0:j1]
            else:
                L1, R1 = T11[fa][0:i0, i0:i1].conj().T, X[ua][0:i0, j0:j1]
                L2, R2 = X[ub][i0:i1, j1:k], T22[fb][j0:j1, j1:k].conj().T
            acc = -(ld(L1) @ ld(R1)) + ld(L2) @ ld(R2)
            mag = np.abs(L1) @ np.abs(R1) + np.abs(L2) @ np.abs(R2)
            out.append(((I, J), e, slice(i0, i1), slice(j0, j1), acc, mag, L1.shape[1] + L2.shape[1]))
    return out


def check_update(eng, name, lr, tile, trans, records=None):
    """every anti-diagonal d >= 1 of the input at one tile width, with and without from_t12; `records` (a list) receives
    what `coverage` reads.  Returns the worst err / bound ratio."""
    ps, _, m = yc.problem(name, lr)
    p = len(ps.Ts)
    keep = [a.copy() for a in list(ps.Ts) + list(ps.Z)]
    X = kernel_x(name, lr)
    _, T12, _ = sc.parts(ps, m)
    rb, cb = yc.partition(ps, m, tile)
    nI, nJ = len(rb) - 1, len(cb) - 1
    assert nI + nJ - 2 >= 1, (name, tile)
    worst = 0.0
    for d in range(1, nI + nJ - 1):
        sums = update_sums(ps, m, X, rb, cb, d, trans)
        for from_t12 in (False, True):
            Y, g = eng.syl_update(ps, m, X, tile, d, trans=trans, from_t12=from_t12)
            assert (g["rb"], g["cb"]) == (rb, cb), (g, rb, cb)  # the driver's own boundaries are the restated ones
            assert g["nsb"] == -(-(tile + 1) // UB) and (g["nI"], g["nJ"]) == (nI, nJ), g
            assert g["ndtiles"] * p == len(sums), (g, d)
            touched = [np.zeros(x.shape, dtype=bool) for x in X]
            for (I, J), e, ri, cj, acc, mag, K in sums:
                C = -T12[e][ri, cj] if from_t12 else X[e][ri, cj]
                ref = ld(C) + acc
                bound = 8 * (K + 2) * EPS * (np.abs(C) + mag)
                err = np.abs(ld(Y[e][ri, cj]) - ref)
                ratio = float(np.max(err / np.maximum(bound, TINY)))
                assert np.all(err <= bound), (name, lr, tile, d, trans, from_t12, (I, J), e, ratio)
                worst = max(worst, ratio)
                touched[e][ri, cj] = True
            for e in range(p):  # nothing else moves
                assert np.array_equal(Y[e][~touched[e]], X[e][~touched[e]]), (name, lr, tile, d, trans, from_t12, e)
            Y2, _ = eng.syl_update(ps, m, X, tile, d, trans=trans, from_t12=from_t12)
            assert all(np.array_equal(a, b) for a, b in zip(Y, Y2)), (name, lr, tile, d, trans, from_t12)
        if records is not None:
            for (I, J), e, ri, cj, acc, mag, K in sums:
                if e == 0:
                    k1 = (rb[I] if trans else m - rb[I + 1])
                    records.append((g["nsb"], ri.stop - ri.start, cj.stop - cj.start, k1, K - k1))
    assert sc.untouched(ps, keep)
    return worst


def coverage(records):
    """From (nsb, tile rows, tile columns, length of the first sum, of the second) of every tile the sweep updated: the
    classes of 32 x 32 sub-block (mi x nj, cut from the tile as the kernel cuts it: from its first row and column) that
    the sweep must contain, so that a later change of a constant cannot silently empty one."""
    subs, slots = [], []   # (nsb, si, sj, mi, nj) of the sub-blocks that exist; (nsb, empty) of every slot
    for nsb, rows, cols, k1, k2 in records:
        for si in range(nsb):
            for sj in range(nsb):
                mi, nj = min(UB, rows - UB * si), min(UB, cols - UB * sj)
                slots.append((nsb, mi <= 0 or nj <= 0))
                if mi > 0 and nj > 0:
                    subs.append((nsb, si, sj, mi, nj))
    has = lambda f: any(f(*s) for s in subs)  # noqa: E731
    assert has(lambda nsb, si, sj, mi, nj: mi == UB and nj == UB)
    assert has(lambda nsb, si, sj, mi, nj: FR < mi < UB) and has(lambda nsb, si, sj, mi, nj: FR < nj < UB)
    assert has(lambda nsb, si, sj, mi, nj: mi == FR + 1) and has(lambda nsb, si, sj, mi, nj: nj == FR + 1)
    assert has(lambda nsb, si, sj, mi, nj: mi <= FR < nj) and has(lambda nsb, si, sj, mi, nj: nj <= FR < mi)
    assert has(lambda nsb, si, sj, mi, nj: nsb >= 2 and si >= 1 and mi == 1)
    assert has(lambda nsb, si, sj, mi, nj: nsb >= 2 and sj >= 1 and nj == 1)
    assert any(nsb >= 2 and empty for nsb, empty in slots)
    assert has(lambda nsb, si, sj, mi, nj: nsb == 3)
    ks = [(k1, k2) for _, _, _, k1, k2 in records]
    assert any(k1 == 0 and k2 > 0 for k1, k2 in ks) and any(k2 == 0 and k1 > 0 for k1, k2 in ks)
    assert any(0 < k < FR for kk in ks for k in kk) and any(k > FR and k % FR != 0 for kk in ks for k in kk)


def case_update_sweep(eng, cplx, lr, trans):
    """TILES x every anti-diagonal x from_t12 of one input, orientation and form of the operator, and the coverage of
    that sweep"""
    records, worst = [], 0.0
    for tile in TILES:
        w = check_update(eng, INPUT[cplx], lr, tile, trans, records)
        print("update %s %s trans=%d tile %d: worst err / bound = %.3g" % (INPUT[cplx], lr, trans, tile, w))
        worst = max(worst, w)
    coverage(records)
    print("update %s %s trans=%d: worst err / bound = %.3g over %d tiles" % (INPUT[cplx], lr, trans, worst, len(records)))
    return worst


def case_update_arguments(eng):
    import pytest

    for cplx in (False, True):
        ps, _, m = yc.problem(INPUT[cplx], "L")
        X = kernel_x(INPUT[cplx], "L")
        rb, cb = yc.partition(ps, m, 32)
        last = len(rb) + len(cb) - 4  # nI + nJ - 2
        for d in (0, -1, last + 1):  # outside 1 .. nI + nJ - 2: nothing is launched
            with pytest.raises(ValueError, match="argument 11"):
                eng.syl_update(ps, m, X, 32, d)
        eng.syl_update(ps, m, X, 32, last)
        for tile in (1, 0, 129):
            with pytest.raises(ValueError, match="argument 10"):
                eng.syl_update(ps, m, X, tile, 1)
        with pytest.raises(ValueError, match="argument 11"):  # one tile: no anti-diagonal behind the first
            eng.syl_update(ps, m, X, 128, 1)
    ps, _, m = yc.problem("d140", "L")
    with pytest.raises(ValueError, match="argument 8"):  # inside the 2x2 block at rows 15, 16
        eng.syl_update(ps, 16, [np.zeros((16, 124))] * 2, 32, 1)
