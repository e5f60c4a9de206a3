"""CPU tier: the Python contract of the whole batch family in one place, on the TEST-ONLY serial simulation of the device
code (tests/hostsim) — which exception each wrong input raises and with which text, what an empty batch returns and
whether it touches `infos_out`, which class each entry returns, which forms overwrite the caller's arrays, and that
`values` is alpha / beta * 2^alphascale bit for bit.  The numerics of the entries are the business of the
test_hostsim_*_batch.py files; the shapes here are the smallest with more than one problem and more than one factor."""
import copy

import numpy as np
import pytest

import psd_amd
from psd_amd import DimensionMismatch, GeneralizedPeriodicSchur, NotImplementedPSD, PeriodicSchur

NB, N, P = 2, 4, 2
SIGNED = [True, False]


def _factors(nb, n, p, cplx, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nb):
        A = [rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0.0) for _ in range(p)]
        out.append([np.asfortranarray(a if cplx else a.real) for a in A])
    return out


def work(probs):
    return [[np.array(a, order="F", copy=True) for a in A] for A in probs]


def hess(probs):
    """(H1, Hs) problems: the factors cut to Hessenberg-triangular form"""
    return [(np.asfortranarray(np.triu(A[0], -1)), [np.asfortranarray(np.triu(a)) for a in A[1:]]) for A in probs]


def clone(ps):
    cp = copy.copy(ps)
    cp.Ts = [np.array(t, order="F", copy=True) for t in ps.Ts]
    cp.Z = [np.array(z, order="F", copy=True) for z in ps.Z]
    cp.values = np.array(ps.values, copy=True)
    return cp


def altered(ps, **kw):
    cp = clone(ps)
    for k, v in kw.items():
        setattr(cp, k, v)
    return cp


class Data:
    pass


@pytest.fixture(scope="module")
def D(sim_engine):
    """The inputs of every table, computed once: factors, their decompositions, and odd ones out."""
    eng, d = sim_engine, Data()
    d.eng = eng
    d.rA, d.zA = _factors(NB, N, P, False, 1), _factors(NB, N, P, True, 2)
    d.rA5, d.zA5 = _factors(1, N + 1, P, False, 3), _factors(1, N + 1, P, True, 4)  # another order
    d.rA3, d.zA3 = _factors(1, N, P + 1, False, 5), _factors(1, N, P + 1, True, 6)  # another period
    d.rPS, d.zPS = eng.pschur_batch(d.rA), eng.zpschur_batch(d.zA)
    d.gPS = eng.zgpschur_batch(d.zA, SIGNED)  # signed
    d.tPS = eng.zgpschur_batch(d.zA, [True] * P)  # GeneralizedPeriodicSchur, all true
    d.rPS5, d.zPS5 = eng.pschur_batch(d.rA5), eng.zpschur_batch(d.zA5)
    d.rPS3, d.zPS3 = eng.pschur_batch(d.rA3), eng.zpschur_batch(d.zA3)
    d.rPSL, d.zPSL = eng.pschur_batch(d.rA, "L"), eng.zpschur_batch(d.zA, "L")  # orientation L, schurindex p
    d.sel = [False] * (N - 1) + [True]
    return d


def _cpu(cplx, nb=NB):
    import torch

    return torch.zeros((nb, P, 3, 3), dtype=torch.complex128 if cplx else torch.float64)


EQ2 = "equal order and period"
EQ4 = "equal order, period, orientation and schurindex"
R_ONLY = "pschur_batch: Float64 only (ComplexF64 problems: zpschur_batch)"
Z_ONLY = "zpschur_batch: ComplexF64 only (use pschur_batch for Float64 problems)"
NEEDS_F64 = "needs writable Fortran-ordered float64 matrices"
SEL_ORD = "select must be [nb][n] flags or one row of n: one entry per eigenvalue"
NOZ = "eigvecs requires Schur vectors in the PSD"

# (id, call on (eng, D), exception, fragment of its text)
ERRORS = [
    # ---- wrong dtype family
    ("dtype-pschur_batch_", lambda e, d: e.pschur_batch_(work(d.zA)), NotImplementedPSD, R_ONLY),
    ("dtype-pschur_batch", lambda e, d: e.pschur_batch(d.zA), NotImplementedPSD, R_ONLY),
    ("dtype-phessenberg_batch_", lambda e, d: e.phessenberg_batch_(work(d.zA)), NotImplementedPSD, R_ONLY),
    ("dtype-pschur_hess_batch_", lambda e, d: e.pschur_hess_batch_(hess(d.zA)), TypeError, NEEDS_F64),
    ("dtype-zpschur_batch_", lambda e, d: e.zpschur_batch_(work(d.rA)), TypeError, Z_ONLY),
    ("dtype-zpschur_batch", lambda e, d: e.zpschur_batch(d.rA), TypeError, Z_ONLY),
    ("dtype-zphessenberg_batch_", lambda e, d: e.zphessenberg_batch_(work(d.rA)), TypeError, Z_ONLY),
    ("dtype-zpschur_hess_batch_", lambda e, d: e.zpschur_hess_batch_(hess(d.rA)), TypeError,
     "zpschur_hess_batch_: ComplexF64 only (use pschur_hess_batch_ for Float64 problems)"),
    ("dtype-zgpschur_batch_", lambda e, d: e.zgpschur_batch_(work(d.rA), SIGNED), TypeError, Z_ONLY),
    ("dtype-zgpschur_batch", lambda e, d: e.zgpschur_batch(d.rA, SIGNED), TypeError, "zgpschur_batch: ComplexF64 only"),
    ("dtype-zgphessenberg_batch_", lambda e, d: e.zgphessenberg_batch_(work(d.rA), SIGNED), TypeError, Z_ONLY),
    ("dtype-zgpschur_hess_batch_", lambda e, d: e.zgpschur_hess_batch_(hess(d.rA), SIGNED), TypeError,
     "zgpschur_hess_batch_: ComplexF64 only"),
    ("dtype-ordschur_batch_", lambda e, d: e.ordschur_batch_([clone(x) for x in d.zPS], d.sel), NotImplementedPSD,
     "ordschur_batch: Float64 only (use ordschur_ per problem for ComplexF64)"),
    ("dtype-ordschur_batch", lambda e, d: e.ordschur_batch(d.zPS, d.sel), NotImplementedPSD,
     "ordschur_batch: Float64 only (use ordschur_ per problem for ComplexF64)"),
    ("dtype-zordschur_batch_", lambda e, d: e.zordschur_batch_([clone(x) for x in d.rPS], d.sel), NotImplementedPSD,
     "zordschur_batch: ComplexF64 only (Float64 problems: ordschur_batch)"),
    ("dtype-zordschur_batch", lambda e, d: e.zordschur_batch(d.rPS, d.sel), NotImplementedPSD,
     "zordschur_batch: ComplexF64 only (Float64 problems: ordschur_batch)"),
    ("dtype-eigvecs_batch", lambda e, d: e.eigvecs_batch(d.zPS, d.sel), NotImplementedPSD,
     "eigvecs_batch: Float64 only (ComplexF64 problems: zeigvecs_batch)"),
    ("dtype-zeigvecs_batch", lambda e, d: e.zeigvecs_batch(d.rPS, d.sel), TypeError,
     "zeigvecs_batch: ComplexF64 only (Float64 problems: eigvecs_batch)"),
    ("dtype-eigvecs_batch-mixed", lambda e, d: e.eigvecs_batch([altered(d.rPS[0], Z=d.zPS[0].Z)], d.sel), TypeError,
     "must be all real or all complex"),
    ("dtype-zeigvecs_batch-mixed", lambda e, d: e.zeigvecs_batch([altered(d.zPS[0], Z=d.rPS[0].Z)], d.sel), TypeError,
     "must be all real or all complex"),
    # ---- unequal order inside a batch
    ("order-pschur_batch_", lambda e, d: e.pschur_batch_(work(d.rA + d.rA5)), DimensionMismatch, EQ2),
    ("order-pschur_batch", lambda e, d: e.pschur_batch(d.rA + d.rA5), DimensionMismatch, EQ2),
    ("order-phessenberg_batch_", lambda e, d: e.phessenberg_batch_(work(d.rA + d.rA5)), DimensionMismatch, EQ2),
    ("order-pschur_hess_batch_", lambda e, d: e.pschur_hess_batch_(hess(d.rA + d.rA5)), DimensionMismatch, EQ2),
    ("order-zpschur_batch_", lambda e, d: e.zpschur_batch_(work(d.zA + d.zA5)), DimensionMismatch, EQ2),
    ("order-zpschur_batch", lambda e, d: e.zpschur_batch(d.zA + d.zA5), DimensionMismatch, EQ2),
    ("order-zphessenberg_batch_", lambda e, d: e.zphessenberg_batch_(work(d.zA + d.zA5)), DimensionMismatch, EQ2),
    ("order-zpschur_hess_batch_", lambda e, d: e.zpschur_hess_batch_(hess(d.zA + d.zA5)), DimensionMismatch, EQ2),
    ("order-zgpschur_batch_", lambda e, d: e.zgpschur_batch_(work(d.zA + d.zA5), SIGNED), DimensionMismatch, EQ2),
    ("order-zgpschur_batch", lambda e, d: e.zgpschur_batch(d.zA + d.zA5, SIGNED), DimensionMismatch, EQ2),
    ("order-zgphessenberg_batch_", lambda e, d: e.zgphessenberg_batch_(work(d.zA + d.zA5), SIGNED), DimensionMismatch,
     EQ2),
    ("order-zgpschur_hess_batch_", lambda e, d: e.zgpschur_hess_batch_(hess(d.zA + d.zA5), SIGNED), DimensionMismatch,
     EQ2),
    ("order-gpschur_batch", lambda e, d: e.gpschur_batch([d.zA[0][:1], d.zA5[0][:1]], [d.zA[1][:1], d.zA5[0][1:]]),
     DimensionMismatch, EQ2),
    ("order-ordschur_batch_", lambda e, d: e.ordschur_batch_([clone(x) for x in d.rPS + d.rPS5], d.sel),
     DimensionMismatch, EQ4),
    ("order-ordschur_batch", lambda e, d: e.ordschur_batch(d.rPS + d.rPS5, d.sel), DimensionMismatch, EQ4),
    ("order-zordschur_batch_", lambda e, d: e.zordschur_batch_([clone(x) for x in d.zPS + d.zPS5], d.sel),
     DimensionMismatch, EQ4),
    ("order-zordschur_batch", lambda e, d: e.zordschur_batch(d.zPS + d.zPS5, d.sel), DimensionMismatch, EQ4),
    ("order-eigvecs_batch", lambda e, d: e.eigvecs_batch(d.rPS + d.rPS5, d.sel), DimensionMismatch, EQ4),
    ("order-zeigvecs_batch", lambda e, d: e.zeigvecs_batch(d.zPS + d.zPS5, d.sel), DimensionMismatch, EQ4),
    # ---- unequal period inside a batch
    ("period-pschur_batch_", lambda e, d: e.pschur_batch_(work(d.rA + d.rA3)), DimensionMismatch, EQ2),
    ("period-pschur_batch", lambda e, d: e.pschur_batch(d.rA + d.rA3), DimensionMismatch, EQ2),
    ("period-phessenberg_batch_", lambda e, d: e.phessenberg_batch_(work(d.rA + d.rA3)), DimensionMismatch, EQ2),
    ("period-pschur_hess_batch_", lambda e, d: e.pschur_hess_batch_(hess(d.rA + d.rA3)), DimensionMismatch, EQ2),
    ("period-zpschur_batch_", lambda e, d: e.zpschur_batch_(work(d.zA + d.zA3)), DimensionMismatch, EQ2),
    ("period-zpschur_batch", lambda e, d: e.zpschur_batch(d.zA + d.zA3), DimensionMismatch, EQ2),
    ("period-zphessenberg_batch_", lambda e, d: e.zphessenberg_batch_(work(d.zA + d.zA3)), DimensionMismatch, EQ2),
    ("period-zpschur_hess_batch_", lambda e, d: e.zpschur_hess_batch_(hess(d.zA + d.zA3)), DimensionMismatch, EQ2),
    ("period-zgpschur_batch_", lambda e, d: e.zgpschur_batch_(work(d.zA + d.zA3), SIGNED), DimensionMismatch, EQ2),
    ("period-zgpschur_batch", lambda e, d: e.zgpschur_batch(d.zA + d.zA3, SIGNED), DimensionMismatch, EQ2),
    ("period-zgphessenberg_batch_", lambda e, d: e.zgphessenberg_batch_(work(d.zA + d.zA3), SIGNED), DimensionMismatch,
     EQ2),
    ("period-zgpschur_hess_batch_", lambda e, d: e.zgpschur_hess_batch_(hess(d.zA + d.zA3), SIGNED), DimensionMismatch,
     EQ2),
    ("period-gpschur_batch", lambda e, d: e.gpschur_batch([d.zA[0][:1], d.zA[1]], [d.zA[1][:1], d.zA[0]]),
     DimensionMismatch, EQ2),
    ("period-gpschur_batch-pairs", lambda e, d: e.gpschur_batch([d.zA[0]], [d.zA[1][:1]]), DimensionMismatch,
     "As and Bs must have the same length"),
    ("period-gpschur_batch-lists", lambda e, d: e.gpschur_batch([d.zA[0]], []), DimensionMismatch, "one Bs per As"),
    ("period-ordschur_batch_", lambda e, d: e.ordschur_batch_([clone(x) for x in d.rPS + d.rPS3], d.sel),
     DimensionMismatch, EQ4),
    ("period-ordschur_batch", lambda e, d: e.ordschur_batch(d.rPS + d.rPS3, d.sel), DimensionMismatch, EQ4),
    ("period-zordschur_batch_", lambda e, d: e.zordschur_batch_([clone(x) for x in d.zPS + d.zPS3], d.sel),
     DimensionMismatch, EQ4),
    ("period-zordschur_batch", lambda e, d: e.zordschur_batch(d.zPS + d.zPS3, d.sel), DimensionMismatch, EQ4),
    ("period-eigvecs_batch", lambda e, d: e.eigvecs_batch(d.rPS + d.rPS3, d.sel), DimensionMismatch, EQ4),
    ("period-zeigvecs_batch", lambda e, d: e.zeigvecs_batch(d.zPS + d.zPS3, d.sel), DimensionMismatch, EQ4),
    # ---- unequal orientation / schurindex (the methods that take decompositions)
    ("orient-ordschur_batch_", lambda e, d: e.ordschur_batch_([clone(d.rPS[0]), altered(d.rPS[1], orientation="L")],
                                                              d.sel), DimensionMismatch, EQ4),
    ("orient-zordschur_batch_", lambda e, d: e.zordschur_batch_([clone(d.zPS[0]), altered(d.zPS[1], orientation="L")],
                                                                d.sel), DimensionMismatch, EQ4),
    ("orient-eigvecs_batch", lambda e, d: e.eigvecs_batch([d.rPS[0], altered(d.rPS[1], orientation="L")], d.sel),
     DimensionMismatch, EQ4),
    ("orient-zeigvecs_batch", lambda e, d: e.zeigvecs_batch([d.zPS[0], altered(d.zPS[1], orientation="L")], d.sel),
     DimensionMismatch, EQ4),
    ("schurindex-ordschur_batch_", lambda e, d: e.ordschur_batch_([clone(d.rPS[0]), altered(d.rPS[1], schurindex=P)],
                                                                  d.sel), DimensionMismatch, EQ4),
    ("schurindex-zordschur_batch_", lambda e, d: e.zordschur_batch_([clone(d.zPS[0]), altered(d.zPS[1], schurindex=P)],
                                                                    d.sel), DimensionMismatch, EQ4),
    ("schurindex-eigvecs_batch", lambda e, d: e.eigvecs_batch([d.rPS[0], altered(d.rPS[1], schurindex=P)], d.sel),
     DimensionMismatch, EQ4),
    ("schurindex-zeigvecs_batch", lambda e, d: e.zeigvecs_batch([d.zPS[0], altered(d.zPS[1], schurindex=P)], d.sel),
     DimensionMismatch, EQ4),
    ("schurindex-inner-ordschur_batch_", lambda e, d: e.ordschur_batch_([altered(x, schurindex=2) for x in d.rPS3],
                                                                        d.sel), ValueError, "schurindex in (1,p)"),
    ("schurindex-inner-zordschur_batch_", lambda e, d: e.zordschur_batch_([altered(x, schurindex=2) for x in d.zPS3],
                                                                          d.sel), ValueError, "schurindex in (1,p)"),
    # ---- Schur vectors
    ("noZ-eigvecs_batch", lambda e, d: e.eigvecs_batch([altered(x, Z=[]) for x in d.rPS], d.sel), ValueError, NOZ),
    ("noZ-zeigvecs_batch", lambda e, d: e.zeigvecs_batch([altered(x, Z=[]) for x in d.zPS], d.sel), ValueError, NOZ),
    ("shortZ-ordschur_batch_", lambda e, d: e.ordschur_batch_([altered(x, Z=x.Z[:1]) for x in d.rPS3], d.sel),
     DimensionMismatch, "one Z per factor"),
    ("shortZ-zordschur_batch_", lambda e, d: e.zordschur_batch_([altered(x, Z=x.Z[:1]) for x in d.zPS3], d.sel),
     DimensionMismatch, "one Z per factor"),
    # ---- a signed GeneralizedPeriodicSchur
    ("signed-ordschur_batch_", lambda e, d: e.ordschur_batch_([clone(x) for x in d.gPS], d.sel), NotImplementedPSD,
     "ordschur_batch: signed GeneralizedPeriodicSchur (use ordschur_ per problem)"),
    ("signed-zordschur_batch_", lambda e, d: e.zordschur_batch_([clone(x) for x in d.gPS], d.sel), NotImplementedPSD,
     "zordschur_batch: signed GeneralizedPeriodicSchur (use ordschur_ per problem)"),
    ("signed-zordschur_batch", lambda e, d: e.zordschur_batch(d.gPS, d.sel), NotImplementedPSD,
     "zordschur_batch: signed GeneralizedPeriodicSchur (use ordschur_ per problem)"),
    ("signed-eigvecs_batch", lambda e, d: e.eigvecs_batch(d.gPS, d.sel), NotImplementedPSD,
     "eigvecs_batch: signed GeneralizedPeriodicSchur (use geigvecs per problem)"),
    ("signed-zeigvecs_batch", lambda e, d: e.zeigvecs_batch(d.gPS, d.sel), NotImplementedPSD,
     "zeigvecs_batch: signed GeneralizedPeriodicSchur (use geigvecs per problem)"),
    # ---- the shape of select, in both spellings
    ("select-ordschur_batch_", lambda e, d: e.ordschur_batch_([clone(x) for x in d.rPS], [True] * (N + 1)),
     DimensionMismatch, SEL_ORD),
    ("select-ordschur_batch", lambda e, d: e.ordschur_batch(d.rPS, np.ones((NB + 1, N), dtype=bool)),
     DimensionMismatch, SEL_ORD),
    ("select-zordschur_batch_", lambda e, d: e.zordschur_batch_([clone(x) for x in d.zPS], [True] * (N + 1)),
     DimensionMismatch, SEL_ORD),
    ("select-zordschur_batch", lambda e, d: e.zordschur_batch(d.zPS, np.ones((NB + 1, N), dtype=bool)),
     DimensionMismatch, SEL_ORD),
    ("select-eigvecs_batch", lambda e, d: e.eigvecs_batch(d.rPS, [True] * (N + 1)), ValueError, "argument 9 invalid"),
    ("select-zeigvecs_batch", lambda e, d: e.zeigvecs_batch(d.zPS, np.ones((NB + 1, N), dtype=bool)), ValueError,
     "argument 9 invalid"),
    # ---- the signature of the signed entries
    ("Slen-zgpschur_batch_", lambda e, d: e.zgpschur_batch_(work(d.zA), [True] * (P + 1)), DimensionMismatch,
     "length of S must match the period"),
    ("Slen-zgpschur_batch", lambda e, d: e.zgpschur_batch(d.zA, [True] * (P + 1)), DimensionMismatch,
     "length of S must match the period"),
    ("Slen-zpschur_batch-S", lambda e, d: e.zpschur_batch(d.zA, "R", S=[True] * (P + 1)), DimensionMismatch,
     "length of S must match the period"),
    ("Slen-zgphessenberg_batch_", lambda e, d: e.zgphessenberg_batch_(work(d.zA), [True] * (P + 1)), DimensionMismatch,
     "length of S must match the period"),
    ("Slen-zgpschur_hess_batch_", lambda e, d: e.zgpschur_hess_batch_(hess(d.zA), [True] * (P + 1)), DimensionMismatch,
     "S must have one entry per factor"),
    ("S1-zgpschur_batch_", lambda e, d: e.zgpschur_batch_(work(d.zA), [False, True]), ValueError,
     "The leftmost entry in S must be true"),
    ("S1-zgpschur_batch-L", lambda e, d: e.zgpschur_batch(d.zA, [True, False], "L"), ValueError,
     "The leftmost entry in S must be true"),
    ("S1-zgphessenberg_batch_", lambda e, d: e.zgphessenberg_batch_(work(d.zA), [False, True]), ValueError,
     "The leftmost entry in S must be true"),
    ("S1-zgpschur_hess_batch_", lambda e, d: e.zgpschur_hess_batch_(hess(d.zA), [False, True]), ValueError,
     "Signature entry S[1] must be true"),
    # ---- in place needs work arrays, and an orientation
    ("work-pschur_batch_", lambda e, d: e.pschur_batch_([[np.ascontiguousarray(a) for a in A] for A in d.rA]),
     TypeError, NEEDS_F64),
    ("work-zpschur_batch_", lambda e, d: e.zpschur_batch_([[np.ascontiguousarray(a) for a in A] for A in d.zA]),
     TypeError, "needs writable Fortran-ordered complex128 matrices"),
    ("work-ordschur_batch_", lambda e, d: e.ordschur_batch_(
        [altered(x, Ts=[np.ascontiguousarray(t) for t in x.Ts]) for x in d.rPS], d.sel), TypeError, NEEDS_F64),
    ("work-zordschur_batch_", lambda e, d: e.zordschur_batch_(
        [altered(x, Z=[np.ascontiguousarray(z) for z in x.Z]) for x in d.zPS], d.sel), TypeError,
     "needs writable Fortran-ordered complex128 matrices"),
    ("lr-pschur_batch", lambda e, d: e.pschur_batch(d.rA, "X"), ValueError, "orientation argument must be either"),
    ("lr-zpschur_batch", lambda e, d: e.zpschur_batch(d.zA, "X"), ValueError, "orientation argument must be either"),
    ("lr-zgpschur_batch", lambda e, d: e.zgpschur_batch(d.zA, SIGNED, "X"), ValueError,
     "orientation argument must be either"),
    # ---- the count of positional arguments
    ("usage-ordschur_batch_", lambda e, d: e.ordschur_batch_([clone(x) for x in d.rPS]), TypeError,
     "ordschur_batch_(problems, select, wantZ=True)"),
    ("usage-zordschur_batch_", lambda e, d: e.zordschur_batch_([clone(x) for x in d.zPS], d.sel, d.sel), TypeError,
     "zordschur_batch_(problems, select, wantZ=True)"),
    ("usage-eigvecs_batch", lambda e, d: e.eigvecs_batch(d.rPS), TypeError,
     "eigvecs_batch(problems, select, shifted=True)"),
    ("usage-zeigvecs_batch", lambda e, d: e.zeigvecs_batch(d.zPS, d.sel, d.sel), TypeError,
     "zeigvecs_batch(problems, select, shifted=True)"),
    ("usage-dev-ordschur_batch_", lambda e, d: e.ordschur_batch_(_cpu(False), _cpu(False)), TypeError,
     "ordschur_batch_(T, Z, select, lr=..., schurindex=...)"),
    ("usage-dev-zordschur_batch_", lambda e, d: e.zordschur_batch_(_cpu(True), _cpu(True)), TypeError,
     "zordschur_batch_(T, Z, select, lr=..., schurindex=...)"),
    ("usage-dev-eigvecs_batch", lambda e, d: e.eigvecs_batch(_cpu(False), _cpu(False), d.sel), TypeError,
     "eigvecs_batch(T, Z, values, select, lr=..., schurindex=...)"),
    ("usage-dev-zeigvecs_batch", lambda e, d: e.zeigvecs_batch(_cpu(True), _cpu(True), d.sel), TypeError,
     "zeigvecs_batch(T, Z, values, select, lr=..., schurindex=...)"),
    # ---- a torch tensor that is not on the device, given to each device entry
    ("host-pschur_batch_", lambda e, d: e.pschur_batch_(_cpu(False)), TypeError,
     "device-resident pschur_batch needs a GPU tensor (use lists of numpy arrays for host input)"),
    ("host-pschur_batch", lambda e, d: e.pschur_batch(_cpu(False)), TypeError,
     "device-resident pschur_batch needs a GPU tensor"),
    ("host-zpschur_batch_", lambda e, d: e.zpschur_batch_(_cpu(True)), TypeError,
     "device-resident zpschur_batch needs a GPU tensor (use lists of numpy arrays for host input)"),
    ("host-zgpschur_batch_", lambda e, d: e.zgpschur_batch_(_cpu(True), SIGNED), TypeError,
     "device-resident zgpschur_batch needs a GPU tensor (use lists of numpy arrays for host input)"),
    ("host-ordschur_batch_", lambda e, d: e.ordschur_batch_(_cpu(False), _cpu(False), [True] * 3), TypeError,
     "device-resident ordschur_batch needs GPU tensors (use a list of PeriodicSchur for host input)"),
    ("host-zordschur_batch_", lambda e, d: e.zordschur_batch_(_cpu(True), None, [True] * 3, wantZ=False), TypeError,
     "device-resident zordschur_batch needs GPU tensors (use a list of PeriodicSchur for host input)"),
    ("host-eigvecs_batch", lambda e, d: e.eigvecs_batch(_cpu(False), _cpu(False), np.zeros((NB, 3)), [True] * 3),
     TypeError, "device-resident eigvecs_batch needs GPU tensors (use a list of PeriodicSchur for host input)"),
    ("host-zeigvecs_batch", lambda e, d: e.zeigvecs_batch(_cpu(True), _cpu(True), np.zeros((NB, 3)), [True] * 3),
     TypeError, "device-resident zeigvecs_batch needs GPU tensors (use a list of PeriodicSchur for host input)"),
    # ---- what the device entries check before that
    ("devshape-pschur_batch_", lambda e, d: e.pschur_batch_(_cpu(False)[:, :, :, :2]), DimensionMismatch,
     "a device batch is one [nb, p, n, n] tensor of square factors"),
    ("devshape-zgpschur_batch_", lambda e, d: e.zgpschur_batch_(_cpu(True)[0], SIGNED), DimensionMismatch,
     "a device batch is one [nb, p, n, n] tensor of square factors"),
    ("devshape-ordschur_batch_", lambda e, d: e.ordschur_batch_(_cpu(False), _cpu(False)[:1], [True] * 3),
     DimensionMismatch, "a device batch is [nb, p, n, n] tensors T and Z of square factors"),
    ("devshape-zeigvecs_batch", lambda e, d: e.zeigvecs_batch(_cpu(True), _cpu(True)[:1], np.zeros((NB, 3)), [True] * 3),
     DimensionMismatch, "a device batch is [nb, p, n, n] tensors T and Z of square factors"),
    ("devdtype-pschur_batch_", lambda e, d: e.pschur_batch_(_cpu(True)), NotImplementedPSD, R_ONLY),
    ("devdtype-zpschur_batch_", lambda e, d: e.zpschur_batch_(_cpu(False)), TypeError, Z_ONLY),
    ("devdtype-zgpschur_batch_", lambda e, d: e.zgpschur_batch_(_cpu(False), SIGNED), TypeError,
     "zgpschur_batch: ComplexF64 only"),
    ("devdtype-ordschur_batch_", lambda e, d: e.ordschur_batch_(_cpu(True), None, [True] * 3), NotImplementedPSD,
     "ordschur_batch: Float64 only (use ordschur_ per problem for ComplexF64)"),
    ("devdtype-zordschur_batch_", lambda e, d: e.zordschur_batch_(_cpu(True), _cpu(False), [True] * 3),
     NotImplementedPSD, "zordschur_batch: ComplexF64 only (Float64 problems: ordschur_batch)"),
    ("devdtype-eigvecs_batch", lambda e, d: e.eigvecs_batch(_cpu(True), _cpu(True), np.zeros((NB, 3)), [True] * 3),
     NotImplementedPSD, "eigvecs_batch: Float64 only (ComplexF64 problems: zeigvecs_batch)"),
    ("devdtype-zeigvecs_batch", lambda e, d: e.zeigvecs_batch(_cpu(False), _cpu(False), np.zeros((NB, 3)), [True] * 3),
     TypeError, "zeigvecs_batch: ComplexF64 only (Float64 problems: eigvecs_batch)"),
    ("devdtype-zeigvecs_batch-mixed", lambda e, d: e.zeigvecs_batch(_cpu(True), _cpu(False), np.zeros((NB, 3)),
                                                                    [True] * 3),
     TypeError, "must be all real or all complex"),
    ("devnoZ-eigvecs_batch", lambda e, d: e.eigvecs_batch(_cpu(False), None, np.zeros((NB, 3)), [True] * 3), ValueError,
     NOZ),
    ("devnoZ-zeigvecs_batch", lambda e, d: e.zeigvecs_batch(_cpu(True), None, np.zeros((NB, 3)), [True] * 3), ValueError,
     NOZ),
]


@pytest.mark.parametrize("call,exc,text", [r[1:] for r in ERRORS], ids=[r[0] for r in ERRORS])
def test_exception_table(D, call, exc, text):
    with pytest.raises(exc) as ei:
        call(D.eng, D)
    assert type(ei.value) is exc and text in str(ei.value), (type(ei.value), str(ei.value))


# (id, call on (eng, infos), the return value checked, whether infos_out is cleared; None: the entry takes no infos_out)
def _is_empty_list(r):
    return r == []


def _is_empty_with_stats(r):
    return r[0] == [] and isinstance(r[1], psd_amd.Stats) and r[1].nlaunch_step == 0


EMPTY = [
    ("pschur_batch_", lambda e, i: e.pschur_batch_([], infos_out=i), _is_empty_list, True),
    ("pschur_batch", lambda e, i: e.pschur_batch([], infos_out=i), _is_empty_list, True),
    ("phessenberg_batch_", lambda e, i: e.phessenberg_batch_([]), _is_empty_with_stats, None),
    ("pschur_hess_batch_", lambda e, i: e.pschur_hess_batch_([], infos_out=i), _is_empty_list, False),
    ("zpschur_batch_", lambda e, i: e.zpschur_batch_([], infos_out=i), _is_empty_list, True),
    ("zpschur_batch", lambda e, i: e.zpschur_batch([], infos_out=i), _is_empty_list, True),
    ("zpschur_batch-S", lambda e, i: e.zpschur_batch([], S=SIGNED, infos_out=i), _is_empty_list, True),
    ("zphessenberg_batch_", lambda e, i: e.zphessenberg_batch_([]), _is_empty_with_stats, None),
    ("zpschur_hess_batch_", lambda e, i: e.zpschur_hess_batch_([], infos_out=i), _is_empty_list, True),
    ("zgpschur_batch_", lambda e, i: e.zgpschur_batch_([], SIGNED, "L", infos_out=i), _is_empty_list, True),
    ("zgpschur_batch", lambda e, i: e.zgpschur_batch([], SIGNED, infos_out=i), _is_empty_list, True),
    ("zgphessenberg_batch_", lambda e, i: e.zgphessenberg_batch_([], SIGNED), _is_empty_with_stats, None),
    ("zgpschur_hess_batch_", lambda e, i: e.zgpschur_hess_batch_([], SIGNED, infos_out=i), _is_empty_list, True),
    ("gpschur_batch", lambda e, i: e.gpschur_batch([], [], infos_out=i), _is_empty_list, False),
    ("ordschur_batch_", lambda e, i: e.ordschur_batch_([], [], infos_out=i), _is_empty_list, True),
    ("ordschur_batch", lambda e, i: e.ordschur_batch([], [], infos_out=i), _is_empty_list, True),
    ("zordschur_batch_", lambda e, i: e.zordschur_batch_([], [], infos_out=i), _is_empty_list, True),
    ("zordschur_batch", lambda e, i: e.zordschur_batch([], [], infos_out=i), _is_empty_list, True),
    ("eigvecs_batch", lambda e, i: e.eigvecs_batch([], []), _is_empty_list, None),
    ("zeigvecs_batch", lambda e, i: e.zeigvecs_batch([], []), _is_empty_list, None),
]


@pytest.mark.parametrize("call,check,cleared", [r[1:] for r in EMPTY], ids=[r[0] for r in EMPTY])
def test_empty_batch_table(sim_engine, call, check, cleared):
    infos = [7]
    assert check(call(sim_engine, infos))
    assert infos == ([] if cleared else [7])


def test_empty_batch_resets_the_call_attributes(D):
    eng = D.eng
    eng.ordschur_batch([clone(x) for x in D.rPS], D.sel)
    assert len(eng.ordschur_batch_nswaps) == NB and eng.ordschur_batch_stats.nlaunch_step > 0
    eng.ordschur_batch_([], [])
    assert len(eng.ordschur_batch_nswaps) == 0 and eng.ordschur_batch_stats.nlaunch_step == 0
    eng.zordschur_batch(D.zPS, D.sel)
    assert len(eng.zordschur_batch_nswaps) == NB and eng.zordschur_batch_stats.nlaunch_step > 0
    eng.zordschur_batch_([], [])
    assert len(eng.zordschur_batch_nswaps) == 0 and eng.zordschur_batch_stats.nlaunch_step == 0
    for full, empty in ((lambda: eng.eigvecs_batch(D.rPS, D.sel), lambda: eng.eigvecs_batch([], [])),
                        (lambda: eng.zeigvecs_batch(D.zPS, D.sel), lambda: eng.zeigvecs_batch([], []))):
        full()
        assert eng.eigvecs_batch_stats.nb == NB and eng.eigvecs_batch_counts.shape == (NB, 3)
        empty()
        assert eng.eigvecs_batch_stats.nb == 0 and eng.eigvecs_batch_counts.shape == (0, 3)


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _scaled(g):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return g.alpha / g.beta * 2.0 ** g.alphascale


def _hess_flat(H):
    return [[h[0]] + list(h[1]) for h in H]


# (id, problems from D, call on (eng, problems), the class returned, flat factors of the problems)
DECOMPOSE = [
    ("pschur_batch_", lambda d: work(d.rA), lambda e, w: e.pschur_batch_(w), PeriodicSchur, lambda w: w),
    ("pschur_hess_batch_", lambda d: hess(d.rA), lambda e, w: e.pschur_hess_batch_(w), PeriodicSchur, _hess_flat),
    ("zpschur_batch_", lambda d: work(d.zA), lambda e, w: e.zpschur_batch_(w), PeriodicSchur, lambda w: w),
    ("zpschur_batch_-S", lambda d: work(d.zA), lambda e, w: e.zpschur_batch_(w, S=SIGNED), GeneralizedPeriodicSchur,
     lambda w: w),
    ("zpschur_hess_batch_", lambda d: hess(d.zA), lambda e, w: e.zpschur_hess_batch_(w), GeneralizedPeriodicSchur,
     _hess_flat),
    ("zgpschur_batch_", lambda d: work(d.zA), lambda e, w: e.zgpschur_batch_(w, SIGNED), GeneralizedPeriodicSchur,
     lambda w: w),
    ("zgpschur_hess_batch_", lambda d: hess(d.zA), lambda e, w: e.zgpschur_hess_batch_(w, SIGNED),
     GeneralizedPeriodicSchur, _hess_flat),
]


@pytest.mark.parametrize("make,call,cls,flat", [r[1:] for r in DECOMPOSE], ids=[r[0] for r in DECOMPOSE])
def test_in_place_forms_return_the_callers_arrays(D, make, call, cls, flat):
    w = make(D)
    before = [[a.copy() for a in A] for A in flat(w)]
    out = call(D.eng, w)
    assert len(out) == NB
    for q, ps in enumerate(out):
        assert type(ps) is cls and len(ps.Ts) == P and len(ps.Z) == P
        assert all(t is a for t, a in zip(ps.Ts, flat(w)[q]))  # the T factors ARE the caller's arrays, overwritten
        assert any(not _bits(a, b) for a, b in zip(flat(w)[q], before[q]))
        assert ps.values.dtype == np.complex128 and ps.values.shape == (N,)
        if cls is GeneralizedPeriodicSchur:
            assert _bits(ps.values, _scaled(ps))
            assert ps.alpha.dtype == np.complex128 and ps.beta.dtype == np.float64 and ps.alphascale.dtype == np.int32


def test_hess_forms_overwrite_a_given_Q(D):
    eng = D.eng
    for probs, call, dt in ((hess(D.rA), eng.pschur_hess_batch_, np.float64),
                            (hess(D.zA), eng.zpschur_hess_batch_, np.complex128),
                            (hess(D.zA), lambda w: eng.zgpschur_hess_batch_(w, SIGNED), np.complex128)):
        Q = [[np.asfortranarray(np.eye(N, dtype=dt)) for _ in range(P)] for _ in range(NB)]
        out = call([(h[0], h[1], q) for h, q in zip(probs, Q)])
        for q in range(NB):
            assert all(z is a for z, a in zip(out[q].Z, Q[q])) and not _bits(Q[q][0], np.eye(N, dtype=dt))
        Q[1] = None  # (no Q for one problem: the identity is taken)
        out = call([(h[0], h[1], q) for h, q in zip(probs, Q)])
        assert len(out[1].Z) == P and all(z is a for z, a in zip(out[0].Z, Q[0]))


COPYING = [
    ("pschur_batch", lambda d: d.rA, lambda e, A: e.pschur_batch(A), PeriodicSchur),
    ("zpschur_batch", lambda d: d.zA, lambda e, A: e.zpschur_batch(A), PeriodicSchur),
    ("zpschur_batch-S", lambda d: d.zA, lambda e, A: e.zpschur_batch(A, S=SIGNED), GeneralizedPeriodicSchur),
    ("zgpschur_batch", lambda d: d.zA, lambda e, A: e.zgpschur_batch(A, SIGNED), GeneralizedPeriodicSchur),
]


@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("make,call,cls", [r[1:] for r in COPYING], ids=[r[0] for r in COPYING])
def test_copying_forms_leave_the_factors(D, make, call, cls, order):
    A = [[np.array(a, order=order, copy=True) for a in Aq] for Aq in make(D)]
    keep = [[a.copy(order="K") for a in Aq] for Aq in A]
    out = call(D.eng, A)
    assert all(type(ps) is cls for ps in out)
    for q in range(NB):
        assert all(_bits(a, b) and a.flags.c_contiguous == b.flags.c_contiguous for a, b in zip(A[q], keep[q]))
        assert not any(t is a for t in out[q].Ts for a in A[q])


def test_gpschur_batch(D):
    As, Bs = [A[:1] for A in D.zA], [A[1:] for A in D.zA]
    keep = [a.copy() for A in D.zA for a in A]
    out = D.eng.gpschur_batch(As, Bs)
    assert all(type(g) is GeneralizedPeriodicSchur and g.S == [True, False] for g in out) and len(out) == NB
    assert all(_bits(a, b) for a, b in zip([a for A in D.zA for a in A], keep))
    assert all(_bits(g.values, _scaled(g)) for g in out)
    real = D.eng.gpschur_batch([A[:1] for A in D.rA], [A[1:] for A in D.rA])  # (real pairs are taken as complex)
    assert all(type(g) is GeneralizedPeriodicSchur and np.iscomplexobj(g.Ts[0]) for g in real)


def test_values_bits(D):
    """`values` of the complex entries is alpha / beta * 2^alphascale of the same result, bit for bit; zpschur_batch
    returns no alpha: its values are those of the signed entry with an all-true signature (the same path)."""
    for g in D.gPS + D.tPS:
        assert _bits(g.values, _scaled(g))
    for ps, g in zip(D.zPS, D.tPS):
        assert type(ps) is PeriodicSchur and not hasattr(ps, "alpha") and _bits(ps.values, g.values)


@pytest.mark.parametrize("z", [False, True], ids=["ordschur", "zordschur"])
def test_ordschur_mutation(D, z):
    eng = D.eng
    ps0 = D.zPS if z else D.rPS
    inplace, copying = (eng.zordschur_batch_, eng.zordschur_batch) if z else (eng.ordschur_batch_, eng.ordschur_batch)
    keep = [clone(x) for x in ps0]
    out = copying(ps0, D.sel)
    for a, b, o in zip(ps0, keep, out):
        assert o is not a and type(o) is PeriodicSchur
        assert all(_bits(x, y) for x, y in zip(a.Ts + a.Z + [a.values], b.Ts + b.Z + [b.values]))
    w = [clone(x) for x in ps0]
    arrays = [x.Ts + x.Z for x in w]
    out2 = inplace(w, D.sel)
    assert out2 is not None and all(o is x for o, x in zip(out2, w))  # the same objects, mutated
    for q, x in enumerate(w):
        assert all(a is b for a, b in zip(x.Ts + x.Z, arrays[q]))  # and the same arrays, overwritten
        assert not _bits(x.Ts[0], keep[q].Ts[0]) and not _bits(x.values, keep[q].values)
        assert all(_bits(a, b) for a, b in zip(x.Ts + x.Z + [x.values], out[q].Ts + out[q].Z + [out[q].values]))
        assert x.stats.nsweeps == (eng.zordschur_batch_nswaps if z else eng.ordschur_batch_nswaps)[q]
    noZ = inplace([altered(x, Z=[]) for x in ps0], D.sel)  # (no Schur vectors: the factors alone)
    assert all(_bits(a.Ts[0], b.Ts[0]) and a.Z == [] for a, b in zip(noZ, w))


def test_zordschur_writes_alpha_back_only_on_generalized(D):
    eng = D.eng
    plain = eng.zordschur_batch_([clone(x) for x in D.zPS], D.sel)
    assert all(type(x) is PeriodicSchur and not hasattr(x, "alpha") for x in plain)
    gen = [clone(g) for g in D.tPS]
    old = [g.alpha for g in gen]
    out = eng.zordschur_batch_(gen, D.sel)
    for g, a0, ps in zip(out, old, plain):
        assert type(g) is GeneralizedPeriodicSchur and g.alpha is not a0 and not _bits(g.alpha, a0)
        assert _bits(g.values, _scaled(g)) and _bits(g.values, ps.values)
        assert g.alpha.shape == (N,) and g.beta.shape == (N,) and g.alphascale.dtype == np.int32
    cp = eng.zordschur_batch(D.tPS, D.sel)  # the copying form: the inputs keep their alpha
    assert all(_bits(g.alpha, c.alpha) for g, c in zip(out, cp)) and all(c is not t for c, t in zip(cp, D.tPS))
    assert all(_bits(t.values, _scaled(t)) for t in D.tPS)


def test_ordschur_takes_a_real_all_true_generalized(D):
    """Float64 GeneralizedPeriodicSchur with S all true (what pschur_ with S returns): reordered like a PeriodicSchur;
    values are updated, alpha / beta / alphascale are not the real entry's to write"""
    eng = D.eng

    def gen():
        return [GeneralizedPeriodicSchur([True] * P, c.Ts, c.Z, np.array(c.values), np.ones(N), np.zeros(N, dtype=np.int32),
                                         c.orientation, c.schurindex) for c in (clone(x) for x in D.rPS)]

    plain = eng.ordschur_batch([clone(x) for x in D.rPS], D.sel)
    G = gen()
    old = [(g.alpha, g.beta, g.alphascale, g.values.copy()) for g in G]
    infos = [7]
    out = eng.ordschur_batch_(G, D.sel, infos_out=infos)
    assert infos == [0] * NB and all(o is g for o, g in zip(out, G))
    for g, o, ps in zip(G, old, plain):
        assert type(g) is GeneralizedPeriodicSchur and g.alpha is o[0] and g.beta is o[1] and g.alphascale is o[2]
        assert _bits(g.values, ps.values) and not _bits(g.values, o[3])
        assert all(_bits(a, b) for a, b in zip(g.Ts + g.Z, ps.Ts + ps.Z))
    G = gen()
    cp = eng.ordschur_batch(G, D.sel)  # the copying form: G stays, the copies keep its alpha
    for c, g, ps, r in zip(cp, G, plain, D.rPS):
        assert type(c) is GeneralizedPeriodicSchur and c is not g and _bits(c.values, ps.values)
        assert _bits(g.values, r.values) and all(_bits(a, b) for a, b in zip(g.Ts + g.Z, r.Ts + r.Z))
    V = eng.eigvecs_batch(gen(), [True] * N)  # and its vectors are those of the PeriodicSchur
    assert all(_bits(a, b) for v, w in zip(V, eng.eigvecs_batch(D.rPS, [True] * N)) for a, b in zip(v, w))


def test_values_are_arrays_of_their_own(D):
    """every problem's `values` owns its memory: none is a view that keeps the arrays of the whole batch alive"""
    eng = D.eng
    results = (D.rPS + D.zPS + D.gPS + eng.pschur_hess_batch_(hess(D.rA)) + eng.zpschur_hess_batch_(hess(D.zA))
               + eng.ordschur_batch(D.rPS, D.sel) + eng.zordschur_batch(D.zPS, D.sel) + eng.zordschur_batch(D.tPS, D.sel))
    assert all(ps.values.base is None and ps.values.flags.owndata for ps in results)


@pytest.mark.parametrize("z", [False, True], ids=["eigvecs", "zeigvecs"])
def test_eigvecs_reads_only(D, z):
    eng = D.eng
    ps0 = (D.tPS if z else D.rPS)
    keep = [clone(x) for x in ps0]
    V = (eng.zeigvecs_batch if z else eng.eigvecs_batch)(ps0, [True] * N)
    assert len(V) == NB and all(len(v) == P and v[0].shape == (N, N) and v[0].dtype == np.complex128 for v in V)
    V1 = (eng.zeigvecs_batch if z else eng.eigvecs_batch)(ps0, [True] * N, shifted=False)
    assert all(len(v) == 1 and _bits(v[0], w[0]) for v, w in zip(V1, V))
    for a, b in zip(ps0, keep):
        assert all(_bits(x, y) for x, y in zip(a.Ts + a.Z + [a.values], b.Ts + b.Z + [b.values]))
    # C-ordered factors are read as they are (a copy is made for the call)
    Vc = (eng.zeigvecs_batch if z else eng.eigvecs_batch)(
        [altered(x, Ts=[np.ascontiguousarray(t) for t in x.Ts]) for x in ps0], [True] * N)
    assert all(_bits(a, b) for v, w in zip(Vc, V) for a, b in zip(v, w))
    if z:  # a plain PeriodicSchur gives its values as alpha with beta = 1, scale 0
        Vp = eng.zeigvecs_batch(D.zPS, [True] * N)
        for v, w in zip(Vp, V):
            assert np.abs(v[0] - w[0]).max() <= 1e-10


def test_infos_out_receives_the_codes(D):
    eng = D.eng
    for call in (lambda i: eng.pschur_batch(D.rA, infos_out=i), lambda i: eng.zpschur_batch(D.zA, infos_out=i),
                 lambda i: eng.zgpschur_batch(D.zA, SIGNED, infos_out=i),
                 lambda i: eng.pschur_hess_batch_(hess(D.rA), infos_out=i),
                 lambda i: eng.zpschur_hess_batch_(hess(D.zA), infos_out=i),
                 lambda i: eng.zgpschur_hess_batch_(hess(D.zA), SIGNED, infos_out=i),
                 lambda i: eng.ordschur_batch(D.rPS, D.sel, infos_out=i),
                 lambda i: eng.zordschur_batch(D.zPS, D.sel, infos_out=i)):
        infos = [7]
        call(infos)
        assert infos == [0] * NB and all(type(x) is int for x in infos)
