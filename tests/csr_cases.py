"""Sparse (CSR) cases of partial_pschur and of the driver's SpMV kernel, shared by the CPU tier (serial simulation) and
the GPU tier.  numpy only: the GPU machine need not have scipy."""
import numpy as np

import psd_amd

CSR = psd_amd.CSR
EPS = np.finfo(np.float64).eps
GROUPS = (0, 1, 2, 4, 8, 16, 32, 64)


def to_csr(dense):
    """Every non-zero of a dense square matrix, columns ascending."""
    dense = np.asarray(dense)
    n = dense.shape[0]
    rows, cols = np.nonzero(dense)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    return CSR(n, indptr, cols.astype(np.int32), np.ascontiguousarray(dense[rows, cols]))


def full_csr(dense):
    """A dense square matrix stored with every entry (zeros included)."""
    dense = np.asarray(dense)
    n = dense.shape[0]
    return CSR(n, np.arange(n + 1, dtype=np.int64) * n, np.tile(np.arange(n, dtype=np.int32), n),
               np.ascontiguousarray(dense).reshape(-1).copy())


def row_index(csr):
    """The row of every stored entry."""
    return np.repeat(np.arange(csr.n), np.diff(np.asarray(csr.indptr)))


def csr_to_dense(csr):
    data = np.asarray(csr.data)
    nnz = int(csr.indptr[-1])
    out = np.zeros((csr.n, csr.n), dtype=data.dtype)
    np.add.at(out, (row_index(csr), np.asarray(csr.indices)[:nnz]), data[:nnz])
    return out


def csr_matmat(csr, X, absolute=False):
    """A X (X a vector or n x k): the products of the stored entries, summed row by row (the entries of a row are
    contiguous; empty rows stay 0); absolute: |A| |X|."""
    X = np.asarray(X)
    indptr = np.asarray(csr.indptr)
    nnz = int(indptr[-1])
    data, cols = np.asarray(csr.data)[:nnz], np.asarray(csr.indices)[:nnz]
    if absolute:
        data, X = np.abs(data), np.abs(X)
    out = np.zeros((csr.n,) + X.shape[1:], dtype=np.result_type(data.dtype, X.dtype))
    filled = np.diff(indptr) > 0
    if nnz:
        prod = data[(slice(None),) + (None,) * (X.ndim - 1)] * X[cols]
        out[filled] = np.add.reduceat(prod, indptr[:-1][filled], axis=0)
    return out


def _randn(rng, shape, cplx):
    if cplx:
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)
    return rng.standard_normal(shape)


def _distinct_columns(rng, n, k):
    """k distinct random columns for each of n rows."""
    if k * k > n:  # (repeats are likely: a random permutation per row)
        return np.argsort(rng.random((n, n)), axis=1)[:, :k]
    cols = rng.integers(0, n, (n, k))
    while True:  # redraw the rows that hold a repeat
        srt = np.sort(cols, axis=1)
        bad = np.any(srt[:, 1:] == srt[:, :-1], axis=1)
        if not bad.any():
            return cols
        cols[bad] = rng.integers(0, n, (int(bad.sum()), k))


def sparse_dominant(n, p, k, cplx=False, seed=0, dense=False):
    """The sparse counterpart of krylov_cases.dominant: diag(d) with 16 leading entries of d from 2.0 to 1.3 and the rest
    1, plus k entries per row at distinct random columns with values 0.3 / sqrt(k) times standard normal numbers.  (A
    random column may be the diagonal's: then the row stores that column twice.)  Returns the p CSR factors, and their
    dense copies as well when dense is set."""
    rng = np.random.default_rng(seed)
    d = np.ones(n)
    d[: min(16, n)] = np.linspace(2.0, 1.3, 16)[: min(16, n)]
    kk = min(k, n)
    out = []
    for _ in range(p):
        cols = _distinct_columns(rng, n, kk)
        vals = 0.3 / np.sqrt(k) * _randn(rng, (n, kk), cplx)
        indices = np.concatenate([np.arange(n)[:, None], cols], axis=1).astype(np.int32)
        data = np.concatenate([d[:, None].astype(vals.dtype), vals], axis=1)
        out.append(CSR(n, np.arange(n + 1, dtype=np.int64) * (kk + 1), indices.reshape(-1), data.reshape(-1)))
    if dense:
        return out, [np.asfortranarray(csr_to_dense(a)) for a in out]
    return out


def random_rows(n, k, cplx, seed):
    """n rows of k entries at random columns (repeats allowed, unsorted), standard normal values."""
    rng = np.random.default_rng(seed)
    return CSR(n, np.arange(n + 1, dtype=np.int64) * k, rng.integers(0, n, n * k).astype(np.int32),
               _randn(rng, n * k, cplx))


def irregular(n, cplx, seed):
    """Row 0 empty, row 1 with all n columns stored (in random order), row 2 with one column three times, the other
    rows with 0 to 5 unsorted entries."""
    rng = np.random.default_rng(seed)
    rows = [np.zeros(0, dtype=np.int64), rng.permutation(n), np.array([5 % n, 1 % n, 5 % n, 5 % n])]
    for r in range(3, n):
        rows.append(rng.integers(0, n, rng.integers(0, 6)))
    rows = rows[:n]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    return CSR(n, indptr, np.concatenate(rows).astype(np.int32), _randn(rng, int(indptr[-1]), cplx))


def matvec_cases(cplx):
    """(name, CSR) of the kernel sweep: n = 257 (no multiple of any 256 / G) at 2, 9 and 40 entries per row (automatic
    G = 2, 16, 64), n = 1, and the irregular matrix."""
    return [("k2", random_rows(257, 2, cplx, 1)), ("k9", random_rows(257, 9, cplx, 2)),
            ("k40", random_rows(257, 40, cplx, 3)), ("n1", random_rows(1, 1, cplx, 4)),
            ("irregular", irregular(257, cplx, 5))]


def check_matvec(eng, csr, cplx, seed=0):
    """y = A x at every group width against csr_matmat.  Row i is within 8 (nnz_i + 2) eps (|A| |x|)_i: the
    dot-product bound gamma_m = m eps / (1 - m eps) holds for any summation order, fused or not, and is taken once for
    each of the two computed values; a complex product adds a factor 2 sqrt(2) < 4 (both sides).  Empty rows: exactly 0."""
    rng = np.random.default_rng(100 + seed)
    x = _randn(rng, csr.n, cplx)
    ref = csr_matmat(csr, x)
    bound = 8 * (np.diff(csr.indptr) + 2) * EPS * csr_matmat(csr, x, absolute=True)
    empty = np.diff(csr.indptr) == 0
    worst = 0.0
    for g in GROUPS:
        y = eng.csr_matvec(csr, x, group=g)
        assert y.shape == ref.shape and np.iscomplexobj(y) == cplx
        err = np.abs(y - ref)
        assert np.all(err <= bound), (g, float(np.max(err - bound)))
        assert np.all(y[empty] == 0), g
        worst = max(worst, float(np.max(err / np.maximum(bound, np.finfo(float).tiny))))
    return worst


# (n, p, k, cplx) of the driver cases, and the call every one of them makes
DRIVER_SHAPES = [(300, 4, 8, False), (300, 4, 8, True), (257, 3, 2, False), (300, 2, 40, False)]
DRIVER_KW = dict(mindim=8, maxdim=16, tol=1e-10, restarts=100, seed=1)
NEV = 4
