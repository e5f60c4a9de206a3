"""periodicschurdecompositions.jl_amd — MI355X-native periodic Schur engine, host-side mirror.

The reference (RalphAS/PeriodicSchurDecompositions.jl) exposes `pschur`, `pschur!`, `phessenberg!`
and the `PeriodicSchur` result type as Julia methods (src/PeriodicSchurDecompositions.jl:11,59-152).
No Julia toolchain exists in the build/GPU images, so this module mirrors that interface — same
names (`!` spelled `_`), argument meaning and error behaviour — in Python over the C ABI of
`libpsd_mi355x.so` (include/psd_mi355x.h).  The Julia `ccall` wrapper a maintainer would add is in
INTEGRATION.md.

All numerical work happens in the HIP library.  There is no CPU fallback: if the library is
missing or no GPU is visible, `Engine()` raises.
"""
import collections
import copy
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpsd_mi355x.so")
# the diagnostic build (-DPSD_DIAG: timing experiments, tuning knobs, fault injection behind environment variables).
# Only tools/ and the fault-injection test pass it as `libpath`; the package itself never loads it.
DIAG_LIB_PATH = os.path.join(_HERE, "libpsd_mi355x_diag.so")

INFO_NOCONV = 1000000
INFO_NOTIMPL = 2000000
INFO_RUNTIME = 3000000


class NotImplementedPSD(Exception):
    """PeriodicSchurDecompositions.NotImplemented (src/PeriodicSchurDecompositions.jl:30)."""


class ConvergenceError(Exception):
    """ErrorException("convergence failed at level i") (src/PeriodicSchurDecompositions.jl:892)."""

    def __init__(self, level):
        super().__init__(f"convergence failed at level {level}")
        self.level = level


class IllConditionedException(Exception):
    """IllConditionedException(info) (src/PeriodicSchurDecompositions.jl:26-28)."""

    def __init__(self, info):
        super().__init__(f"IllConditionedException({info})")
        self.info = info


class SingularException(Exception):
    """LinearAlgebra.SingularException (src/utils.jl:123-131)."""


class DimensionMismatch(ValueError):
    """DimensionMismatch (src/PeriodicSchurDecompositions.jl:216-222)."""


class Stats(C.Structure):
    _fields_ = [
        ("niter", C.c_int64), ("maxits", C.c_int32), ("nsweeps", C.c_int32), ("nrqpass", C.c_int32),
        ("ndefl1", C.c_int32), ("ndefl2", C.c_int32), ("nwindows", C.c_int32), ("nlaunch_step", C.c_int32),
        ("window", C.c_int32), ("nlog", C.c_int32), ("ms_hess", C.c_double), ("ms_formq", C.c_double),
        ("ms_iter", C.c_double), ("ms_total", C.c_double), ("ms_copy", C.c_double), ("bytes_sweeps", C.c_double),
        ("bytes_hess", C.c_double), ("bytes_formq", C.c_double), ("step_kernel_ms_avg", C.c_double),
        ("step_kernel_samples", C.c_int32), ("reserved", C.c_int32), ("step_cycles", C.c_int64 * 6),
    ]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["step_cycles"] = list(self.step_cycles)
        return d


class PeriodicSchur:
    """Mirror of the reference's `PeriodicSchur` (src/PeriodicSchurDecompositions.jl:59-92).

    `T1` is the quasi-triangular factor (position `schurindex` in the user's sequence), `T` the
    remaining p-1 upper-triangular factors in order, `Z` the p orthogonal factors (empty if
    wantZ=False), `values` the eigenvalues of the product, `orientation` 'R' or 'L'.
    """

    def __init__(self, Ts, Z, values, orientation, schurindex, stats=None, sweeplog=None):
        self.Ts = Ts  # all p factors in user order (T1 included)
        self.Z = Z
        self.values = values
        self.orientation = orientation
        self.schurindex = schurindex
        self.stats = stats
        self.sweeplog = sweeplog

    @property
    def T1(self):
        return self.Ts[self.schurindex - 1]

    @property
    def T(self):
        return [t for j, t in enumerate(self.Ts) if j != self.schurindex - 1]

    @property
    def period(self):  # src/PeriodicSchurDecompositions.jl:85-91
        return len(self.Ts)


def _scaled_values(alpha, beta, alphascale):
    """values = alpha ./ beta .* 2 .^ alphascale (src/generalized.jl:31-85), for one problem or a batch of them."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return alpha / beta * np.exp2(alphascale.astype(np.float64))


class GeneralizedPeriodicSchur(PeriodicSchur):
    """Mirror of `GeneralizedPeriodicSchur` (src/generalized.jl:31-85): eigenvalues in scaled form
    `values = alpha ./ beta .* 2 .^ alphascale`."""

    def __init__(self, S, Ts, Z, alpha, beta, alphascale, orientation, schurindex, stats=None, sweeplog=None):
        values = _scaled_values(alpha, beta, alphascale)
        super().__init__(Ts, Z, values, orientation, schurindex, stats, sweeplog)
        self.S = list(S)
        self.alpha, self.beta, self.alphascale = alpha, beta, alphascale


class KrylovStats(C.Structure):
    """psd_krylov_stats (include/psd_mi355x.h): History fields and counters of one partial_pschur call."""
    _fields_ = [
        ("nprods", C.c_int64), ("nconverged", C.c_int32), ("converged", C.c_int32), ("nev", C.c_int32),
        ("restarts", C.c_int32), ("nreorth", C.c_int32), ("nreinit", C.c_int32), ("ndeflate", C.c_int32),
        ("suspect", C.c_int32), ("ms_arnoldi", C.c_double), ("ms_proj", C.c_double), ("ms_basis", C.c_double),
        ("ms_total", C.c_double),
    ]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KrylovGeom(C.Structure):
    """psd_krylov_geom (include/psd_mi355x.h): launch geometry of the dense Krylov kernels."""
    _fields_ = [("rp", C.c_int32), ("tiles", C.c_int32), ("nchunk", C.c_int32), ("ccols", C.c_int32),
                ("nblk", C.c_int32), ("ldp", C.c_int32)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SylGeom(C.Structure):
    """psd_syl_geom (include/psd_mi355x.h): partition and grid of one update launch of the periodic Sylvester walk."""
    _fields_ = [("nI", C.c_int32), ("nJ", C.c_int32), ("nsb", C.c_int32), ("ndtiles", C.c_int32)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class EvecStats(C.Structure):
    """psd_evec_stats (include/psd_mi355x.h): counters and device times of one eigvecs call by back-substitution."""
    _fields_ = [
        ("nvec", C.c_int32), ("nperturbed", C.c_int32), ("nrescaled", C.c_int32), ("nzero", C.c_int32),
        ("ms_solve", C.c_double), ("ms_backtransform", C.c_double), ("ms_kernels", C.c_double),
    ]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BevecStats(C.Structure):
    """psd_bevec_stats (include/psd_mi355x.h): counters, launches and device times of one eigvecs_batch call."""
    _fields_ = [
        ("nb", C.c_int32), ("nvec_total", C.c_int32), ("nperturbed", C.c_int32), ("nrescaled", C.c_int32),
        ("nzero", C.c_int32), ("nlaunch", C.c_int32), ("ngroups", C.c_int32), ("reserved", C.c_int32),
        ("ms_solve", C.c_double), ("ms_backtransform", C.c_double), ("ms_kernels", C.c_double),
    ]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BcheckStats(C.Structure):
    """psd_bcheck_stats (include/psd_mi355x.h): counters, launches and device times of one checkpsd_batch call."""
    _fields_ = [
        ("nb", C.c_int32), ("nfail", C.c_int32), ("nlaunch", C.c_int32), ("ngroups", C.c_int32),
        ("ms_kernels", C.c_double), ("ms_copy", C.c_double),
    ]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_ct = C  # (psylvester_batch has an argument of the name C)


class BsylvStats(C.Structure):
    """psd_bsylv_stats (include/psd_mi355x.h): launches, estimator iterations and device times of one psylvester_batch
    or subspacecond_batch call."""
    _fields_ = [
        ("nb", C.c_int32), ("ngroups", C.c_int32), ("nsolve", C.c_int32), ("nnorms", C.c_int32),
        ("nest_steps", C.c_int32), ("nest_iter", C.c_int32), ("nsingular", C.c_int32), ("reserved", C.c_int32),
        ("ms_kernels", C.c_double), ("ms_copy", C.c_double),
    ]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SylvStats(C.Structure):
    """psd_sylv_stats (include/psd_mi355x.h): the tile walk, launches, estimator solves and device times of one
    psylvester or subspacecond call."""
    _fields_ = [
        ("tile", C.c_int32), ("ntiles", C.c_int32), ("ndiag", C.c_int32), ("nsolve", C.c_int32), ("nupdate", C.c_int32),
        ("nnorms", C.c_int32), ("nest_steps", C.c_int32), ("nest_solves", C.c_int32), ("nest_iter", C.c_int32),
        ("nsingular", C.c_int32),
        ("ms_solve", C.c_double), ("ms_update", C.c_double), ("ms_est", C.c_double), ("ms_copy", C.c_double),
    ]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PKSFailure(Exception):
    """PKSFailure (src/krylov.jl:21-23): the Arnoldi re-initialisation failed."""


class PartialPeriodicSchur(PeriodicSchur):
    """Mirror of `PartialPeriodicSchur` (src/krylov.jl:87-139): k Schur vectors of length n per factor, left
    orientation, A_l Z_l = Z_{l+1} T_l (l < p) and A_p Z_p = Z_1 T_p; `T1` = T_p (schurindex = p)."""

    def __init__(self, Ts, Z, values, stats=None):
        super().__init__(Ts, Z, values, "L", len(Ts), stats)


class History:
    """Mirror of `ArnoldiMethod.History`: matrix-vector products, converged count, converged flag, nev."""

    def __init__(self, mvproducts, nconverged, converged, nev):
        self.mvproducts, self.nconverged, self.converged, self.nev = mvproducts, nconverged, converged, nev

    def __repr__(self):
        return (f"History(mvproducts={self.mvproducts}, nconverged={self.nconverged}, converged={self.converged}, "
                f"nev={self.nev})")


# partial_pschur targets (ArnoldiMethod's LM / LR / SR / LI / SI) as the ABI's char codes
KRYLOV_TARGETS = {"LM": "M", "LR": "R", "SR": "r", "LI": "I", "SI": "i"}

# psd_diag_scalar_op (include/psd_mi355x.h): the ops of the scalar diagnostic entry, by name
DIAG_SCALAR_OPS = {nm: k for k, nm in enumerate(
    ("rcp", "sqrt_pair", "rsqrt2", "refl2", "refl3", "refl2_lean", "refl3_lean", "refl32_pair", "reflector_small",
     "h2_larfg", "zh2_larfg", "givens", "zgivens", "zgivens_lean", "c3_scale"))}


# One sparse factor of partial_pschur in CSR form: order n, row pointers (n + 1), column indices and values (0-based).
CSR = collections.namedtuple("CSR", "n indptr indices data")


def _is_torch_csr(a):
    return type(a).__module__.split(".")[0] == "torch" and str(getattr(a, "layout", "")) == "torch.sparse_csr"


def _host_csr(a):
    """A sparse factor given on the host as a CSR tuple, or None: a `CSR` (or any (n, indptr, indices, data)), a bare
    (indptr, indices, data) of a square matrix, or an object with .indptr / .indices / .data / .shape and
    format == "csr" (scipy's csr_matrix / csr_array, by duck typing); other scipy formats through their own .tocsr()."""
    if isinstance(a, tuple) and len(a) == 4:
        return CSR(int(a[0]), *a[1:])
    if isinstance(a, tuple) and len(a) == 3:
        return CSR(len(a[0]) - 1, *a)
    fmt = getattr(a, "format", None)
    if isinstance(fmt, str) and fmt != "csr" and hasattr(a, "tocsr"):
        a = a.tocsr()
        fmt = getattr(a, "format", None)
    if fmt == "csr" and all(hasattr(a, k) for k in ("indptr", "indices", "data", "shape")):
        if len(a.shape) != 2 or a.shape[0] != a.shape[1]:
            raise DimensionMismatch("all As must have the same (square) size")  # krylov.jl:460-464
        return CSR(int(a.shape[0]), a.indptr, a.indices, a.data)
    return None


def _csr_arrays(a, dt):
    """(indptr int64, indices int32, data dt) of a host CSR factor, contiguous.  Column indices that int32 cannot hold
    are clamped to -1 / n, which the library reports as out of range."""
    if a.n < 1:
        raise DimensionMismatch("all As must have the same (square) size")
    indptr = np.ascontiguousarray(np.asarray(a.indptr).reshape(-1), dtype=np.int64)
    ind = np.asarray(a.indices).reshape(-1)
    if ind.dtype != np.int32:
        ind = np.clip(ind.astype(np.int64), -1, a.n).astype(np.int32)
    data = np.ascontiguousarray(np.asarray(a.data).reshape(-1), dtype=dt)
    if indptr.shape[0] != a.n + 1:
        raise DimensionMismatch("all As must have the same (square) size")
    if ind.shape[0] != data.shape[0] or indptr[-1] > ind.shape[0]:
        raise ValueError("invalid CSR row pointers (indptr): the last entry exceeds the stored entries")
    return indptr, np.ascontiguousarray(ind), data


_CSR_ERRORS = {-19: "invalid CSR row pointers (indptr): they must start at 0, not decrease and end at the entry count",
               -20: "CSR column index outside [0, n)"}


def char_lr(lr):
    """src/PeriodicSchurDecompositions.jl:155-163,175-177."""
    if lr in ("R", ":R"):
        return "R"
    if lr in ("L", ":L"):
        return "L"
    raise ValueError("orientation argument must be either :R (right) or :L (left)")


def _check_square(A):
    """src/PeriodicSchurDecompositions.jl:214-222."""
    if len(A) == 0:
        raise DimensionMismatch("empty sequence")
    n = A[0].shape[0]
    for a in A:
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise DimensionMismatch("matrices must be square")
        if a.shape[0] != n:
            raise DimensionMismatch("matrices must have equal order")
    return n


# What the Float64 and the ComplexF64 batch entries differ by: the ABI prefix, the numpy dtype (torch's has the same
# name), and how the pschur entries of the family turn away a problem of the other one.
_Family = collections.namedtuple("_Family", "tag dtype wrong_exc wrong_text")
_D = _Family("d", np.float64, NotImplementedPSD, "pschur_batch: Float64 only (ComplexF64 problems: zpschur_batch)")
_Z = _Family("z", np.complex128, TypeError, "zpschur_batch: ComplexF64 only (use pschur_batch for Float64 problems)")
# the Float64 SIGNED entries (psd_d_gp*_batch): the ABI prefix and dtype of _D, the scaled eigenvalues, the
# GeneralizedPeriodicSchur results and the per-problem codes of the ComplexF64 entries
_DG = _Family("d", np.float64, TypeError, "dgpschur_batch: Float64 only (ComplexF64 problems: zgpschur_batch)")


_ORD_WRONG = {_D: "ordschur_batch: Float64 only (use ordschur_ per problem for ComplexF64)",
              _Z: "zordschur_batch: ComplexF64 only (Float64 problems: ordschur_batch)"}
_GORD_WRONG = {_Z: "zgordschur_batch: ComplexF64 only (Float64 problems: dgordschur_batch)",
               _DG: "dgordschur_batch: Float64 only (ComplexF64 problems: zgordschur_batch)"}


def _other_family(fam, cplx, every=False):
    """Whether matrices (`cplx`: which of them are complex) belong to the other family: a complex one among Float64;
    among ComplexF64 none complex, or with `every` not all (one complex matrix makes a problem complex: the in-place
    contract turns the real ones away afterwards)."""
    return any(cplx) if fam.dtype is np.float64 else not (all(cplx) if every else any(cplx))


def _eig_alloc(fam, shape, nan=False):
    """The eigenvalue outputs of a batch call in ABI order, (wr, wi) or (alpha, beta, alphascale); `nan`: pre-filled
    so that a row the library does not write reads NaN."""
    if fam is _D:
        return [np.full(shape, np.nan) if nan else np.zeros(shape), np.zeros(shape)]
    return [np.full(shape, np.nan if nan else 0.0, dtype=np.complex128), np.ones(shape) if nan else np.zeros(shape),
            np.zeros(shape, dtype=np.int32)]


def _eig_values(eig):
    """`values` from the eigenvalue arguments of either family."""
    return eig[0] + 1j * eig[1] if len(eig) == 2 else _scaled_values(*eig)


def _dev_blocks(X, fam, policy):
    """[nb][p][n][n] blocks of column-major matrices from an [nb, p, n, n] tensor: the transpose of each factor,
    contiguous (as partial_pschur), which is what the device entries return a transposed view of.  `policy`:
      "copy":              always a fresh copy, the caller's tensor is never modified (pschur);
      "inplace_if_blocks": a tensor that already is such a view, of the family's dtype, is used as it is and written
                           IN PLACE; any other layout is copied and stays as it was (ordschur);
      "readonly":          the blocks are only read: a copy only where .to() / .contiguous() need one (eigvecs)."""
    import torch

    dt = getattr(torch, np.dtype(fam.dtype).name)
    if policy == "inplace_if_blocks" and X.dtype == dt and X.transpose(2, 3).is_contiguous():
        return X.transpose(2, 3)
    dX = X.to(dt).transpose(2, 3).contiguous()
    if policy == "copy" and dX.data_ptr() == X.data_ptr():
        dX = dX.clone()
    return dX


class Engine:
    """One device context (stream + workspace). One call at a time per Engine."""

    def __init__(self, device=0, libpath=None):
        path = libpath or LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        self.lib = lib = C.CDLL(path)
        dp, dpp = C.POINTER(C.c_double), C.POINTER(C.c_void_p)
        ip = C.POINTER(C.c_int)
        lib.psd_version.restype = C.c_char_p
        lib.psd_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        lib.psd_destroy.argtypes = [C.c_void_p]
        lib.psd_set_profile.argtypes = [C.c_void_p, C.c_int]
        lib.psd_d_phessenberg.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, dp, C.POINTER(Stats), ip]
        lib.psd_d_pschur.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, C.POINTER(C.c_uint8), C.c_char, C.c_int,
                                     C.c_int, C.c_int, dpp, dp, dp, ip, C.POINTER(Stats), C.POINTER(C.c_int32),
                                     C.c_int64, ip]
        lib.psd_d_pschur_hess.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, dpp, C.c_int, C.c_int, C.c_int, dp, dp,
                                          C.POINTER(Stats), C.POINTER(C.c_int32), C.c_int64, ip]
        lib.psd_d_pschur_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_char, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, dp, dp, ip, C.POINTER(Stats), C.POINTER(C.c_int32), C.c_int64, ip]
        i32p = C.POINTER(C.c_int32)
        lib.psd_z_phessenberg.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, dp, C.POINTER(Stats), ip]
        lib.psd_z_pschur.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, C.POINTER(C.c_uint8), C.c_char, C.c_int,
                                     C.c_int, C.c_int, dpp, dp, dp, i32p, ip, C.POINTER(Stats), i32p, C.c_int64, ip]
        lib.psd_z_pschur_hess.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, C.POINTER(C.c_uint8), dpp, C.c_int,
                                          C.c_int, C.c_int, dp, dp, i32p, C.POINTER(Stats), i32p, C.c_int64, ip]
        lib.psd_d_gpschur_hess.argtypes = lib.psd_z_pschur_hess.argtypes
        lib.psd_d_gphessenberg.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, C.POINTER(C.c_uint8), dpp,
                                           C.POINTER(Stats), ip]
        lib.psd_z_gphessenberg.argtypes = lib.psd_d_gphessenberg.argtypes
        lib.psd_d_rphessenberg.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, dpp, dpp, C.c_int, C.c_int, ip]
        lib.psd_z_rphessenberg.argtypes = lib.psd_d_rphessenberg.argtypes
        lib.psd_d_gpschur.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, C.POINTER(C.c_uint8), C.c_char, C.c_int,
                                      C.c_int, C.c_int, dpp, dp, dp, i32p, ip, C.POINTER(Stats), ip]
        lib.psd_z_pschur_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_char, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, dp, dp, i32p, ip, C.POINTER(Stats), i32p, C.c_int64, ip]
        lib.psd_z_ordschur.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, dpp, C.c_char, C.c_int, C.POINTER(C.c_uint8),
                                       C.c_int, dp, dp, i32p, C.POINTER(Stats), ip]
        lib.psd_z_gordschur.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, dpp, C.POINTER(C.c_uint8), C.c_char, C.c_int,
                                        C.POINTER(C.c_uint8), C.c_int, dp, dp, i32p, C.POINTER(Stats), ip]
        lib.psd_d_gordschur.argtypes = lib.psd_z_gordschur.argtypes
        lib.psd_d_ordschur.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, dpp, C.c_char, C.c_int, C.POINTER(C.c_uint8),
                                       C.c_int, dp, dp, C.POINTER(Stats), ip]
        u8p = C.POINTER(C.c_uint8)
        lib.psd_d_checkpsd.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, dpp, dpp, u8p, C.c_char, C.c_int, dp,
                                       C.c_double, C.c_int, dp, dp, dp, ip, ip]
        lib.psd_z_checkpsd.argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, dpp, dpp, u8p, C.c_char, C.c_int,
                                       C.c_double, C.c_int, dp, dp, dp, ip, ip]
        lib.psd_d_checkpsd_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, u8p,
                                           C.c_char, C.c_int, C.c_double, C.c_int, dp, dp, dp, ip, ip]
        if hasattr(lib, "psd_z_checkpsd_dev"):  # (tools load builds of earlier commits)
            lib.psd_z_checkpsd_dev.argtypes = lib.psd_d_checkpsd_dev.argtypes
        # the batch entries: one description per entry family, crossed with d / z (the eigenvalue arguments), plain /
        # signed (the signature after the factors) and host / dev (how the matrices are passed).  The signed pschur and
        # ordschur entries of both types return scaled eigenvalues (alpha, beta, alphascale).
        sp, head = C.POINTER(Stats), [C.c_void_p, C.c_int, C.c_int, C.c_int]  # (head: ctx, nb, n, p)
        for t, eig in (("d", [dp, dp]), ("z", [dp, dp, i32p])):
            sigs = {f"psd_{t}_phessenberg_batch": head + [dpp, dp, sp, ip],
                    f"psd_{t}_gphessenberg_batch": head + [dpp, u8p, dpp, sp, ip]}
            for g, sig, ge in (("", [], eig), ("g", [u8p], [dp, dp, i32p])):
                sigs[f"psd_{t}_{g}pschur_hess_batch"] = (head + [dpp] + sig + [dpp, C.c_int, C.c_int, C.c_int] + ge
                                                         + [ip, sp, ip])
            for dev, mats in (("", dpp), ("_dev", C.c_void_p)):
                for g, sig, ge in (("", [], eig), ("g", [u8p], [dp, dp, i32p])):
                    sigs[f"psd_{t}_{g}pschur_batch{dev}"] = (head + [mats] + sig + [C.c_char, C.c_int, C.c_int, C.c_int,
                                                                                     mats] + ge + [ip, ip, sp, ip])
                    sigs[f"psd_{t}_{g}ordschur_batch{dev}"] = (head + [mats, mats] + sig + [C.c_char, C.c_int, u8p, C.c_int]
                                                               + ge + [ip, ip, sp, ip])
                sigs[f"psd_{t}_eigvecs_batch{dev}"] = (head + [mats, mats] + eig + [C.c_char, C.c_int, u8p, C.c_int, mats,
                                                                                    C.c_int, ip, i32p,
                                                                                    C.POINTER(BevecStats), ip])
                sigs[f"psd_{t}_leigvecs_batch{dev}"] = sigs[f"psd_{t}_eigvecs_batch{dev}"]  # (the left vectors)
                sigs[f"psd_eigcond_batch{dev}"] = head + [mats, mats, C.c_char, C.c_int, ip, dp, ip]
                # (no eigenvalue arguments: the signature, and the scalars a behind maxvec)
                sigs[f"psd_{t}_geigvecs_batch{dev}"] = (head + [mats, mats, u8p, C.c_char, C.c_int, u8p, C.c_int, mats,
                                                                C.c_int, dp, ip, i32p, C.POINTER(BevecStats), ip])
                sigs[f"psd_{t}_checkpsd_batch{dev}"] = (head + [mats, mats, mats, u8p, C.c_char, C.c_int, C.c_double,
                                                                C.c_int, dp, dp, dp, i32p, C.POINTER(BcheckStats), ip])
                # (T, orient, schurindex, m, then C, xb, trans, from_t12 / s, sep, X, xb)
                sigs[f"psd_{t}_psylv_batch{dev}"] = (head + [mats, C.c_char, C.c_int, ip, mats, C.c_int64, C.c_int, C.c_int,
                                                             ip, C.POINTER(BsylvStats), ip])
                sigs[f"psd_{t}_subcond_batch{dev}"] = (head + [mats, C.c_char, C.c_int, ip, dp, dp, mats, C.c_int64, ip,
                                                               C.POINTER(BsylvStats), ip])
                # (the single-problem entries: no nb, xb and infos, m one int)
                one = [C.c_void_p, C.c_int, C.c_int, mats, C.c_char, C.c_int, C.c_int]
                sigs[f"psd_{t}_psylv{dev}"] = one + [mats, C.c_int, C.c_int, C.POINTER(SylvStats), ip]
                sigs[f"psd_{t}_subcond{dev}"] = one + [dp, dp, mats, C.POINTER(SylvStats), ip]
            # (test plumbing: X, tile, d, trans, from_t12, geom, bounds)
            sigs[f"psd_{t}_syl_update"] = ([C.c_void_p, C.c_int, C.c_int, dpp, C.c_char, C.c_int, C.c_int, dpp, C.c_int,
                                            C.c_int, C.c_int, C.c_int, C.POINTER(SylGeom), C.POINTER(C.c_int32), ip])
            for nm, sig in sigs.items():
                if hasattr(lib, nm):  # (tools load builds of earlier commits to time their single calls)
                    getattr(lib, nm).argtypes = sig
        lib.psd_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.psd_shard_owned.argtypes = [C.c_void_p, C.c_int, C.c_char, u8p]
        for nm, dev in (("psd_d_partial_pschur", False), ("psd_z_partial_pschur", False),
                        ("psd_d_partial_pschur_dev", True), ("psd_z_partial_pschur_dev", True)):
            getattr(lib, nm).argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p if dev else dpp, C.c_int, C.c_char,
                                         C.c_int, C.c_int, dp, C.c_uint64, C.c_double, C.c_double, C.c_int, C.c_int,
                                         ip, dpp, C.c_void_p if dev else dpp, dp, dp, C.POINTER(KrylovStats), ip]
        for nm, dev in (("psd_d_partial_pschur_csr", False), ("psd_z_partial_pschur_csr", False),
                        ("psd_d_partial_pschur_csr_dev", True), ("psd_z_partial_pschur_csr_dev", True)):
            getattr(lib, nm).argtypes = [C.c_void_p, C.c_int, C.c_int, dpp, dpp, dpp, C.c_int, C.c_char, C.c_int, C.c_int,
                                         dp, C.c_uint64, C.c_double, C.c_double, C.c_int, C.c_int, ip, dpp,
                                         C.c_void_p if dev else dpp, dp, dp, C.POINTER(KrylovStats), ip]
        lib.psd_d_csr_matvec.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, dp, dp, C.c_int, ip]
        lib.psd_z_csr_matvec.argtypes = lib.psd_d_csr_matvec.argtypes
        if hasattr(lib, "psd_d_dense_matvec"):  # (tools load builds of earlier commits)
            lib.psd_d_dense_matvec.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, dp, dp, C.POINTER(KrylovGeom), ip]
            lib.psd_z_dense_matvec.argtypes = lib.psd_d_dense_matvec.argtypes
            lib.psd_d_kr_orth.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp, dp, dp, dp, C.POINTER(C.c_int32), ip]
            lib.psd_z_kr_orth.argtypes = lib.psd_d_kr_orth.argtypes
            lib.psd_d_kr_basis.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp,
                                           C.POINTER(C.c_int32), ip]
            lib.psd_z_kr_basis.argtypes = lib.psd_d_kr_basis.argtypes
        if hasattr(lib, "psd_diag_scalar"):
            lib.psd_diag_scalar.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp, ip]
        i32p = C.POINTER(C.c_int32)
        for nm, dev, cplx in (("psd_d_eigvecs", False, False), ("psd_z_eigvecs", False, True),
                              ("psd_d_eigvecs_dev", True, False), ("psd_z_eigvecs_dev", True, True)):
            mats = C.c_void_p if dev else dpp
            vals = [dp, dp, i32p] if cplx else [dp, dp]
            getattr(lib, nm).argtypes = ([C.c_void_p, C.c_int, C.c_int, mats, mats] + vals +
                                         [u8p, C.c_char, C.c_int, u8p, C.c_int, C.c_int, mats, C.c_int,
                                          C.POINTER(EvecStats), ip])
        for nm, dev in (("psd_d_geigvecs", False), ("psd_z_geigvecs", False), ("psd_d_geigvecs_dev", True),
                        ("psd_z_geigvecs_dev", True)):
            mats = C.c_void_p if dev else dpp
            getattr(lib, nm).argtypes = [C.c_void_p, C.c_int, C.c_int, mats, mats, u8p, C.c_char, C.c_int, u8p, C.c_int,
                                         C.c_int, mats, C.c_int, dp, C.POINTER(EvecStats), ip]
        self.ctx = C.c_void_p()
        rc = lib.psd_create(C.byref(self.ctx), device)
        if rc != 0:
            raise RuntimeError(f"psd_create failed (info={rc}): no usable HIP device; there is no CPU fallback")

    def version(self):
        return self.lib.psd_version().decode()

    def set_train(self, bulges):
        """Multishift trains of the real pschur! path (psd_set_train): bulges >= 2 (default 32) or 0 for the reference's
        one-shift-one-sweep iteration."""
        self.lib.psd_set_train.argtypes = [C.c_void_p, C.c_int]
        self.lib.psd_set_train(self.ctx, int(bulges))

    def set_train_z(self, bulges):
        self.lib.psd_set_train_z.argtypes = [C.c_void_p, C.c_int]
        self.lib.psd_set_train_z(self.ctx, int(bulges))

    def get_train_z(self):
        self.lib.psd_get_train_z.argtypes = [C.c_void_p]
        return int(self.lib.psd_get_train_z(self.ctx))

    def set_train_g(self, bulges):
        """Multishift trains of the signed paths, real and complex (psd_set_train_g; default 32; 0 = the reference's iteration)."""
        self.lib.psd_set_train_g.argtypes = [C.c_void_p, C.c_int]
        self.lib.psd_set_train_g(self.ctx, int(bulges))

    def get_train_g(self):
        self.lib.psd_get_train_g.argtypes = [C.c_void_p]
        return int(self.lib.psd_get_train_g(self.ctx))

    def get_train(self):
        self.lib.psd_get_train.argtypes = [C.c_void_p]
        return int(self.lib.psd_get_train(self.ctx))

    def set_slices(self, slices):
        """Factor-sliced sweep windows of the real engine (psd_set_slices): `slices` workgroups per window, each with the
        window blocks of its contiguous slice of the period; 1 = off."""
        self.lib.psd_set_slices.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.psd_set_slices(self.ctx, int(slices))
        if rc != 0:
            raise ValueError(f"psd_set_slices({slices}): argument {-rc} invalid")

    def get_slices(self):
        self.lib.psd_get_slices.argtypes = [C.c_void_p]
        return int(self.lib.psd_get_slices(self.ctx))

    def hess_pipe(self):
        """1 if this engine's multi-stream Hessenberg reductions take the pipe form (psd_get_hess_pipe): fixed at
        creation, forced on by set_shard with world > 1."""
        self.lib.psd_get_hess_pipe.argtypes = [C.c_void_p]
        return int(self.lib.psd_get_hess_pipe(self.ctx))

    def set_shard(self, rank, world):
        """Period sharding (include/psd_mi355x.h, psd_set_shard): this engine keeps the Schur vectors Z_j of its
        contiguous slice of the period; the chains and the factors are computed identically on every rank."""
        rc = self.lib.psd_set_shard(self.ctx, int(rank), int(world))
        if rc != 0:
            raise ValueError(f"psd_set_shard({rank}, {world}): argument {-rc} invalid")
        self.shard = (int(rank), int(world))

    def owned_slots(self, p, lr="R"):
        """Boolean mask over the user slots of Z that this (sharded) engine holds after a call with orientation lr."""
        owned = (C.c_uint8 * p)()
        rc = self.lib.psd_shard_owned(self.ctx, p, char_lr(lr).encode(), owned)
        if rc != 0:
            raise ValueError(f"psd_shard_owned: argument {-rc} invalid")
        return np.array([bool(x) for x in owned])

    def set_profile(self, on):
        self.lib.psd_set_profile(self.ctx, int(on))

    def close(self):
        if self.ctx:
            self.lib.psd_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------------------------------
    @staticmethod
    def _ptrs(mats):
        arr = (C.c_void_p * len(mats))()
        for j, a in enumerate(mats):
            arr[j] = a.ctypes.data
        return arr

    @staticmethod
    def _raise(info):
        if info == 0:
            return
        if info < 0:
            raise ValueError(f"argument {-info} invalid")
        if info >= INFO_RUNTIME:
            raise RuntimeError(f"HIP runtime failure (code {info - INFO_RUNTIME})")
        if info >= INFO_NOTIMPL:
            raise NotImplementedPSD("not implemented in this build")
        if info >= INFO_NOCONV:
            raise ConvergenceError(info - INFO_NOCONV)
        raise RuntimeError(f"info={info}")

    @staticmethod
    def _as_work(A, dtype=np.float64):
        """In-place contract: every A[j] must be a Fortran-contiguous matrix of `dtype` we may overwrite."""
        for a in A:
            if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.f_contiguous and a.flags.writeable):
                raise TypeError(f"needs writable Fortran-ordered {np.dtype(dtype).name} matrices (use pschur for a copy)")

    @staticmethod
    def _is_complex(A):
        return any(np.iscomplexobj(a) for a in A)

    def phessenberg_(self, A):
        """phessenberg!(A) — src/PeriodicSchurDecompositions.jl:213-259.
        Overwrites A LAPACK-style; returns (H list, tau[p][n]) where H[0] = triu(A[0],-1), H[j] = triu(A[j])."""
        n = _check_square(A)
        if self._is_complex(A):
            self._as_work(A, np.complex128)
            p = len(A)
            tau = np.zeros((p, n), dtype=np.complex128)
            st = Stats()
            info = C.c_int(0)
            self.lib.psd_z_phessenberg(self.ctx, n, p, self._ptrs(A), tau.view(np.float64).ctypes.data_as(
                C.POINTER(C.c_double)), C.byref(st), C.byref(info))
            self._raise(info.value)
            return [np.triu(a, -1 if j == 0 else 0) for j, a in enumerate(A)], tau, st
        self._as_work(A)
        p = len(A)
        tau = np.zeros((p, n))
        st = Stats()
        info = C.c_int(0)
        self.lib.psd_d_phessenberg(self.ctx, n, p, self._ptrs(A), tau.ctypes.data_as(C.POINTER(C.c_double)),
                                   C.byref(st), C.byref(info))
        self._raise(info.value)
        Hs = [np.triu(a, -1 if j == 0 else 0) for j, a in enumerate(A)]
        return Hs, tau, st

    def pschur_(self, A, lr="R", S=None, wantZ=True, wantT=True, maxitfac=30):
        """pschur!(A, lr; wantZ, wantT, maxitfac) — src/PeriodicSchurDecompositions.jl:120-152.
        `A` is workspace and is overwritten with the T factors."""
        orient = char_lr(lr)
        n = _check_square(A)
        if self._is_complex(A):
            return self._zpschur_(A, orient, S, wantZ, wantT, maxitfac)
        self._as_work(A)
        p = len(A)
        if S is not None:  # pschur!(A, S, lr) — src/rgeneralized.jl:3-45 (also for all(S), as the reference)
            return self._gpschur_(A, S, orient, wantZ, wantT, 120 if maxitfac == 30 else maxitfac)
        Z = [np.zeros((n, n), order="F") for _ in range(p)] if wantZ else []
        wr = np.zeros(n)
        wi = np.zeros(n)
        si = C.c_int(0)
        st = Stats()
        maxlog = 2 * maxitfac * n + n + 16
        log = np.zeros(3 * maxlog, dtype=np.int32)
        info = C.c_int(0)
        Sarr = None
        if S is not None:
            if len(S) != p:
                raise DimensionMismatch("length of S must match the period")
            Sarr = (C.c_uint8 * p)(*[1 if s else 0 for s in S])
        dp = C.POINTER(C.c_double)
        self.lib.psd_d_pschur(self.ctx, n, p, self._ptrs(A), Sarr, orient.encode(), int(wantT), int(wantZ), int(maxitfac),
                              self._ptrs(Z) if wantZ else None, wr.ctypes.data_as(dp), wi.ctypes.data_as(dp),
                              C.byref(si), C.byref(st), log.ctypes.data_as(C.POINTER(C.c_int32)), maxlog,
                              C.byref(info))
        self._raise(info.value)
        nl = min(st.nlog, maxlog)
        return PeriodicSchur(list(A), Z, wr + 1j * wi, orient, si.value, st, log[: 3 * nl].reshape(-1, 3).copy())

    def _gpschur_(self, A, S, orient, wantZ, wantT, maxitfac):
        """pschur!(A, S, lr; wantZ, wantT) for Float64 — src/rgeneralized.jl:3-45 -> GeneralizedPeriodicSchur."""
        n = A[0].shape[0]
        p = len(A)
        if len(S) != p:
            raise DimensionMismatch("length of S must match the period")
        first = S[p - 1] if orient == "L" else S[0]
        if not first:
            raise ValueError("The leftmost entry in S must be true")  # src/rgeneralized.jl:37
        Z = [np.zeros((n, n), order="F") for _ in range(p)] if wantZ else []
        alpha = np.zeros(n, dtype=np.complex128)
        beta = np.zeros(n)
        sc = np.zeros(n, dtype=np.int32)
        si = C.c_int(0)
        st = Stats()
        info = C.c_int(0)
        Sarr = (C.c_uint8 * p)(*[1 if x else 0 for x in S])
        dp = C.POINTER(C.c_double)
        self.lib.psd_d_gpschur(self.ctx, n, p, self._ptrs(A), Sarr, orient.encode(), int(wantT), int(wantZ),
                               int(maxitfac), self._ptrs(Z) if wantZ else None,
                               alpha.view(np.float64).ctypes.data_as(dp), beta.ctypes.data_as(dp),
                               sc.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(si), C.byref(st), C.byref(info))
        self._raise(info.value)
        return GeneralizedPeriodicSchur(list(S), list(A), Z, alpha, beta, sc, orient, si.value, st, None)

    def gphessenberg_(self, A, S, wantQ=True):
        """_phessenberg!(A, S; wantQ) for Float64 / ComplexF64 — src/generalized.jl:988-1082.  Overwrites A with the Hessenberg /
        triangular factors; returns (A, Qs)."""
        n = _check_square(A)
        cplx = self._is_complex(A)
        dt = np.complex128 if cplx else np.float64
        self._as_work(A, dt)
        p = len(A)
        if len(S) != p:
            raise DimensionMismatch("length of S must match the period")
        if not S[0]:
            raise ValueError("The leftmost entry in S must be true")  # src/generalized.jl:990
        Q = [np.zeros((n, n), dtype=dt, order="F") for _ in range(p)] if wantQ else []
        st = Stats()
        info = C.c_int(0)
        Sarr = (C.c_uint8 * p)(*[1 if x else 0 for x in S])
        fn = self.lib.psd_z_gphessenberg if cplx else self.lib.psd_d_gphessenberg
        fn(self.ctx, n, p, self._ptrs(A), Sarr, self._ptrs(Q) if wantQ else None, C.byref(st), C.byref(info))
        self._raise(info.value)
        self.last_stats = st
        return list(A), Q

    def rphessenberg_(self, Ap, A, Q=None):
        """_rphessenberg!(Ap, A, Q) — src/rhessx.jl:55-109 (Float64 / ComplexF64): row-wise periodic Hessenberg reduction
        for the left orientation.  Ap: m x n with m in (n, n+1); A: p-1 matrices n x n; Q: p matrices with at least n
        columns that are post-multiplied (or None).  Everything is overwritten; returns (Ap, A)."""
        m, n = Ap.shape
        if m not in (n, n + 1):
            raise ValueError("only implemented for square or 1 extra row")  # src/rhessx.jl:62
        p = len(A) + 1
        for a in A:
            if a.shape != (n, n):
                raise DimensionMismatch("all factors must be n x n")  # src/rhessx.jl:66
        cplx = np.iscomplexobj(Ap)
        dt = np.complex128 if cplx else np.float64
        self._as_work([Ap] + list(A) + (list(Q) if Q is not None else []), dt)
        nq = nqc = 0
        if Q is not None:
            if len(Q) != p:
                raise DimensionMismatch("one Q per factor")
            nq, nqc = Q[0].shape
            if nqc < n or any(q.shape != (nq, nqc) for q in Q):
                raise DimensionMismatch("Q matrices must share a shape with at least n columns")
        info = C.c_int(0)
        fn = self.lib.psd_z_rphessenberg if cplx else self.lib.psd_d_rphessenberg
        fn(self.ctx, m, n, p, Ap.ctypes.data, self._ptrs(A) if p > 1 else None, self._ptrs(Q) if Q is not None else None,
           nq, nqc, C.byref(info))
        self._raise(info.value)
        return Ap, list(A)

    def _zpschur_(self, A, orient, S, wantZ, wantT, maxitfac):
        """pschur!(A::Vector{Matrix{ComplexF64}}[, S], lr) — src/PeriodicSchurDecompositions.jl:1106-1111,
        src/generalized.jl:108-148.  Without S the result is a PeriodicSchur (as at :1110)."""
        n = A[0].shape[0]
        self._as_work(A, np.complex128)
        p = len(A)
        Z = [np.zeros((n, n), dtype=np.complex128, order="F") for _ in range(p)] if wantZ else []
        alpha = np.zeros(n, dtype=np.complex128)
        beta = np.zeros(n)
        sc = np.zeros(n, dtype=np.int32)
        si = C.c_int(0)
        st = Stats()
        maxlog = 2 * maxitfac * n + n + 16
        log = np.zeros(3 * maxlog, dtype=np.int32)
        info = C.c_int(0)
        Sarr = None
        if S is not None:
            if len(S) != p:
                raise DimensionMismatch("length of S must match the period")
            first = S[p - 1] if orient == "L" else S[0]
            if not first:
                raise ValueError("The leftmost entry in S must be true")  # src/generalized.jl:140
            Sarr = (C.c_uint8 * p)(*[1 if x else 0 for x in S])
        dp = C.POINTER(C.c_double)
        self.lib.psd_z_pschur(self.ctx, n, p, self._ptrs(A), Sarr, orient.encode(), int(wantT), int(wantZ),
                              int(maxitfac), self._ptrs(Z) if wantZ else None,
                              alpha.view(np.float64).ctypes.data_as(dp), beta.ctypes.data_as(dp),
                              sc.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(si), C.byref(st),
                              log.ctypes.data_as(C.POINTER(C.c_int32)), maxlog, C.byref(info))
        self._raise(info.value)
        nl = min(st.nlog, maxlog)
        slog = log[: 3 * nl].reshape(-1, 3).copy()
        g = GeneralizedPeriodicSchur([True] * p if S is None else S, list(A), Z, alpha, beta, sc, orient, si.value, st,
                                     slog)
        if S is None:
            return PeriodicSchur(g.Ts, g.Z, g.values, g.orientation, g.schurindex, st, slog)
        return g

    def pschur(self, A, lr="R", **kw):
        """pschur(A, lr; kwargs...) — copying variant, src/PeriodicSchurDecompositions.jl:108-113."""
        dt = np.complex128 if self._is_complex(A) else np.float64
        Atmp = [np.array(a, dtype=dt, order="F", copy=True) for a in A]
        return self.pschur_(Atmp, lr, **kw)

    def gpschur(self, As, Bs, **kw):
        """gpschur(As, Bs) — src/generalized.jl:1191-1211: generalized periodic Schur decomposition for the formal
        product B_p^-1 A_p ... B_1^-1 A_1 of paired series in left operator order.  As the reference, the arguments are
        complexified and interleaved by `_mkpsargs` (:1198-1211) and handed to pschur!(Cs, Ss)."""
        ph = len(As)
        if len(Bs) != ph:
            raise DimensionMismatch("As and Bs must have the same length")
        cz = lambda m: np.array(m, dtype=np.complex128, order="F", copy=True)  # noqa: E731
        ib = 0 if ph == 1 else ph - 2
        Cs, Ss = [cz(As[ph - 1]), cz(Bs[ib])], [True, False]
        for j in range(ph - 1, 0, -1):  # j = ph-1 .. 1 (1-based)
            Cs.append(cz(As[j - 1]))
            jx = ph if j == 1 else j - 1
            Cs.append(cz(Bs[jx - 1]))
            Ss += [True, False]
        return self.pschur_(Cs, "R", S=Ss, **kw)

    def zpschur_hess_(self, H1, Hs, S=None, Q=None, wantT=True, wantZ=True, maxitfac=30, rev=False):
        """pschur!(H1, Hs, S; wantT, wantZ, Q, maxitfac, rev) for ComplexF64 — src/generalized.jl:166-175."""
        H = [H1] + list(Hs)
        n = _check_square(H)
        self._as_work(H, np.complex128)
        p = len(H)
        S = [True] * p if S is None else list(S)
        if not S[0]:
            raise ValueError("Signature entry S[1] must be true")  # src/generalized.jl:182
        if wantZ:
            if Q is None:
                Q = [np.asfortranarray(np.eye(n, dtype=np.complex128)) for _ in range(p)]
            self._as_work(Q, np.complex128)
        alpha = np.zeros(n, dtype=np.complex128)
        beta = np.zeros(n)
        sc = np.zeros(n, dtype=np.int32)
        st = Stats()
        maxlog = 2 * maxitfac * n + n + 16
        log = np.zeros(3 * maxlog, dtype=np.int32)
        info = C.c_int(0)
        Sarr = (C.c_uint8 * p)(*[1 if x else 0 for x in S])
        dp = C.POINTER(C.c_double)
        self.lib.psd_z_pschur_hess(self.ctx, n, p, self._ptrs(H), Sarr, self._ptrs(Q) if wantZ else None, int(wantT),
                                   int(wantZ), int(maxitfac), alpha.view(np.float64).ctypes.data_as(dp),
                                   beta.ctypes.data_as(dp), sc.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st),
                                   log.ctypes.data_as(C.POINTER(C.c_int32)), maxlog, C.byref(info))
        self._raise(info.value)
        nl = min(st.nlog, maxlog)
        slog = log[: 3 * nl].reshape(-1, 3).copy()
        Z = list(Q) if wantZ else []
        if rev:  # src/generalized.jl:910-927
            Zr = ([Z[0]] + [Z[p + 1 - l] for l in range(2, p + 1)]) if wantZ else Z
            Ts = [H[p - l] for l in range(1, p)] + [H[0]]
            return GeneralizedPeriodicSchur(S[::-1], Ts, Zr, alpha, beta, sc, "L", p, st, slog)
        return GeneralizedPeriodicSchur(S, H, Z, alpha, beta, sc, "R", 1, st, slog)

    def gpschur_hess_(self, H1, Hs, S, Q=None, wantT=True, wantZ=True, maxitfac=120, rev=False):
        """pschur!(H1, Hs, S; wantT, wantZ, Q, maxitfac, rev) for Float64 — src/rgeneralized.jl:49-59."""
        H = [H1] + list(Hs)
        n = _check_square(H)
        self._as_work(H)
        p = len(H)
        S = list(S)
        if len(S) != p:
            raise DimensionMismatch("S must have one entry per factor")
        if not S[0]:
            raise ValueError("Signature entry S[1] must be true")  # src/rgeneralized.jl:73
        if wantZ:
            if Q is None:
                Q = [np.asfortranarray(np.eye(n)) for _ in range(p)]
            self._as_work(Q)
        alpha = np.zeros(n, dtype=np.complex128)
        beta = np.zeros(n)
        sc = np.zeros(n, dtype=np.int32)
        st = Stats()
        maxlog = 2 * maxitfac * n + n + 16
        log = np.zeros(3 * maxlog, dtype=np.int32)
        info = C.c_int(0)
        Sarr = (C.c_uint8 * p)(*[1 if x else 0 for x in S])
        dp = C.POINTER(C.c_double)
        self.lib.psd_d_gpschur_hess(self.ctx, n, p, self._ptrs(H), Sarr, self._ptrs(Q) if wantZ else None, int(wantT),
                                    int(wantZ), int(maxitfac), alpha.view(np.float64).ctypes.data_as(dp),
                                    beta.ctypes.data_as(dp), sc.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st),
                                    log.ctypes.data_as(C.POINTER(C.c_int32)), maxlog, C.byref(info))
        self._raise(info.value)
        nl = min(st.nlog, maxlog)
        slog = log[: 3 * nl].reshape(-1, 3).copy()
        Z = list(Q) if wantZ else []
        if rev:  # src/rgeneralized.jl:1062-1079
            Zr = ([Z[0]] + [Z[p + 1 - l] for l in range(2, p + 1)]) if wantZ else Z
            Ts = [H[p - l] for l in range(1, p)] + [H[0]]
            return GeneralizedPeriodicSchur(S[::-1], Ts, Zr, alpha, beta, sc, "L", p, st, slog)
        return GeneralizedPeriodicSchur(S, H, Z, alpha, beta, sc, "R", 1, st, slog)

    def pschur_hess_(self, H1, Hs, Q=None, wantT=True, wantZ=True, maxitfac=30, rev=False):
        """pschur!(H1, Hs; wantT, wantZ, Q, maxitfac, rev) — src/PeriodicSchurDecompositions.jl:322-330."""
        H = [H1] + list(Hs)
        n = _check_square(H)
        self._as_work(H)
        p = len(H)
        if wantZ:
            if Q is None:
                Q = [np.asfortranarray(np.eye(n)) for _ in range(p)]
            self._as_work(Q)
        wr = np.zeros(n)
        wi = np.zeros(n)
        st = Stats()
        maxlog = 2 * maxitfac * n + n + 16
        log = np.zeros(3 * maxlog, dtype=np.int32)
        info = C.c_int(0)
        dp = C.POINTER(C.c_double)
        self.lib.psd_d_pschur_hess(self.ctx, n, p, self._ptrs(H), self._ptrs(Q) if wantZ else None, int(wantT),
                                   int(wantZ), int(maxitfac), wr.ctypes.data_as(dp), wi.ctypes.data_as(dp),
                                   C.byref(st), log.ctypes.data_as(C.POINTER(C.c_int32)), maxlog, C.byref(info))
        self._raise(info.value)
        nl = min(st.nlog, maxlog)
        lam = wr + 1j * wi
        Z = list(Q) if wantZ else []
        slog = log[: 3 * nl].reshape(-1, 3).copy()
        if rev:  # src/PeriodicSchurDecompositions.jl:1078-1092
            Zr = ([Z[0]] + [Z[p + 1 - l] for l in range(2, p + 1)]) if wantZ else Z
            Ts = [H[p - l] for l in range(1, p)] + [H[0]]
            return PeriodicSchur(Ts, Zr, lam, "L", p, st, slog)
        return PeriodicSchur(H, Z, lam, "R", 1, st, slog)

    # ---- The batch family (psd_?_*_batch): many small problems of one shape per call.  The Float64 and the ComplexF64
    # entries (in the iteration 32 problems side by side / one wavefront per problem) share the wrappers below; what
    # differs between them is an argument: the `_Family`, the text that turns the other family away, the rule for a
    # fatal call-wide code (`_batch_finish`), the copy policy of device tensors (`_dev_blocks`).
    def _batch_factors(self, fam, problems):
        """(n, p, flat list of factors) of a batch of general problems; DimensionMismatch unless all have one shape, the
        family's exception for a problem of the other one."""
        shape = None
        flat = []
        for A in problems:
            A = list(A)
            if len(A) < 1:
                raise DimensionMismatch("empty sequence")
            if _other_family(fam, [np.iscomplexobj(a) for a in A]):
                raise fam.wrong_exc(fam.wrong_text)
            shape = self._batch_shape(A, shape)
            flat += A
        return (*shape, flat)

    @staticmethod
    def _batch_shape(A, shape):
        """(n, p) of the factors A of one problem, which must be `shape` (None: the first problem of a batch)."""
        nq = _check_square(A)
        if shape is not None and (nq, len(A)) != shape:
            raise DimensionMismatch("the problems of a batch must have equal order and period")
        return nq, len(A)

    def _batch_hess(self, fam, problems, wantZ, wrong):
        """(n, p, flat H, flat Q) of a batch of Hessenberg-triangular problems (H1, Hs[, Q]), all work arrays; a problem
        without Q gets the identity.  `wrong`: the exception for a problem of the other family (None: left to the
        in-place contract)."""
        Hall, Qall = [], []
        shape = None
        for pr in problems:
            H = [pr[0]] + list(pr[1])
            shape = n, p = self._batch_shape(H, shape)
            if wrong is not None and _other_family(fam, [np.iscomplexobj(h) for h in H]):
                raise wrong
            self._as_work(H, fam.dtype)
            Hall += H
            if wantZ:
                Q = (list(pr[2]) if len(pr) > 2 and pr[2] is not None
                     else [np.asfortranarray(np.eye(n, dtype=fam.dtype)) for _ in range(p)])
                self._as_work(Q, fam.dtype)
                Qall += Q
        return n, p, Hall, Qall

    def _batch_copies(self, fam, wrong, problems, every=False):
        """The work copies behind the copying forms: Fortran-ordered copies of the factors of every problem, a list of
        matrices or a PeriodicSchur (copied with its Z and values); `wrong` for a problem of the other family."""
        def mats(A):
            return [np.array(a, dtype=fam.dtype, order="F", copy=True) for a in A]

        work = []
        for A in problems:
            dec = isinstance(A, PeriodicSchur)
            if _other_family(fam, [np.iscomplexobj(a) for a in (A.Ts if dec else A)], every):
                raise wrong
            if dec:
                cp = copy.copy(A)
                cp.Ts, cp.Z, cp.values = mats(A.Ts), mats(A.Z), np.array(A.values, copy=True)
            work.append(cp if dec else mats(A))
        return work

    def _dev_batch(self, fam, name, wrong, T, *Z, mixed=False):
        """(nb, p, n) of a device batch: one [nb, p, n, n] torch tensor, or T with Z (None: no Schur vectors) of the
        same shape.  `wrong`: the exception for tensors of the other family; `mixed`: a complex tensor next to a real
        one is the error of eigvecs instead."""
        ts = [T] + [z for z in Z if z is not None]
        if T.dim() != 4 or T.shape[2] != T.shape[3] or any(z.shape != T.shape for z in ts[1:]):
            raise DimensionMismatch("a device batch is [nb, p, n, n] tensors T and Z of square factors" if Z else
                                    "a device batch is one [nb, p, n, n] tensor of square factors")
        cplx = [t.is_complex() for t in ts]
        if _other_family(fam, cplx, every=not mixed):
            raise wrong
        if mixed and not all(cplx) and fam is _Z:
            raise TypeError("eigvecs: the factors T and the Schur vectors Z must be all real or all complex")
        if not all(t.is_cuda for t in ts):
            raise TypeError(f"device-resident {name} needs GPU tensors (use a list of PeriodicSchur for host input)" if Z
                            else f"device-resident {name} needs a GPU tensor (use lists of numpy arrays for host input)")
        return T.shape[0], T.shape[1], T.shape[2]

    def _batch_finish(self, info, infos, infos_out, raiser, strict, result):
        """The end of every batch call.  A fatal call-wide code `info` raises: always with `strict` (the Float64 pschur
        entries and every ordschur entry), otherwise only when no problem carries that code (the ComplexF64 pschur
        entries: a code that a problem carries is that problem's, the others are complete).  Then `result()` builds
        what the call returns, and the per-problem codes `infos` go to `infos_out`, or the first non-zero one raises
        through `raiser`."""
        codes = list(infos)
        if (info < 0 or info >= INFO_NOTIMPL) and (strict or info not in codes):
            self._raise(info)
        out = result()
        if infos_out is not None:
            infos_out[:] = codes
            return out
        for code in codes:
            raiser(code)
        return out

    @staticmethod
    def _batch_results(general, S, nb, p, Tall, Zall, eig, orient, si, st):
        """The decompositions of a pschur batch call from its flat factor lists: PeriodicSchur, or with `general`
        GeneralizedPeriodicSchur of signature S (None: all true)."""
        if general:
            S = [True] * p if S is None else S
            return [GeneralizedPeriodicSchur(S, Tall[q * p:(q + 1) * p], Zall[q * p:(q + 1) * p], eig[0][q], eig[1][q],
                                             eig[2][q], orient, si, st) for q in range(nb)]
        values = _eig_values(eig)  # (each problem gets a row as an array of its own, not a view of the batch's)
        return [PeriodicSchur(Tall[q * p:(q + 1) * p], Zall[q * p:(q + 1) * p], values[q].copy(), orient, si, st)
                for q in range(nb)]

    def _phessenberg_batch_(self, fam, problems):
        nb = len(problems)
        if nb == 0:
            return [], Stats()
        n, p, flat = self._batch_factors(fam, problems)
        self._as_work(flat, fam.dtype)
        tau = np.zeros((nb, p, n), dtype=fam.dtype)
        st = Stats()
        info = C.c_int(0)
        getattr(self.lib, f"psd_{fam.tag}_phessenberg_batch")(self.ctx, nb, n, p, self._ptrs(flat),
                                                              *self._evec_ptrs([tau]), C.byref(st), C.byref(info))
        self._raise(info.value)
        out = []
        for q in range(nb):
            A = flat[q * p:(q + 1) * p]
            out.append(([np.triu(a, -1 if j == 0 else 0) for j, a in enumerate(A)], tau[q]))
        return out, st

    def _pschur_batch_call(self, fam, Sarr, dev, nb, n, p, A, Z, orient, wantT, wantZ, maxitfac, infos_out, result):
        """psd_?_[g]pschur_batch[_dev] on packed factors: A and Z flat lists of work arrays, or with `dev` device
        blocks.  `result(eig, schurindex, stats)` builds what the call returns from the eigenvalue outputs."""
        ptrs = (lambda X: C.c_void_p(X.data_ptr())) if dev else self._ptrs
        eig = _eig_alloc(fam, (nb, n))
        infos, si, st, info = (C.c_int * nb)(), C.c_int(0), Stats(), C.c_int(0)
        fn = getattr(self.lib, f"psd_{fam.tag}_{'' if Sarr is None else 'g'}pschur_batch{'_dev' if dev else ''}")
        fn(self.ctx, nb, n, p, ptrs(A), *([] if Sarr is None else [Sarr]), orient.encode(), int(wantT), int(wantZ),
           int(maxitfac), ptrs(Z) if wantZ else None, *self._evec_ptrs(eig), infos, C.byref(si), C.byref(st),
           C.byref(info))
        return self._batch_finish(info.value, infos, infos_out, self._raise, fam is _D,
                                  lambda: result(eig, si.value, st))

    def _pschur_batch_(self, fam, name, problems, S, lr, wantZ, wantT, maxitfac, infos_out):
        """pschur_batch_ / zpschur_batch_ / zgpschur_batch_ / dgpschur_batch_ (`S` None: all true, the entry without a
        signature)."""
        orient = char_lr(lr)
        if hasattr(problems, "data_ptr"):
            return self._pschur_batch_dev(fam, name, problems, S, orient, wantZ, wantT, maxitfac, infos_out)
        nb = len(problems)
        if nb == 0:
            if infos_out is not None:
                infos_out[:] = []
            return []
        n, p, A = self._batch_factors(fam, problems)
        Sarr = None
        if S is None and fam is _DG:  # (the real signed entries take every signature, the all-true one included)
            S = [True] * p
        if S is not None:
            S, Sarr = self._zgbatch_sig(S, p, orient)
        self._as_work(A, fam.dtype)
        Z = [np.zeros((n, n), dtype=fam.dtype, order="F") for _ in range(nb * p)] if wantZ else []
        return self._pschur_batch_call(
            fam, Sarr, False, nb, n, p, A, Z, orient, wantT, wantZ, maxitfac, infos_out,
            lambda eig, si, st: self._batch_results(S is not None, S, nb, p, A, Z, eig, orient, si, st))

    def _pschur_batch_dev(self, fam, name, dA, S, orient, wantZ, wantT, maxitfac, infos_out):
        import torch

        wrong = fam.wrong_exc(fam.wrong_text if S is None or fam is _DG else "zgpschur_batch: ComplexF64 only")
        nb, p, n = self._dev_batch(fam, name, wrong, dA)
        Sarr = None
        if S is None and fam is _DG:
            S = [True] * p
        if S is not None:
            S, Sarr = self._zgbatch_sig(S, p, orient)
        if nb == 0:
            if infos_out is not None:
                infos_out[:] = []
            return dA.clone(), (dA.clone() if wantZ else None), np.zeros((0, n), dtype=complex), Stats()
        dT = _dev_blocks(dA, fam, "copy")
        dZ = torch.zeros_like(dT) if wantZ else None
        torch.cuda.synchronize(dA.device)
        return self._pschur_batch_call(
            fam, Sarr, True, nb, n, p, dT, dZ, orient, wantT, wantZ, maxitfac, infos_out,
            lambda eig, si, st: (dT.transpose(2, 3), (dZ.transpose(2, 3) if wantZ else None), _eig_values(eig), st))

    def _pschur_hess_batch_(self, fam, problems, S, wrong, wantT, wantZ, maxitfac, infos_out, general):
        """The *_hess_batch_ entries on a non-empty batch (`S` None: no signature argument).  `general`: whether the
        results are GeneralizedPeriodicSchur (the Float64 all-true entry returns PeriodicSchur)."""
        nb = len(problems)
        n, p, Hall, Qall = self._batch_hess(fam, problems, wantZ, wrong)
        sig = [] if S is None else [(C.c_uint8 * p)(*[1 if x else 0 for x in S])]
        eig = _eig_alloc(fam, (nb, n))
        infos, st, info = (C.c_int * nb)(), Stats(), C.c_int(0)
        fn = getattr(self.lib, f"psd_{fam.tag}_{'' if S is None else 'g'}pschur_hess_batch")
        fn(self.ctx, nb, n, p, self._ptrs(Hall), *sig, self._ptrs(Qall) if wantZ else None, int(wantT), int(wantZ),
           int(maxitfac), *self._evec_ptrs(eig), infos, C.byref(st), C.byref(info))
        return self._batch_finish(info.value, infos, infos_out, self._raise, fam is _D,
                                  lambda: self._batch_results(general, S, nb, p, Hall, Qall, eig, "R", 1, st))

    def pschur_hess_batch_(self, problems, wantT=True, wantZ=True, maxitfac=30, infos_out=None):
        """pschur!(H1, Hs; wantT, wantZ, Q, maxitfac) (src/PeriodicSchurDecompositions.jl:322-330) for a list of
        problems of equal shape in ONE call (psd_d_pschur_hess_batch: what src/krylov.jl:575-592,800-829 issues one
        by one).  `problems`: list of (H1, Hs) or (H1, Hs, Q); matrices are overwritten.  Returns a list of
        PeriodicSchur; a problem that fails to converge raises like the single call, after all have run — the other
        problems of the batch are complete then (a failure ends only the problem it occurs in).  `infos_out`: a list
        that receives the per-problem info codes instead (nothing is raised for a failed problem then; an empty batch
        leaves it as it is)."""
        if len(problems) == 0:
            return []
        return self._pschur_hess_batch_(_D, problems, None, None, wantT, wantZ, maxitfac, infos_out, False)

    def phessenberg_batch_(self, problems):
        """phessenberg!(A) (src/PeriodicSchurDecompositions.jl:213-259) for a list of problems of equal shape in ONE call
        (psd_d_phessenberg_batch).  `problems`: list of lists of p writable Fortran-ordered matrices, overwritten
        LAPACK-style.  Returns a list of (H list, tau[p][n]) like phessenberg_, and the Stats of the call."""
        return self._phessenberg_batch_(_D, problems)

    def pschur_batch_(self, problems, lr="R", wantZ=True, wantT=True, maxitfac=30, infos_out=None):
        """pschur!(A, lr; wantZ, wantT, maxitfac) (src/PeriodicSchurDecompositions.jl:120-152) for many small problems of
        equal shape in ONE call (psd_d_pschur_batch): the reduction and the Q formation run over the whole batch, the
        iteration 32 problems at a time side by side.  Float64, all-true signature.

        `problems`: a list of lists of p writable Fortran-ordered n x n matrices, overwritten with the T factors; returns
        a list of PeriodicSchur.  Or one torch [nb, p, n, n] device tensor (device-resident entry,
        psd_d_pschur_batch_dev; the input is not modified): returns (T, Z, values, stats) with T, Z torch tensors
        [nb, p, n, n] on the same device (Z None when not wantZ), values a complex [nb, n] array; orientation and
        schurindex (1 for "R", p for "L") are those of the call.

        A problem that fails to converge raises like the single call, after all have run — the others are complete
        then.  `infos_out`: a list that receives the per-problem info codes instead (nothing is raised for a failed
        problem then)."""
        return self._pschur_batch_(_D, "pschur_batch", problems, None, lr, wantZ, wantT, maxitfac, infos_out)

    def pschur_batch(self, problems, lr="R", **kw):
        """Copying form of pschur_batch_: the factors are left untouched."""
        if not hasattr(problems, "data_ptr"):
            problems = self._batch_copies(_D, _D.wrong_exc(_D.wrong_text), problems)
        return self.pschur_batch_(problems, lr, **kw)

    def zphessenberg_batch_(self, problems):
        """phessenberg!(A) for a list of ComplexF64 problems of equal shape in ONE call (psd_z_phessenberg_batch): one
        workgroup reduces one problem.  `problems`: list of lists of p writable Fortran-ordered complex128 matrices,
        overwritten LAPACK-style.  Returns a list of (H list, tau[p][n]) like phessenberg_, and the Stats of the call."""
        return self._phessenberg_batch_(_Z, problems)

    def zpschur_batch_(self, problems, lr="R", wantZ=True, wantT=True, maxitfac=30, infos_out=None, S=None):
        """pschur!(A::Vector{Matrix{ComplexF64}}, lr; wantZ, wantT, maxitfac) for many small problems of equal shape in
        ONE call (psd_z_pschur_batch): the reduction and the Q formation one workgroup per problem (and factor), the
        iteration one wavefront per problem in a single launch.  All signatures +1; with `S` (one signature for the
        batch) the call is zgpschur_batch_(problems, S, lr, ...).

        `problems`: a list of lists of p writable Fortran-ordered complex128 n x n matrices, overwritten with the T
        factors; returns a list of PeriodicSchur.  Or one torch complex128 [nb, p, n, n] device tensor (device-resident
        entry, psd_z_pschur_batch_dev; the input is not modified): returns (T, Z, values, stats) as pschur_batch_ does.

        A problem that fails to converge raises like the single call, after all have run — the others are complete
        then.  `infos_out`: a list that receives the per-problem info codes instead (nothing is raised for a failed
        problem then)."""
        name = "zpschur_batch" if S is None else "zgpschur_batch"
        return self._pschur_batch_(_Z, name, problems, S, lr, wantZ, wantT, maxitfac, infos_out)

    def zpschur_batch(self, problems, lr="R", **kw):
        """Copying form of zpschur_batch_: the factors are left untouched."""
        if not hasattr(problems, "data_ptr"):
            problems = self._batch_copies(_Z, _Z.wrong_exc(_Z.wrong_text), problems)
        return self.zpschur_batch_(problems, lr, **kw)

    def zpschur_hess_batch_(self, problems, wantT=True, wantZ=True, maxitfac=30, infos_out=None):
        """pschur!(H1, Hs, S; wantT, wantZ, Q, maxitfac) for ComplexF64 with S all true (src/generalized.jl:166-175) for a
        list of Hessenberg-triangular problems of equal shape in ONE call (psd_z_pschur_hess_batch).  `problems`: list
        of (H1, Hs) or (H1, Hs, Q); matrices are overwritten.  Returns a list of GeneralizedPeriodicSchur, as zpschur_hess_
        does; failures and `infos_out` as zpschur_batch_."""
        if len(problems) == 0:
            if infos_out is not None:
                infos_out[:] = []
            return []
        wrong = TypeError("zpschur_hess_batch_: ComplexF64 only (use pschur_hess_batch_ for Float64 problems)")
        return self._pschur_hess_batch_(_Z, problems, None, wrong, wantT, wantZ, maxitfac, infos_out, True)

    # ---- ComplexF64 batch family with a signed signature (psd_z_gp*_batch): gpschur(As, Bs) for many small problems
    def _zgbatch_sig(self, S, p, orient):
        """The signature of a batch as a C array; the checks of pschur!(A, S, lr) (src/generalized.jl:138-141)."""
        S = [bool(x) for x in S]
        if len(S) != p:
            raise DimensionMismatch("length of S must match the period")
        if not (S[p - 1] if orient == "L" else S[0]):
            raise ValueError("The leftmost entry in S must be true")  # src/generalized.jl:140
        return S, (C.c_uint8 * p)(*[1 if x else 0 for x in S])

    def zgphessenberg_batch_(self, problems, S, wantQ=True):
        """_phessenberg!(A, S; wantQ) for ComplexF64 (src/generalized.jl:988-1082) for a list of problems of equal shape
        and ONE signature in ONE call (psd_z_gphessenberg_batch): stage 1 one workgroup per problem, stage 2 one
        wavefront per problem.  `problems`: list of lists of p writable Fortran-ordered complex128 matrices, overwritten
        with the Hessenberg / triangular factors.  Returns a list of (H list, Q list) like gphessenberg_, and the Stats
        of the call."""
        nb = len(problems)
        if nb == 0:
            return [], Stats()
        n, p, flat = self._batch_factors(_Z, problems)
        self._as_work(flat, np.complex128)
        S, Sarr = self._zgbatch_sig(S, p, "R")
        Qall = [np.zeros((n, n), dtype=np.complex128, order="F") for _ in range(nb * p)] if wantQ else []
        st = Stats()
        info = C.c_int(0)
        self.lib.psd_z_gphessenberg_batch(self.ctx, nb, n, p, self._ptrs(flat), Sarr, self._ptrs(Qall) if wantQ else None,
                                          C.byref(st), C.byref(info))
        self._raise(info.value)
        return [(flat[q * p:(q + 1) * p], Qall[q * p:(q + 1) * p] if wantQ else []) for q in range(nb)], st

    def zgpschur_batch_(self, problems, S, lr="R", wantZ=True, wantT=True, maxitfac=30, infos_out=None):
        """pschur!(A::Vector{Matrix{ComplexF64}}, S, lr; wantZ, wantT, maxitfac) (src/generalized.jl:108-148) for many
        small problems of equal shape and ONE signature `S` in ONE call (psd_z_gpschur_batch): the signed Hessenberg
        reduction and the signed periodic QZ iteration, one workgroup / one wavefront per problem.

        `problems`: a list of lists of p writable Fortran-ordered complex128 n x n matrices, overwritten with the T
        factors; returns a list of GeneralizedPeriodicSchur.  Or one torch complex128 [nb, p, n, n] device tensor
        (device-resident entry, psd_z_gpschur_batch_dev; the input is not modified): returns (T, Z, values, stats).
        An all-true `S` runs the path of zpschur_batch_ (the same bits).  Failures and `infos_out` as zpschur_batch_."""
        return self._pschur_batch_(_Z, "zgpschur_batch", problems, S, lr, wantZ, wantT, maxitfac, infos_out)

    def zgpschur_batch(self, problems, S, lr="R", **kw):
        """Copying form of zgpschur_batch_: the factors are left untouched."""
        if not hasattr(problems, "data_ptr"):
            problems = self._batch_copies(_Z, TypeError("zgpschur_batch: ComplexF64 only"), problems)
        return self.zgpschur_batch_(problems, S, lr, **kw)

    def zgpschur_hess_batch_(self, problems, S, wantT=True, wantZ=True, maxitfac=30, infos_out=None):
        """pschur!(H1, Hs, S; wantT, wantZ, Q, maxitfac) for ComplexF64 (src/generalized.jl:166-175) for a list of
        Hessenberg-triangular problems of equal shape and ONE signature in ONE call (psd_z_gpschur_hess_batch).
        `problems`: list of (H1, Hs) or (H1, Hs, Q); matrices are overwritten.  Returns a list of
        GeneralizedPeriodicSchur, as zpschur_hess_ does; failures and `infos_out` as zpschur_batch_."""
        if len(problems) == 0:
            if infos_out is not None:
                infos_out[:] = []
            return []
        S = [bool(x) for x in S]
        if len(S) != len(problems[0][1]) + 1:
            raise DimensionMismatch("S must have one entry per factor")
        if not S[0]:
            raise ValueError("Signature entry S[1] must be true")  # src/generalized.jl:182
        wrong = TypeError("zgpschur_hess_batch_: ComplexF64 only")
        return self._pschur_hess_batch_(_Z, problems, S, wrong, wantT, wantZ, maxitfac, infos_out, True)

    # ---- Float64 batch family with a signature (psd_d_gp*_batch): pencils and generalized periodic products with real
    # data; real quasi-triangular T_1, orthogonal Z, conjugate pairs as exact conjugates
    def dgphessenberg_batch_(self, problems, S, wantQ=True):
        """_phessenberg!(A, S; wantQ) for Float64 (src/generalized.jl:988-1082) for a list of problems of equal shape and
        ONE signature in ONE call (psd_d_gphessenberg_batch): stage 1 one workgroup per problem, stage 2 one wavefront
        per problem.  `problems`: list of lists of p writable Fortran-ordered float64 matrices, overwritten with the
        Hessenberg / triangular factors.  `S` None: all true.  Returns a list of (H list, Q list) like gphessenberg_,
        and the Stats of the call."""
        nb = len(problems)
        if nb == 0:
            return [], Stats()
        n, p, flat = self._batch_factors(_DG, problems)
        self._as_work(flat, np.float64)
        S, Sarr = self._zgbatch_sig([True] * p if S is None else S, p, "R")
        Qall = [np.zeros((n, n), order="F") for _ in range(nb * p)] if wantQ else []
        st = Stats()
        info = C.c_int(0)
        self.lib.psd_d_gphessenberg_batch(self.ctx, nb, n, p, self._ptrs(flat), Sarr, self._ptrs(Qall) if wantQ else None,
                                          C.byref(st), C.byref(info))
        self._raise(info.value)
        return [(flat[q * p:(q + 1) * p], Qall[q * p:(q + 1) * p] if wantQ else []) for q in range(nb)], st

    def dgpschur_batch_(self, problems, S, lr="R", wantZ=True, wantT=True, maxitfac=120, infos_out=None):
        """pschur!(A::Vector{Matrix{Float64}}, S, lr; wantZ, wantT, maxitfac) (src/rgeneralized.jl:3-45) for many small
        problems of equal shape and ONE signature `S` in ONE call (psd_d_gpschur_batch): the signed Hessenberg
        reduction and the real signed periodic QZ iteration (after MB03BD), one workgroup / one wavefront per problem.
        The default `maxitfac` is that of pschur_(..., S=...) for Float64.

        `problems`: a list of lists of p writable Fortran-ordered float64 n x n matrices, overwritten with the T
        factors; returns a list of GeneralizedPeriodicSchur with real Ts (the one at schurindex quasi-triangular) and
        real orthogonal Z; the `values` of a 2 x 2 block are exact conjugates.  Or one torch float64 [nb, p, n, n]
        device tensor (device-resident entry, psd_d_gpschur_batch_dev; the input is not modified): returns
        (T, Z, values, stats).  `S` None or all true: the same signed kernels (as pschur_(..., S=...) — not the path of
        pschur_batch_, whose results have another form).  A problem that fails to converge raises like the single
        call, after all have run — the others are complete then.  `infos_out`: a list that receives the per-problem
        info codes instead."""
        return self._pschur_batch_(_DG, "dgpschur_batch", problems, S, lr, wantZ, wantT, maxitfac, infos_out)

    def dgpschur_batch(self, problems, S, lr="R", **kw):
        """Copying form of dgpschur_batch_: the factors are left untouched."""
        if not hasattr(problems, "data_ptr"):
            problems = self._batch_copies(_DG, _DG.wrong_exc(_DG.wrong_text), problems)
        return self.dgpschur_batch_(problems, S, lr, **kw)

    def dgpschur_hess_batch_(self, problems, S, wantT=True, wantZ=True, maxitfac=120, infos_out=None):
        """pschur!(H1, Hs, S; wantT, wantZ, Q, maxitfac) for Float64 (src/rgeneralized.jl:49-80) for a list of
        Hessenberg-triangular problems of equal shape and ONE signature in ONE call (psd_d_gpschur_hess_batch).
        `problems`: list of (H1, Hs) or (H1, Hs, Q); matrices are overwritten.  `S` None: all true.  Returns a list of
        GeneralizedPeriodicSchur, as gpschur_hess_ does; failures and `infos_out` as dgpschur_batch_."""
        if len(problems) == 0:
            if infos_out is not None:
                infos_out[:] = []
            return []
        p = len(problems[0][1]) + 1
        S = [True] * p if S is None else [bool(x) for x in S]
        if len(S) != p:
            raise DimensionMismatch("S must have one entry per factor")
        if not S[0]:
            raise ValueError("Signature entry S[1] must be true")  # src/rgeneralized.jl:73
        wrong = TypeError("dgpschur_hess_batch_: Float64 only (ComplexF64 problems: zgpschur_hess_batch_)")
        return self._pschur_hess_batch_(_DG, problems, S, wrong, wantT, wantZ, maxitfac, infos_out, True)

    def gpschur_batch(self, As_list, Bs_list, real=False, **kw):
        """gpschur(As, Bs) (src/generalized.jl:1191-1211) for many pairs of series of equal shape in ONE call: the
        interleaving of `gpschur` per problem, then zgpschur_batch_ with the common signature (T, F, T, F, ...).
        Returns a list of GeneralizedPeriodicSchur.  `real`: all matrices must be real, and the interleaving goes to
        dgpschur_batch_ as it is (real quasi-triangular T, orthogonal Z, exact conjugate pairs) instead of being cast to
        ComplexF64; a complex matrix raises TypeError then."""
        if len(As_list) != len(Bs_list):
            raise DimensionMismatch("one Bs per As")
        if real and any(np.iscomplexobj(m) for Ms in list(As_list) + list(Bs_list) for m in Ms):
            raise TypeError("gpschur_batch(real=True): the matrices must be real (real=False takes complex ones)")
        cz = lambda m: np.array(m, dtype=np.float64 if real else np.complex128, order="F", copy=True)  # noqa: E731
        problems = []
        for As, Bs in zip(As_list, Bs_list):
            ph = len(As)
            if len(Bs) != ph:
                raise DimensionMismatch("As and Bs must have the same length")
            ib = 0 if ph == 1 else ph - 2
            Cs = [cz(As[ph - 1]), cz(Bs[ib])]
            for j in range(ph - 1, 0, -1):  # j = ph-1 .. 1 (1-based), as gpschur
                Cs.append(cz(As[j - 1]))
                jx = ph if j == 1 else j - 1
                Cs.append(cz(Bs[jx - 1]))
            problems.append(Cs)
        if not problems:
            return []
        # (pairs of another length make a problem of another period: turned away with those of another order)
        run = self.dgpschur_batch_ if real else self.zgpschur_batch_
        return run(problems, [True, False] * len(As_list[0]), "R", **kw)


    def ordschur_(self, P, select, wantZ=True, Z=None):
        """LinearAlgebra.ordschur!(P, select; wantZ, Z) — src/ordschur.jl:11-73 (ComplexF64).  Mutates and returns P.
        `Z`: supplementary matrices that receive the transformations instead of P.Z (src/ordschur.jl:17,34-42; not for
        the right orientation, :36-38)."""
        if Z is not None and wantZ:
            if P.orientation == "R":
                raise NotImplementedPSD("no logic for reversing supplementary Z")  # src/ordschur.jl:37
            if len(Z) != len(P.Ts):
                raise DimensionMismatch("one supplementary Z per factor")
            keep = P.Z
            P.Z = list(Z)
            try:
                return self.ordschur_(P, select, wantZ=True)
            finally:
                P.Z = keep
        n = P.Ts[0].shape[0]
        p = len(P.Ts)
        if len(select) != n:
            raise DimensionMismatch("select must have one entry per eigenvalue")
        if isinstance(P, GeneralizedPeriodicSchur) and not all(P.S):
            return self._gordschur_(P, select, wantZ)
        if not np.iscomplexobj(P.Ts[0]):
            return self._rordschur_(P, select, wantZ)
        if P.schurindex not in (1, p):
            raise ValueError("only implemented for schurindex in (1,p)")  # src/ordschur.jl:32
        self._as_work(P.Ts, np.complex128)
        wantZ = wantZ and len(P.Z) > 0
        if wantZ:
            self._as_work(P.Z, np.complex128)
        sel = (C.c_uint8 * n)(*[1 if x else 0 for x in select])
        alpha = np.zeros(n, dtype=np.complex128)
        beta = np.zeros(n)
        sc = np.zeros(n, dtype=np.int32)
        st = Stats()
        info = C.c_int(0)
        dp = C.POINTER(C.c_double)
        self.lib.psd_z_ordschur(self.ctx, n, p, self._ptrs(P.Ts), self._ptrs(P.Z) if wantZ else None,
                                P.orientation.encode(), P.schurindex, sel, int(wantZ),
                                alpha.view(np.float64).ctypes.data_as(dp), beta.ctypes.data_as(dp),
                                sc.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st), C.byref(info))
        iv = info.value
        if iv == 3000:
            raise SingularException()
        if 2000 <= iv < 3000:
            raise IllConditionedException(iv - 2000)
        self._raise(iv)
        P.values = _scaled_values(alpha, beta, sc)
        if isinstance(P, GeneralizedPeriodicSchur):
            P.alpha, P.beta, P.alphascale = alpha, beta, sc
        P.stats = st
        return P

    def _gordschur_(self, P, select, wantZ):
        """ordschur!(P::GeneralizedPeriodicSchur, select; wantZ) with a signed S — src/ordschur.jl:11-96,323-328,
        src/sylswap.jl:638-764 (1x1 swaps; a Float64 decomposition needs a real spectrum in this build)."""
        n = P.Ts[0].shape[0]
        p = len(P.Ts)
        if P.schurindex not in (1, p):
            raise ValueError("only implemented for schurindex in (1,p)")  # src/ordschur.jl:32
        cplx = np.iscomplexobj(P.Ts[0])
        dt = np.complex128 if cplx else np.float64
        self._as_work(P.Ts, dt)
        wantZ = wantZ and len(P.Z) > 0
        if wantZ:
            self._as_work(P.Z, dt)
        sel = (C.c_uint8 * n)(*[1 if x else 0 for x in select])
        Sarr = (C.c_uint8 * p)(*[1 if x else 0 for x in P.S])
        alpha = np.zeros(n, dtype=np.complex128)
        beta = np.zeros(n)
        sc = np.zeros(n, dtype=np.int32)
        st = Stats()
        info = C.c_int(0)
        dp = C.POINTER(C.c_double)
        fn = self.lib.psd_z_gordschur if cplx else self.lib.psd_d_gordschur
        fn(self.ctx, n, p, self._ptrs(P.Ts), self._ptrs(P.Z) if wantZ else None, Sarr, P.orientation.encode(),
           P.schurindex, sel, int(wantZ), alpha.view(np.float64).ctypes.data_as(dp), beta.ctypes.data_as(dp),
           sc.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st), C.byref(info))
        iv = info.value
        if iv == 3000:
            raise SingularException()
        if 2000 <= iv < 3000:
            raise IllConditionedException(iv - 2000)
        self._raise(iv)
        P.values = _scaled_values(alpha, beta, sc)
        P.alpha, P.beta, P.alphascale = alpha, beta, sc
        P.stats = st
        return P

    def _rordschur_(self, P, select, wantZ):
        """LinearAlgebra.ordschur!(P, select; wantZ) for Float64 — src/rordschur.jl:3-132."""
        n = P.Ts[0].shape[0]
        p = len(P.Ts)
        if P.schurindex not in (1, p):
            raise ValueError("only implemented for schurindex in (1,p)")  # src/rordschur.jl:25
        self._as_work(P.Ts)
        wantZ = wantZ and len(P.Z) > 0
        if wantZ:
            self._as_work(P.Z)
        sel = (C.c_uint8 * n)(*[1 if x else 0 for x in select])
        wr = np.zeros(n)
        wi = np.zeros(n)
        st = Stats()
        info = C.c_int(0)
        dp = C.POINTER(C.c_double)
        self.lib.psd_d_ordschur(self.ctx, n, p, self._ptrs(P.Ts), self._ptrs(P.Z) if wantZ else None,
                                P.orientation.encode(), P.schurindex, sel, int(wantZ), wr.ctypes.data_as(dp),
                                wi.ctypes.data_as(dp), C.byref(st), C.byref(info))
        iv = info.value
        if iv == 3000:
            raise SingularException()
        if 2000 <= iv < 3000:
            raise IllConditionedException(iv - 2000)
        self._raise(iv)
        P.values = wr + 1j * wi
        P.stats = st
        return P

    @staticmethod
    def _raise_ord(iv):
        """The per-problem codes of ordschur!: 3000 singular, 2000 + row ill-conditioned."""
        if iv == 3000:
            raise SingularException()
        if 2000 <= iv < 3000:
            raise IllConditionedException(iv - 2000)
        Engine._raise(iv)

    def _ord_batch_select(self, select, nb, n):
        try:
            return self._batch_select(select, nb, n)
        except ValueError:
            raise DimensionMismatch("select must be [nb][n] flags or one row of n: one entry per eigenvalue") from None

    def _batch_decomps(self, fam, name, wrong, problems, needZ, work, signed=False):
        """(n, p, orientation, schurindex, flat Ts) of a batch of PeriodicSchur, which must agree in all four and be of
        the family.  `needZ`: the Schur vectors are required, of the family like the factors, and returned as a flat
        list too (eigvecs); otherwise they may be missing and are the caller's business (ordschur).  `work`: the factors
        are returned as they are, for the in-place contract (ordschur mutates); otherwise as read-only Fortran copies
        (eigvecs never writes the problems).  `signed`: the entry takes signed GeneralizedPeriodicSchur, which must
        agree in S too; the common signature (all true for a plain PeriodicSchur) is returned last.

        Which kinds of factors T and vectors Z each entry turns away (`wrong`: the entry's own exception; "mixed": the
        TypeError of the single eigvecs call; otherwise the problem goes on, to the in-place contract for ordschur):
                            T real, Z real   T real, Z complex   T complex, Z real   T complex, Z complex
            ordschur  d     -                wrong               wrong               wrong
            ordschur  z     wrong            wrong               -                   -
            eigvecs   d     -                mixed               wrong               wrong
            eigvecs   z     wrong            mixed               mixed               -
        (a list of factors or of vectors that is only partly complex: `any` for d, `all` for z, as the code says)."""
        n = S = None
        Ts, Zs = [], []
        for ps in problems:
            if not signed and isinstance(ps, GeneralizedPeriodicSchur) and not all(ps.S):
                raise NotImplementedPSD(f"{name}: signed GeneralizedPeriodicSchur "
                                        f"(use {'geigvecs' if needZ else 'ordschur_'} per problem)")
            if needZ and (len(ps.Z) == 0 or ps.Z[0].shape[0] == 0):
                raise ValueError("eigvecs requires Schur vectors in the PSD")  # vectors.jl:30-32
            cT, cZ = [np.iscomplexobj(t) for t in ps.Ts], [np.iscomplexobj(z) for z in ps.Z]
            if needZ:  # eigvecs: factors and vectors of different kinds are the error of the single call
                other = any(cT) if fam.dtype is np.float64 else not any(cT + cZ)
                mixed = any(cZ) if fam.dtype is np.float64 else not all(cT + cZ)
            else:  # ordschur: real vectors beside complex factors are left to the in-place contract
                other = any(cT + cZ) if fam.dtype is np.float64 else not all(cT)
                mixed = False
            if other:
                raise wrong
            if mixed:
                raise TypeError("eigvecs: the factors T and the Schur vectors Z must be all real or all complex")
            nq = ps.Ts[0].shape[0] if needZ else _check_square(ps.Ts)
            if n is None:
                n, p, orient, si = nq, len(ps.Ts), ps.orientation, ps.schurindex
            if (nq != n or len(ps.Ts) != p or (needZ and len(ps.Z) != p) or ps.orientation != orient
                    or ps.schurindex != si or any(a.shape != (n, n) for a in list(ps.Ts) + list(ps.Z))):
                raise DimensionMismatch("the problems of a batch must have equal order, period, orientation and schurindex")
            if signed:
                Sq = [bool(x) for x in getattr(ps, "S", [True] * p)]
                S = Sq if S is None else S
                if Sq != S:
                    raise DimensionMismatch("the problems of a batch must have equal signatures S")
            Ts += ps.Ts if work else [np.asfortranarray(t, dtype=fam.dtype) for t in ps.Ts]
            if needZ:
                Zs += ps.Z if work else [np.asfortranarray(z, dtype=fam.dtype) for z in ps.Z]
        return (n, p, orient, si, Ts) + ((Zs,) if needZ else ()) + ((S,) if signed else ())

    def _ordschur_batch_call(self, fam, name, dev, nb, n, p, T, Z, orient, si, sel, wantZ, infos_out, result, S=None):
        """psd_?_[g]ordschur_batch[_dev] on packed factors: T and Z flat lists of work arrays, or with `dev` device
        blocks (the values row of a problem that failed is NaN then); `S`: the signature of the signed entry (None: the
        entry without one).  Leaves the call's stats and swap counts in self.<name>_stats / _nswaps;
        `result(eig, codes, nswaps, stats)` builds what the call returns."""
        if S is not None and not S[si - 1]:
            raise ValueError("The entry of S at schurindex must be true")  # src/generalized.jl:182
        ptrs = (lambda X: C.c_void_p(X.data_ptr())) if dev else self._ptrs
        eig = _eig_alloc(fam, (nb, n), nan=dev)
        infos, nsw, st, info = (C.c_int * nb)(), (C.c_int * nb)(), Stats(), C.c_int(0)
        fn = getattr(self.lib, f"psd_{fam.tag}_{'' if S is None else 'g'}ordschur_batch{'_dev' if dev else ''}")
        sig = [] if S is None else [(C.c_uint8 * p)(*[1 if x else 0 for x in S])]
        fn(self.ctx, nb, n, p, ptrs(T), ptrs(Z) if wantZ else None, *sig, orient.encode(), int(si),
           sel.ctypes.data_as(C.POINTER(C.c_uint8)), int(wantZ), *self._evec_ptrs(eig), infos, nsw, C.byref(st),
           C.byref(info))

        def done():
            self._ordschur_batch_attrs(name, st, np.array(list(nsw), dtype=np.int32))
            return result(eig, infos, nsw, st)

        return self._batch_finish(info.value, infos, infos_out, self._raise_ord, True, done)

    def _ordschur_batch_attrs(self, name, st, nswaps):
        setattr(self, name + "_stats", st)
        setattr(self, name + "_nswaps", nswaps)

    def _ordschur_batch_(self, fam, name, problems, args, wantZ, infos_out, lr, schurindex, signed=False, S=None):
        """ordschur_batch_ / zordschur_batch_ / zgordschur_batch_ / dgordschur_batch_ (`signed`: the entry with a
        signature, which the problems carry; `S`: that of device tensors)."""
        wrong = NotImplementedPSD((_GORD_WRONG if signed else _ORD_WRONG)[fam])
        if hasattr(problems, "data_ptr"):
            if len(args) != 2:
                raise TypeError(f"{name}_(T, Z, select, lr=..., schurindex=...)")
            return self._ordschur_batch_dev(fam, name, wrong, problems, args[0], args[1], lr, schurindex, wantZ, infos_out,
                                            signed, S)
        if len(args) != 1:
            raise TypeError(f"{name}_(problems, select, wantZ=True)")
        problems = list(problems)
        nb = len(problems)
        if nb == 0:
            if infos_out is not None:
                infos_out[:] = []
            self._ordschur_batch_attrs(name, Stats(), np.zeros(0, dtype=np.int32))
            return []
        n, p, orient, si, Ts, *S = self._batch_decomps(fam, name, wrong, problems, needZ=False, work=True, signed=signed)
        S = S[0] if S else None  # (the entries without a signature pass none on)
        if si not in (1, p):
            raise ValueError("only implemented for schurindex in (1,p)")  # src/ordschur.jl:32, src/rordschur.jl:25
        wantZ = bool(wantZ) and all(len(ps.Z) > 0 for ps in problems)
        Zs = []
        if wantZ:
            for ps in problems:
                if len(ps.Z) != p:
                    raise DimensionMismatch("one Z per factor")
                Zs += ps.Z
        sel = self._ord_batch_select(args[0], nb, n)
        self._as_work(Ts, fam.dtype)
        self._as_work(Zs, fam.dtype)

        def result(eig, infos, nsw, st):
            values = _eig_values(eig)
            for q, ps in enumerate(problems):
                if infos[q] == 0:  # (a problem that failed keeps its old values)
                    ps.values = values[q].copy()  # (its own array, not a view that keeps the batch's alive)
                    if fam is not _D and isinstance(ps, GeneralizedPeriodicSchur):  # (the real unsigned entry has no scaled form)
                        ps.alpha, ps.beta, ps.alphascale = eig[0][q].copy(), eig[1][q].copy(), eig[2][q].copy()
                ps.stats = Stats.from_buffer_copy(st)
                ps.stats.nsweeps = nsw[q]
            return problems

        return self._ordschur_batch_call(fam, name, False, nb, n, p, Ts, Zs, char_lr(orient), si, sel, wantZ, infos_out,
                                         result, S)

    def _ordschur_batch_dev(self, fam, name, wrong, T, Z, select, lr, schurindex, wantZ, infos_out, signed=False, S=None):
        import torch

        nb, p, n = self._dev_batch(fam, name, wrong, T, Z)
        if signed:
            S = [True] * p if S is None else [bool(x) for x in S]
            if len(S) != p:
                raise DimensionMismatch("length of S must match the period")
        wantZ = bool(wantZ) and Z is not None
        orient = char_lr(lr)
        if schurindex not in (1, p):
            raise ValueError("only implemented for schurindex in (1,p)")  # src/ordschur.jl:32, src/rordschur.jl:25
        if nb == 0:
            if infos_out is not None:
                infos_out[:] = []
            self._ordschur_batch_attrs(name, Stats(), np.zeros(0, dtype=np.int32))
            return T, Z, np.zeros((0, n), dtype=complex), getattr(self, name + "_stats")
        sel = self._ord_batch_select(select, nb, n)
        dT = _dev_blocks(T, fam, "inplace_if_blocks")
        dZ = _dev_blocks(Z, fam, "inplace_if_blocks") if wantZ else None
        torch.cuda.synchronize(T.device)
        return self._ordschur_batch_call(
            fam, name, True, nb, n, p, dT, dZ, orient, schurindex, sel, wantZ, infos_out,
            lambda eig, infos, nsw, st: (dT.transpose(2, 3), (dZ.transpose(2, 3) if wantZ else Z), _eig_values(eig), st), S)

    def _ordschur_batch(self, fam, inplace, problems, args, kw, wrong=None):
        """The copying forms of the four entries."""
        if hasattr(problems, "data_ptr"):
            Z = args[0] if len(args) > 0 else None
            return inplace(problems.clone(), Z.clone() if Z is not None else None, *args[1:], **kw)
        wrong = NotImplementedPSD(wrong or _ORD_WRONG[fam])
        return inplace(self._batch_copies(fam, wrong, problems, every=True), *args, **kw)

    def ordschur_batch_(self, problems, *args, wantZ=True, infos_out=None, lr="R", schurindex=1):
        """LinearAlgebra.ordschur!(P, select; wantZ) (src/rordschur.jl:3-132) for MANY small decompositions of one shape
        in ONE call (psd_d_ordschur_batch): the follow-up of pschur_batch.  Float64, all-true signature.  Per problem
        the result contract is that of `ordschur_`; a problem's result does not depend on its place in the batch.

        ordschur_batch_(problems, select, wantZ=True, infos_out=None): `problems` a list of PeriodicSchur of equal order,
        period, orientation and schurindex (1 or p) with writable Fortran-ordered factors; each is mutated (Ts, Z, values,
        stats) and the list returned.  The `stats` of a problem are the call's, with `nsweeps` its own swap count; the
        call's own are left in `self.ordschur_batch_stats` (nsweeps: all swaps, nlaunch_step: launches of the swap
        kernel, one per group), the swap counts in `self.ordschur_batch_nswaps` ([nb]).
        ordschur_batch_(T, Z, select, lr=..., schurindex=..., wantZ=True, infos_out=None): the torch outputs of the
        device-resident pschur_batch_ ([nb, p, n, n] tensors; Z may be None with wantZ=False); returns (T, Z, values,
        stats).  Tensors in the layout pschur_batch_ returns — a transposed view of contiguous column-major blocks,
        float64 — are reordered IN PLACE without a copy, and the returned tensors share their storage; any other layout
        is copied first and the inputs stay as they were.  With wantZ=False the Z that was passed (a tensor or None) is
        returned as it is.  The `values` row of a failed problem is NaN.

        `select`: [nb][n] flags, or one [n] row used for every problem; selecting one member of a conjugate pair takes
        its partner along, per problem.  A problem whose swap is rejected (equal eigenvalues: SingularException, an
        ill-conditioned swap: IllConditionedException) ends alone, a consistent decomposition with its old `values`;
        the exception of the first such problem is raised after all have run — the others are complete then.
        `infos_out`: a list that receives the per-problem codes instead (nothing is raised for a failed problem)."""
        return self._ordschur_batch_(_D, "ordschur_batch", problems, args, wantZ, infos_out, lr, schurindex)

    def ordschur_batch(self, problems, *args, **kw):
        """Copying form of ordschur_batch_: the decompositions are left untouched (device tensors are copied too)."""
        return self._ordschur_batch(_D, self.ordschur_batch_, problems, args, kw)

    def zordschur_batch_(self, problems, *args, wantZ=True, infos_out=None, lr="R", schurindex=1):
        """LinearAlgebra.ordschur!(P, select; wantZ) (src/ordschur.jl:11-73) for MANY small ComplexF64 decompositions of
        one shape in ONE call (psd_z_ordschur_batch): the follow-up of zpschur_batch, the complex counterpart of
        ordschur_batch_.  All-true signature.  Per problem the result contract is that of `ordschur_`; a problem's
        result does not depend on its place in the batch.

        zordschur_batch_(problems, select, wantZ=True, infos_out=None): `problems` a list of complex PeriodicSchur (or
        GeneralizedPeriodicSchur with S all true) of equal order, period, orientation and schurindex (1 or p) with
        writable Fortran-ordered complex128 factors; each is mutated (Ts, Z, values, stats) and the list returned.  The
        `stats` of a problem are the call's, with `nsweeps` its own swap count; the call's own are left in
        `self.zordschur_batch_stats` (nsweeps: all swaps, nlaunch_step: launches of the swap kernel, one per group),
        the swap counts in `self.zordschur_batch_nswaps` ([nb]).
        zordschur_batch_(T, Z, select, lr=..., schurindex=..., wantZ=True, infos_out=None): the torch outputs of the
        device-resident zpschur_batch_ ([nb, p, n, n] complex128 tensors; Z may be None with wantZ=False); returns
        (T, Z, values, stats).  Tensors in the layout zpschur_batch_ returns — a transposed view of contiguous
        column-major blocks — are reordered IN PLACE without a copy, and the returned tensors share their storage; any
        other layout is copied first and the inputs stay as they were.  The `values` row of a failed problem is NaN.

        `select`: [nb][n] flags, or one [n] row used for every problem, used as given.  A problem whose swap is
        rejected (equal eigenvalues: SingularException, an ill-conditioned swap: IllConditionedException) ends alone, a
        consistent decomposition with its old `values`; the exception of the first such problem is raised after all
        have run — the others are complete then.  `infos_out`: a list that receives the per-problem codes instead
        (nothing is raised for a failed problem)."""
        return self._ordschur_batch_(_Z, "zordschur_batch", problems, args, wantZ, infos_out, lr, schurindex)

    def zordschur_batch(self, problems, *args, **kw):
        """Copying form of zordschur_batch_: the decompositions are left untouched (device tensors are copied too)."""
        return self._ordschur_batch(_Z, self.zordschur_batch_, problems, args, kw)

    def zgordschur_batch_(self, problems, *args, wantZ=True, infos_out=None, lr="R", schurindex=1, S=None):
        """LinearAlgebra.ordschur!(P::GeneralizedPeriodicSchur, select; wantZ) (src/ordschur.jl:11-96, the signed swaps of
        src/sylswap.jl:638-764) for MANY small ComplexF64 decompositions of one shape and ONE signature in ONE call
        (psd_z_gordschur_batch): the follow-up of zgpschur_batch / gpschur_batch, the signed counterpart of
        zordschur_batch_.  Per problem the result contract is that of `ordschur_`; a problem's result does not depend on
        its place in the batch.  An all-true signature runs the path of zordschur_batch_ (the same bits).

        zgordschur_batch_(problems, select, wantZ=True, infos_out=None): `problems` a list of complex
        GeneralizedPeriodicSchur of equal order, period, orientation, schurindex (1 or p) and S, with writable
        Fortran-ordered complex128 factors; each is mutated (Ts, Z, values, alpha, beta, alphascale, stats) and the list
        returned.  The `stats` of a problem are the call's, with `nsweeps` its own swap count; the call's own are left
        in `self.zgordschur_batch_stats`, the swap counts in `self.zgordschur_batch_nswaps` ([nb]).
        zgordschur_batch_(T, Z, select, S=..., lr=..., schurindex=..., wantZ=True, infos_out=None): the torch outputs
        of the device-resident zgpschur_batch_ ([nb, p, n, n] complex128 tensors; Z may be None with wantZ=False) and
        the signature of that call; returns (T, Z, values, stats), in place or through a copy as zordschur_batch_ does.

        `select`, rejected swaps and `infos_out` as zordschur_batch_."""
        return self._ordschur_batch_(_Z, "zgordschur_batch", problems, args, wantZ, infos_out, lr, schurindex, True, S)

    def zgordschur_batch(self, problems, *args, **kw):
        """Copying form of zgordschur_batch_: the decompositions are left untouched (device tensors are copied too)."""
        return self._ordschur_batch(_Z, self.zgordschur_batch_, problems, args, kw, _GORD_WRONG[_Z])

    def dgordschur_batch_(self, problems, *args, wantZ=True, infos_out=None, lr="R", schurindex=1, S=None):
        """LinearAlgebra.ordschur!(P::GeneralizedPeriodicSchur{Float64}, select; wantZ) (src/rordschur.jl:3-132 with the
        signed block swaps of src/sylswap.jl:197-538) for MANY small real decompositions of one shape and ONE signature in
        ONE call (psd_d_gordschur_batch): the follow-up of dgpschur_batch / gpschur_batch(..., real=True), the signed
        counterpart of ordschur_batch_.  T stays real and quasi-triangular, Z orthogonal, conjugate pairs exact
        conjugates.  Per problem the result contract is that of `ordschur_`; a problem's result does not depend on its
        place in the batch.  An all-true signature stays on the signed kernels: the result is always in the scaled form.
        Above the order cap the real signed single driver runs problem by problem — every problem, while `ordschur_`
        sends a problem with a purely real spectrum through the complex kernel.

        dgordschur_batch_(problems, select, wantZ=True, infos_out=None): `problems` a list of real
        GeneralizedPeriodicSchur of equal order, period, orientation, schurindex (1 or p) and S, with writable
        Fortran-ordered float64 factors; each is mutated (Ts, Z, values, alpha, beta, alphascale, stats) and the list
        returned.  The `stats` of a problem are the call's, with `nsweeps` its own swap count; the call's own are left
        in `self.dgordschur_batch_stats`, the swap counts in `self.dgordschur_batch_nswaps` ([nb]).
        dgordschur_batch_(T, Z, select, S=..., lr=..., schurindex=..., wantZ=True, infos_out=None): the torch outputs
        of the device-resident dgpschur_batch_ ([nb, p, n, n] float64 tensors; Z may be None with wantZ=False) and
        the signature of that call; returns (T, Z, values, stats), in place or through a copy as ordschur_batch_ does.

        `select` (one member of a conjugate pair takes its partner along), rejected swaps and `infos_out` as
        ordschur_batch_."""
        return self._ordschur_batch_(_DG, "dgordschur_batch", problems, args, wantZ, infos_out, lr, schurindex, True, S)

    def dgordschur_batch(self, problems, *args, **kw):
        """Copying form of dgordschur_batch_: the decompositions are left untouched (device tensors are copied too)."""
        return self._ordschur_batch(_DG, self.dgordschur_batch_, problems, args, kw, _GORD_WRONG[_DG])

    def eigvecs(self, ps0, select, shifted=True, method="ordschur"):
        """LinearAlgebra.eigvecs(ps::PeriodicSchur, select; shifted) — src/vectors.jl:25-138: selected right
        eigenvectors of the product (and of its circular shifts).  A loop of `ordschur!` calls (on the device) that
        brings one selected eigenvalue (or conjugate pair) after the other to the top, where its vector is read off
        the leading Schur vectors; for a pair the 2x2 cyclic problem is solved (babd.jl, here a dense 2p x 2p solve).
        `select` is completed to conjugate pairs for a real decomposition (vectors.jl:42-62); `ps0` is not modified.
        Returns a list of p (shifted) or one complex n x nvec matrices, normalised so that A_l v_l = mu v_{l+1},
        mu^p = lambda_k (left orientation).

        method="backsub": periodic back-substitution on the device instead (psd_?_eigvecs: no reordering, one call for
        all selected vectors; see `_eigvecs_backsub`).  The counters of that call are left in `self.eigvecs_stats`."""
        import copy

        if method == "backsub":
            return self._eigvecs_backsub(ps0, select, shifted)
        if method != "ordschur":
            raise ValueError(f"unknown method {method!r}: 'ordschur' or 'backsub'")
        if isinstance(ps0, PartialPeriodicSchur):
            return self._partial_eigvecs(ps0, select, shifted)
        if isinstance(ps0, GeneralizedPeriodicSchur) and not all(ps0.S):
            # (the reordering below applies every factor forwards: its vectors would be wrong)
            raise NotImplementedPSD("eigvecs of a signed GeneralizedPeriodicSchur: use Engine.geigvecs")
        if len(ps0.Z) == 0 or ps0.Z[0].shape[0] == 0:
            raise ValueError("eigvecs requires Schur vectors in the PSD")  # vectors.jl:30-32
        n, m = ps0.Z[0].shape
        select = [bool(x) for x in select]
        if len(select) != m:
            raise ValueError("length of `select` must correspond to rank of Schur (sub-)space")  # vectors.jl:34-36
        real = not np.iscomplexobj(ps0.Ts[0])
        dt = np.float64 if real else np.complex128
        ps = PeriodicSchur([np.array(t, dtype=dt, order="F") for t in ps0.Ts],
                           [np.array(z, dtype=dt, order="F") for z in ps0.Z], np.array(ps0.values, dtype=complex),
                           ps0.orientation, ps0.schurindex)
        p = ps.period
        left = ps.orientation == "L"
        if not all(select):
            if real:  # vectors.jl:42-62
                j = 0
                while j < m:
                    if ps.values[j].imag != 0 and j + 1 < m:
                        if select[j] or select[j + 1]:
                            select[j] = select[j + 1] = True
                        j += 2
                    else:
                        j += 1
            self.ordschur_(ps, select)
        nvec = sum(select)
        sel = [k < nvec for k in range(m)]
        nmat = p if shifted else 1
        Vs = [np.zeros((n, nvec), dtype=np.complex128, order="F") for _ in range(nmat)]
        k = 0
        while k < nvec:
            lam = complex(ps.values[0])
            mu = lam ** (1.0 / p)
            if real and lam.imag != 0:
                # the 2x2 cyclic problem (vectors.jl:73-112): | D1 0 .. Lp ; L1 D2 .. ; .. Lp-1 Dp | x = e1 with the
                # first row replaced by the normalisation x_1[1] + x_1[2] = 1
                M = np.zeros((2 * p, 2 * p), dtype=np.complex128)
                for l in range(p):
                    M[2 * l:2 * l + 2, 2 * l:2 * l + 2] += -mu * np.eye(2)
                for l in range(1, p + 1):
                    lx = l if left else (p + 1 - l)
                    blk = ps.Ts[l - 1][0:2, 0:2]
                    r = lx % p  # block column lx (1-based) couples into block row lx + 1 (cyclically)
                    M[2 * r:2 * r + 2, 2 * (lx - 1):2 * (lx - 1) + 2] += blk
                y = np.zeros(2 * p, dtype=np.complex128)
                M[0, :] = 0.0
                M[0, 0:2] = 1.0
                y[0] = 1.0
                x = np.linalg.solve(M, y)
                t = 1.0 / np.linalg.norm(x[0:2])
                for l in range(1, nmat + 1):
                    i0 = (l - 1) * 2 if left else (0 if l == 1 else (p + 1 - l) * 2)
                    Vs[l - 1][:, k] = t * (ps.Z[l - 1][:, 0:2] @ x[i0:i0 + 2])
                    Vs[l - 1][:, k + 1] = np.conj(Vs[l - 1][:, k])
                nl = 2
            else:  # A_1 x_1 = T_1[1,1] Z_2[:,1] = mu x_2, ... (vectors.jl:113-129)
                fac = 1.0 + 0.0j
                for l in range(1, nmat + 1):
                    Vs[l - 1][:, k] = fac * ps.Z[l - 1][:, 0]
                    fac *= ps.Ts[l - 1][0, 0] / mu
                nl = 1
            for q in range(nl):
                sel[q] = False
            self.ordschur_(ps, sel)  # vectors.jl:133
            k += nl
            sel = sel[nl:] + sel[:nl]  # circshift!(sel, -nl)
        return Vs

    @staticmethod
    def _evec_values(ps, cplx):
        """The eigenvalue arguments of psd_?_eigvecs: (wr, wi) or (alpha, beta, ascale)."""
        if not cplx:
            v = np.asarray(ps.values, dtype=np.complex128)
            return [np.ascontiguousarray(v.real), np.ascontiguousarray(v.imag)]
        if isinstance(ps, GeneralizedPeriodicSchur):
            return [np.ascontiguousarray(ps.alpha, dtype=np.complex128), np.ascontiguousarray(ps.beta, dtype=np.float64),
                    np.ascontiguousarray(ps.alphascale, dtype=np.int32)]
        v = np.ascontiguousarray(ps.values, dtype=np.complex128)
        return [v, np.ones(len(v)), np.zeros(len(v), dtype=np.int32)]

    @staticmethod
    def _evec_ptrs(vals):
        dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        return [v.ctypes.data_as(i32p if v.dtype == np.int32 else dp) for v in vals]

    def _eigvecs_backsub(self, ps0, select, shifted):
        """eigvecs(ps, select; shifted) by periodic back-substitution (psd_d_eigvecs / psd_z_eigvecs): the triangular
        factors are solved bottom up on the device and V_l = Z_l X_l is formed on the matrix cores.  Same result contract
        as the default method (src/vectors.jl:25-138), plus: ||V_1[:, j]|| = 1 with its largest-modulus entry real and
        positive; a zero eigenvalue gives a column of NaNs (counted in eigvecs_stats.nzero).  PartialPeriodicSchur: the
        projected k x k problem, then Z_l times its vectors.  A signed GeneralizedPeriodicSchur: NotImplementedPSD."""
        if isinstance(ps0, PartialPeriodicSchur):
            return self._partial_eigvecs(ps0, select, shifted, "backsub")
        if isinstance(ps0, GeneralizedPeriodicSchur) and not all(ps0.S):
            raise NotImplementedPSD("eigenvectors of a signed GeneralizedPeriodicSchur")
        if len(ps0.Z) == 0 or ps0.Z[0].shape[0] == 0:
            raise ValueError("eigvecs requires Schur vectors in the PSD")  # vectors.jl:30-32
        n, m = ps0.Z[0].shape
        if len(select) != m:
            raise ValueError("length of `select` must correspond to rank of Schur (sub-)space")  # vectors.jl:34-36
        cplx = np.iscomplexobj(ps0.Ts[0])
        if any(np.iscomplexobj(t) != cplx for t in ps0.Ts) or any(np.iscomplexobj(z) != cplx for z in ps0.Z):
            # (a real quasi-triangular factor sent through the complex path would lose its 2x2 row blocks)
            raise TypeError("eigvecs: the factors T and the Schur vectors Z must be all real or all complex")
        dt = np.complex128 if cplx else np.float64
        Ts = [np.asfortranarray(t, dtype=dt) for t in ps0.Ts]  # (read only: ps0 is never written)
        Zs = [np.asfortranarray(z, dtype=dt) for z in ps0.Z]
        p = len(Ts)
        vals = self._evec_values(ps0, cplx)
        sel = (C.c_uint8 * m)(*[1 if x else 0 for x in select])
        st = EvecStats()
        info = C.c_int(0)
        fn = self.lib.psd_z_eigvecs if cplx else self.lib.psd_d_eigvecs
        args = [self.ctx, n, p, self._ptrs(Ts), self._ptrs(Zs)] + self._evec_ptrs(vals) + [None,
                ps0.orientation.encode(), ps0.schurindex, sel, m, int(bool(shifted))]
        fn(*args, None, 0, C.byref(st), C.byref(info))  # size query: select completed, st.nvec
        self._raise(info.value)
        nvec = st.nvec
        Vs = [np.zeros((n, nvec), dtype=np.complex128, order="F") for _ in range(p if shifted else 1)]
        fn(*args, self._ptrs(Vs), nvec, C.byref(st), C.byref(info))
        self._raise(info.value)
        self.eigvecs_stats = st
        return Vs

    def eigvecs_dev(self, dT, dZ, values, select, lr="R", schurindex=1, shifted=True, S=None):
        """Device-resident eigvecs by back-substitution (psd_d_eigvecs_dev / psd_z_eigvecs_dev), mirroring pschur_dev:
        dT, dZ are torch device tensors holding the [p][n][n] column-major blocks pschur_dev / zpschur_dev leave (float64
        or complex128, user order, T[schurindex-1] quasi-triangular); `values` the eigenvalues they returned.  Returns a
        list of (p if shifted else 1) torch device tensors n x nvec (complex128) and leaves the counters in
        `self.eigvecs_stats`."""
        import torch

        p, n = dT.shape[0], dT.shape[1]
        if dZ is None:
            raise ValueError("eigvecs requires Schur vectors in the PSD")
        if S is not None and not all(S):
            raise NotImplementedPSD("eigenvectors of a signed GeneralizedPeriodicSchur")
        cplx = dT.is_complex()
        if dZ.dtype != dT.dtype:
            raise TypeError("eigvecs_dev: dT and dZ must have the same dtype (float64 or complex128)")
        if len(select) != n:
            raise ValueError("length of `select` must correspond to rank of Schur (sub-)space")
        v = np.asarray(values, dtype=np.complex128)
        vals = ([v, np.ones(n), np.zeros(n, dtype=np.int32)] if cplx
                else [np.ascontiguousarray(v.real), np.ascontiguousarray(v.imag)])
        sel = (C.c_uint8 * n)(*[1 if x else 0 for x in select])
        st = EvecStats()
        info = C.c_int(0)
        fn = self.lib.psd_z_eigvecs_dev if cplx else self.lib.psd_d_eigvecs_dev
        args = [self.ctx, n, p, C.c_void_p(dT.data_ptr()), C.c_void_p(dZ.data_ptr())] + self._evec_ptrs(vals) + [
            None, char_lr(lr).encode(), int(schurindex), sel, n, int(bool(shifted))]
        fn(*args, None, 0, C.byref(st), C.byref(info))
        self._raise(info.value)
        nvec = st.nvec
        nmat = p if shifted else 1
        dV = torch.empty((nmat, max(nvec, 1), n), dtype=torch.complex128, device=dT.device)
        torch.cuda.synchronize(dT.device)
        fn(*args, C.c_void_p(dV.data_ptr()), nvec, C.byref(st), C.byref(info))
        self._raise(info.value)
        self.eigvecs_stats = st
        return [dV[l, :nvec, :].transpose(0, 1) for l in range(nmat)]

    @staticmethod
    def _batch_select(select, nb, n):
        """[nb][n] flags (uint8, contiguous, a copy) from [nb][n] or one [n] row for every problem."""
        sel = np.asarray(select)
        if sel.ndim == 1 and sel.shape[0] == n:
            sel = np.broadcast_to(sel, (nb, n))
        if sel.shape != (nb, n):
            raise ValueError("argument 9 invalid: `select` must be [nb][n] flags or one row of n "
                             "(its length must correspond to the rank of the Schur space)")  # vectors.jl:34-36
        return np.ascontiguousarray(sel.astype(bool), dtype=np.uint8)

    def _eigvecs_batch_call(self, fam, dev, nb, n, p, T, Z, ev, orient, si, sel, shifted, V=None, maxvec=0, left=False):
        """One call of psd_?_eigvecs_batch[_dev] (left: psd_?_leigvecs_batch[_dev]) on packed factors (T, Z, V: ctypes
        arguments; ev: the eigenvalue arguments).  Without V the size query (select completed); with V the stats and
        counters of the call are left in self.eigvecs_batch_*.  Returns the vectors per problem, nvec."""
        nvec = (C.c_int * nb)()
        cnts = np.zeros((nb, 3), dtype=np.int32)
        st = BevecStats()
        info = C.c_int(0)
        fn = getattr(self.lib, f"psd_{fam.tag}_{'l' if left else ''}eigvecs_batch{'_dev' if dev else ''}")
        fn(self.ctx, nb, n, p, T, Z, *self._evec_ptrs(ev), orient.encode(), int(si),
           sel.ctypes.data_as(C.POINTER(C.c_uint8)), int(bool(shifted)), V, maxvec, nvec,
           cnts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st), C.byref(info))
        self._raise(info.value)
        if V is not None:
            self.eigvecs_batch_stats = st
            self.eigvecs_batch_counts = cnts
        return nvec

    def _geigvecs_batch_call(self, fam, dev, nb, n, p, T, Z, S, orient, si, sel, shifted, V=None, maxvec=0):
        """One call of psd_?_geigvecs_batch[_dev] on packed factors (T, Z, V: ctypes arguments; S: the signature, a list
        of p flags).  Without V the size query (the Float64 entry completes `sel` to whole pairs); with V the stats and
        counters of the call are left in self.eigvecs_batch_*.  Returns nvec and the scalars a [nb, maxvec, p] (None
        without V)."""
        nvec = (C.c_int * nb)()
        cnts = np.zeros((nb, 3), dtype=np.int32)
        st = BevecStats()
        info = C.c_int(0)
        a = None if V is None else np.zeros((nb, maxvec, p), dtype=np.complex128)
        fn = getattr(self.lib, f"psd_{fam.tag}_geigvecs_batch{'_dev' if dev else ''}")
        fn(self.ctx, nb, n, p, T, Z, (C.c_uint8 * p)(*[1 if x else 0 for x in S]), orient.encode(), int(si),
           sel.ctypes.data_as(C.POINTER(C.c_uint8)), int(bool(shifted)), V, maxvec,
           None if a is None else a.ctypes.data_as(C.POINTER(C.c_double)), nvec,
           cnts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st), C.byref(info))
        self._raise(info.value)
        if V is not None:
            self.eigvecs_batch_stats = st
            self.eigvecs_batch_counts = cnts
        return nvec, a

    @staticmethod
    def _bevec_sides(side):
        """the calls of side = "R" (right vectors), "L" (left) or "B" (both): whether each is the left entry"""
        try:
            return {"R": (False,), "L": (True,), "B": (False, True)}[side]
        except (KeyError, TypeError):
            raise ValueError(f'side must be "R", "L" or "B", not {side!r}') from None

    def _eigvecs_batch(self, fam, name, wrong, problems, args, shifted, lr, schurindex, side="R"):
        """eigvecs_batch / zeigvecs_batch."""
        sides = self._bevec_sides(side)
        if hasattr(problems, "data_ptr"):
            if len(args) != 3:
                raise TypeError(f"{name}(T, Z, values, select, lr=..., schurindex=...)")
            Vs, nvec = self._eigvecs_batch_dev(fam, name, wrong, problems, args[0], args[1], args[2], lr, schurindex,
                                               shifted, sides)
            return (*Vs, nvec)
        if len(args) != 1:
            raise TypeError(f"{name}(problems, select, shifted=True)")
        Vs, nvec, _, _ = self._eigvecs_batch_host(fam, name, wrong, list(problems), args[0], shifted, sides)
        out = [[[np.asfortranarray(v[:, :nvec[q]]) for v in Vq] for q, Vq in enumerate(V)] for V in Vs]
        return out[0] if len(sides) == 1 else tuple(out)

    def _eigvecs_batch_host(self, fam, name, wrong, problems, select, shifted, sides):
        """The list form of _eigvecs_batch and eigcond_batch: per side the blocks as the entry leaves them (per problem
        nmat matrices n x maxvec), and nvec, n, maxvec."""
        nb = len(problems)
        if nb == 0:
            self.eigvecs_batch_stats = BevecStats()
            self.eigvecs_batch_counts = np.zeros((0, 3), dtype=np.int32)
            return [[] for _ in sides], [], 0, 0
        n, p, orient, si, Ts, Zs = self._batch_decomps(fam, name, wrong, problems, needZ=True, work=False)
        sel = self._batch_select(select, nb, n)
        if fam is _D:
            vals = np.array([np.asarray(ps.values, dtype=np.complex128) for ps in problems])
            ev = [np.ascontiguousarray(vals.real), np.ascontiguousarray(vals.imag)]
        else:
            vals = [self._evec_values(ps, True) for ps in problems]
            ev = [np.ascontiguousarray(np.array([v[k] for v in vals])) for k in range(3)]
        call = (fam, False, nb, n, p, self._ptrs(Ts), self._ptrs(Zs), ev, orient, si, sel, shifted)
        maxvec = max(self._eigvecs_batch_call(*call, left=sides[0]))
        nmat = p if shifted else 1
        out = []
        for left in sides:
            Vs = [np.zeros((n, maxvec), dtype=np.complex128, order="F") for _ in range(nb * nmat)]
            nvec = self._eigvecs_batch_call(*call, self._ptrs(Vs), maxvec, left=left)
            out.append([Vs[q * nmat:(q + 1) * nmat] for q in range(nb)])
        return out, list(nvec), n, maxvec

    def _eigvecs_batch_dev(self, fam, name, wrong, T, Z, values, select, lr, schurindex, shifted, sides=(False,)):
        """The device form: the blocks [nb, nmat, n, maxvec] of every side, and nvec."""
        import torch

        if Z is None:
            raise ValueError("eigvecs requires Schur vectors in the PSD")
        nb, p, n = self._dev_batch(fam, name, wrong, T, Z, mixed=True)
        orient = char_lr(lr)
        nmat = p if shifted else 1
        if nb == 0:
            self.eigvecs_batch_stats = BevecStats()
            self.eigvecs_batch_counts = np.zeros((0, 3), dtype=np.int32)
            return ([torch.zeros((0, nmat, n, 0), dtype=torch.complex128, device=T.device) for _ in sides],
                    np.zeros(0, dtype=np.int32))
        sel = self._batch_select(select, nb, n)
        vals = np.ascontiguousarray(values, dtype=np.complex128)
        if vals.shape != (nb, n):
            raise DimensionMismatch("values must be [nb, n]")
        # (the complex entry as eigvecs_dev passes them: alpha = values, beta = 1, scale 0)
        ev = ([np.ascontiguousarray(vals.real), np.ascontiguousarray(vals.imag)] if fam is _D
              else [vals, np.ones((nb, n)), np.zeros((nb, n), dtype=np.int32)])
        dT, dZ = _dev_blocks(T, fam, "readonly"), _dev_blocks(Z, fam, "readonly")
        call = (fam, True, nb, n, p, C.c_void_p(dT.data_ptr()), C.c_void_p(dZ.data_ptr()), ev, orient, schurindex, sel,
                shifted)
        torch.cuda.synchronize(T.device)
        maxvec = max(self._eigvecs_batch_call(*call, left=sides[0]))
        out = []
        for left in sides:
            dV = torch.empty((nb, nmat, max(maxvec, 1), n), dtype=torch.complex128, device=T.device)
            if maxvec == 0:
                dV.zero_()
            torch.cuda.synchronize(T.device)
            nvec = self._eigvecs_batch_call(*call, C.c_void_p(dV.data_ptr()), max(maxvec, 1), left=left)
            out.append(dV[:, :, :maxvec, :].transpose(2, 3))
        return out, np.array(list(nvec), dtype=np.int32)

    def eigcond_batch(self, problems, *args, lr="R", schurindex=1):
        """Reciprocal condition numbers of the eigenvalues of MANY small periodic Schur decompositions with respect to
        every factor (psd_eigcond_batch: the periodic form of xTRSNA's S), with the right and left eigenvectors they are
        computed from.  Float64 or ComplexF64, picked from the dtype; all-true signature.

        eigcond_batch(problems, select): returns (s, V, W); V and W what eigvecs_batch(problems, select, side="B")
        returns (every factor's vectors), s a list of [p, nvec_q] arrays.
        eigcond_batch(T, Z, values, select, lr=..., schurindex=...): the device form; returns (s, V, W, nvec) with V, W
        as the device form of eigvecs_batch returns them and s a host array [nb, p, maxvec] (zero at and beyond nvec[q]).

        With mu_j the principal p-th root of eigenvalue j, v_l and w_l its right and left vectors (l + 1 cyclic):
        lr "L": s[l, j] = |w_l' v_l| / (||w_{l+1}|| ||v_l||);  lr "R": s[l, j] = |w_l' v_l| / (||w_l|| ||v_{l+1}||).
        To first order |d lambda_j / lambda_j| <= sum_l ||dA_l||_2 / (|mu_j| s[l, j]).  A zero eigenvalue gives NaN.
        The stats of the eigenvector calls are left as by eigvecs_batch(..., side="B")."""
        sides = (False, True)
        if hasattr(problems, "data_ptr"):
            if len(args) != 3:
                raise TypeError("eigcond_batch(T, Z, values, select, lr=..., schurindex=...)")
            fam = _Z if problems.is_complex() else _D
            wrong = TypeError("eigcond_batch: T and Z must both be float64 or both complex128")
            (V, W), nvec = self._eigvecs_batch_dev(fam, "eigcond_batch", wrong, problems, args[0], args[1], args[2], lr,
                                                   schurindex, True, sides)
            nb, p, n, maxvec = V.shape
            s = np.zeros((nb, maxvec, p))
            if nb > 0 and maxvec > 0:
                # (the blocks behind the views: [nb][p][maxvec][n], contiguous)
                dV, dW = V.transpose(2, 3), W.transpose(2, 3)
                assert dV.is_contiguous() and dW.is_contiguous()
                self._eigcond_call(True, nb, n, p, C.c_void_p(dV.data_ptr()), C.c_void_p(dW.data_ptr()), char_lr(lr),
                                   maxvec, nvec, s)
            return np.ascontiguousarray(s.transpose(0, 2, 1)), V, W, nvec
        if len(args) != 1:
            raise TypeError("eigcond_batch(problems, select)")
        problems = list(problems)
        fam = _Z if problems and len(problems[0].Ts) > 0 and np.iscomplexobj(problems[0].Ts[0]) else _D
        wrong = TypeError("eigcond_batch: the problems of a batch must all be Float64 or all ComplexF64")
        (V, W), nvec, n, maxvec = self._eigvecs_batch_host(fam, "eigcond_batch", wrong, problems, args[0], True, sides)
        nb = len(problems)
        if nb == 0:
            return [], [], []
        p = len(V[0])
        s = np.zeros((nb, maxvec, p))
        if maxvec > 0:
            self._eigcond_call(False, nb, n, p, self._ptrs([v for Vq in V for v in Vq]),
                               self._ptrs([w for Wq in W for w in Wq]), problems[0].orientation, maxvec, nvec, s)
        trim = [[[np.asfortranarray(v[:, :nvec[q]]) for v in Xq] for q, Xq in enumerate(X)] for X in (V, W)]
        return [np.ascontiguousarray(s[q, :nvec[q], :].T) for q in range(nb)], trim[0], trim[1]

    def _eigcond_call(self, dev, nb, n, p, V, W, orient, maxvec, nvec, s):
        """psd_eigcond_batch[_dev] on the blocks of both sides (V, W: ctypes arguments); s [nb][maxvec][p] is filled"""
        info = C.c_int(0)
        nv = (C.c_int * nb)(*[int(x) for x in nvec])
        fn = getattr(self.lib, "psd_eigcond_batch_dev" if dev else "psd_eigcond_batch")
        fn(self.ctx, nb, n, p, V, W, orient.encode(), maxvec, nv, s.ctypes.data_as(C.POINTER(C.c_double)),
           C.byref(info))
        self._raise(info.value)

    # ---- periodic Sylvester solves and the condition of an invariant periodic subspace ----------------------------
    def _bsylv_inputs(self, name, problems, m, lr, schurindex):
        """What psylvester_batch and subspacecond_batch share: (fam, dev, nb, n, p, T argument, orient, schurindex, m
        as int32 [nb], xb, keep-alive); `problems` a list of PeriodicSchur or a GPU tensor [nb, p, n, n]."""
        wrong = TypeError(f"{name}: the problems of a batch must all be Float64 or all ComplexF64")
        if hasattr(problems, "data_ptr"):
            import torch

            if problems.dtype not in (torch.float64, torch.complex128):
                raise TypeError(f"{name}: a float64 or complex128 tensor")
            fam = _Z if problems.is_complex() else _D
            nb, p, n = self._dev_batch(fam, name, wrong, problems)
            orient, si = char_lr(lr), int(schurindex)
            keep = _dev_blocks(problems, fam, "readonly") if nb else problems
            T = C.c_void_p(keep.data_ptr())
            dev = True
        else:
            problems = list(problems)
            nb = len(problems)
            if nb == 0:
                return None
            fam = _Z if len(problems[0].Ts) > 0 and np.iscomplexobj(problems[0].Ts[0]) else _D
            n, p, orient, si, keep = self._batch_decomps(fam, name, wrong, problems, needZ=False, work=False)
            orient = char_lr(orient)
            T = self._ptrs(keep)
            dev = False
        mm = np.asarray(m)
        if mm.ndim == 0:
            mm = np.full(nb, mm)
        if mm.shape != (nb,) or not np.issubdtype(mm.dtype, np.integer):
            raise DimensionMismatch(f"{name}: m must be an int or [nb] ints")
        mm = np.ascontiguousarray(mm, dtype=np.int32)
        xb = max(1, int(np.max(mm.astype(np.int64) * (n - mm)))) if nb else 1
        return fam, dev, nb, n, p, T, orient, si, mm, xb, keep

    @staticmethod
    def _bsylv_blocks(buf, mm, n, q):
        """the m x k matrices of problem q from its flat blocks"""
        mq = int(mm[q])
        return [np.asfortranarray(b[:mq * (n - mq)].reshape((mq, n - mq), order="F")) for b in buf]

    def _bsylv_dev_x(self, X, mm, n):
        """the device blocks [nb, p, xb] as the device forms return them: [nb, p, m, k] views for one common m"""
        nb, p = X.shape[0], X.shape[1]
        if nb > 0 and np.all(mm == mm[0]) and 0 < mm[0] < n:
            mq = int(mm[0])
            return X[:, :, :mq * (n - mq)].reshape(nb, p, n - mq, mq).transpose(2, 3)
        return X

    def psylvester_batch(self, problems, m, C=None, trans=False, lr="R", schurindex=1, infos_out=None):
        """Periodic Sylvester solves on the off-diagonal block of MANY small periodic Schur forms of one shape in ONE
        call (psd_?_psylv_batch).  Float64 or ComplexF64, picked from the dtype; all-true signature (a signed
        GeneralizedPeriodicSchur: NotImplementedPSD).

        Problem q is split at m[q] (`m`: an int or [nb] ints, 0 <= m <= n, not inside a 2x2 block), k = n - m:
        T_l = [T11_l T12_l; 0 T22_l].  With (a, b) = (l + 1, l) cyclically for orientation "L" and (l, l + 1) for "R",
            S(X)_l = T11_l X_b - X_a T22_l ,   l = 1..p,
        and the call solves S(X) = C, or with trans=True S^H(Y) = C (the adjoint under the Frobenius inner product over
        the stacked blocks).  C=None: C_l = -T12_l; the solution then block-diagonalises the form,
        T_l [X_b; I] = [X_a; I] T22_l, so that Y_l = Z_l [X_l; I] spans the complementary periodic invariant
        subspace (A_l Y_b = Y_a T22_l).  There is no scale factor (xTRSYL carries one); above order 128: NotImplementedPSD (use `psylvester` per problem).

        psylvester_batch(problems, m, C=None, trans=False): `problems` a list of PeriodicSchur, `C` per problem p
        matrices m x k; returns per problem the p matrices X_l.
        psylvester_batch(T, m, C=None, trans=False, lr=..., schurindex=...): T a GPU tensor [nb, p, n, n] as
        pschur_batch_ / ordschur_batch_ return it (only read, not copied in that layout); C and the result GPU tensors
        [nb, p, m, k] for one common m, otherwise [nb, p, xb] flat column-major blocks, xb = max m (n - m).  C is not
        written.

        A problem whose small solve is rejected (T11 and T22 share an eigenvalue of the product) or whose solution is
        not finite has X = NaN; the others complete, and SingularException is raised afterwards, or the codes go to
        `infos_out`.  A problem's result does not depend on its place in the batch, bit for bit.  Stats:
        `self.psylvester_batch_stats` (BsylvStats)."""
        name = "psylvester_batch"
        inp = self._bsylv_inputs(name, problems, m, lr, schurindex)
        self.psylvester_batch_stats = BsylvStats()
        if inp is None:
            if infos_out is not None:
                infos_out[:] = []
            return []
        fam, dev, nb, n, p, T, orient, si, mm, xb, keep = inp
        if dev:
            import torch

            dt = getattr(torch, np.dtype(fam.dtype).name)
            X = torch.zeros((nb, p, xb), dtype=dt, device=problems.device)
            if C is not None:
                if C.dim() == 4:  # [nb, p, m, k] of one common m
                    mq = int(mm[0]) if nb else 0
                    if nb and (not np.all(mm == mq) or tuple(C.shape) != (nb, p, mq, n - mq)):
                        raise DimensionMismatch(f"{name}: C must be [nb, p, m, k] (one common m) or [nb, p, xb]")
                    X[:, :, :mq * (n - mq)] = C.to(dt).transpose(2, 3).reshape(nb, p, mq * (n - mq))
                elif tuple(C.shape) == (nb, p, xb):
                    X.copy_(C.to(dt))
                else:
                    raise DimensionMismatch(f"{name}: C must be [nb, p, m, k] (one common m) or [nb, p, xb]")
            if nb == 0:
                if infos_out is not None:
                    infos_out[:] = []
                return X
            torch.cuda.synchronize(problems.device)
            Xarg = _ct.c_void_p(X.data_ptr())
        else:
            bufs = [np.zeros(xb, dtype=fam.dtype) for _ in range(nb * p)]
            if C is not None:
                C = list(C)
                if len(C) != nb:
                    raise DimensionMismatch(f"{name}: one list of p right-hand sides per problem")
                for q, Cq in enumerate(C):
                    Cq = list(Cq)
                    mq = int(mm[q])
                    if len(Cq) != p or any(np.shape(c) != (mq, n - mq) for c in Cq):
                        raise DimensionMismatch(f"{name}: the right-hand sides of a problem are p matrices m x k")
                    if fam is _D and any(np.iscomplexobj(c) for c in Cq):
                        raise TypeError(f"{name}: the problems of a batch must all be Float64 or all ComplexF64")
                    for l, c in enumerate(Cq):
                        bufs[q * p + l][:mq * (n - mq)] = np.asarray(c, dtype=fam.dtype).reshape(-1, order="F")
            Xarg = self._ptrs(bufs)
        infos, st, info = (_ct.c_int * nb)(), BsylvStats(), _ct.c_int(0)
        fn = getattr(self.lib, f"psd_{fam.tag}_psylv_batch{'_dev' if dev else ''}")
        fn(self.ctx, nb, n, p, T, orient.encode(), si, mm.ctypes.data_as(_ct.POINTER(_ct.c_int)), Xarg, xb, int(bool(trans)),
           int(C is None), infos, _ct.byref(st), _ct.byref(info))
        self.psylvester_batch_stats = st

        def result():
            if dev:
                return self._bsylv_dev_x(X, mm, n)
            return [self._bsylv_blocks(bufs[q * p:(q + 1) * p], mm, n, q) for q in range(nb)]

        return self._batch_finish(info.value, infos, infos_out, self._raise_ord, True, result)

    def subspacecond_batch(self, problems, m, want_x=False, lr="R", schurindex=1, infos_out=None):
        """How well separated the leading invariant periodic subspace of MANY small periodic Schur forms is: the
        periodic form of xTRSEN's S and SEP (psd_?_subcond_batch), the follow-up of ordschur_batch.  Float64 or
        ComplexF64, picked from the dtype; all-true signature (a signed GeneralizedPeriodicSchur: NotImplementedPSD).

        With the split m (an int or [nb] ints), the operator S and X the solution of S(X) = -T12 as in
        `psylvester_batch`:
            s[q, l] = 1 / sqrt(1 + ||X_l||_F^2): the reciprocal of the Frobenius bound on the norm of the spectral
                      projector of factor l (p = 1: xTRSEN's S);
            sep[q]  = 1 / est, est the estimate of ||S^-1||_1 on the p m k stacked unknowns (blocks in user order, each
                      column-major) by LAPACK's xLACN2 — real variant for Float64, complex for ComplexF64, at most 5
                      iterations and the final alternating-sign vector (p = 1: xTRSEN's SEP).
        m = 0 or m = n: s = 1, sep = inf, X empty.  There is no scale factor; above order 128: NotImplementedPSD (use
        `subspacecond` per problem).

        subspacecond_batch(problems, m, want_x=False) with a list of PeriodicSchur, or
        subspacecond_batch(T, m, want_x=False, lr=..., schurindex=...) with a GPU tensor [nb, p, n, n] (only read):
        returns (s, sep), numpy arrays [nb, p] and [nb], with want_x also X as `psylvester_batch` returns it.

        A problem whose small solve is rejected or whose numbers are not finite gets s = 0, sep = 0, X = NaN; the others
        complete, and SingularException is raised afterwards, or the codes go to `infos_out`.  A problem's numbers do
        not depend on its place in the batch, bit for bit.  Stats: `self.subspacecond_batch_stats` (BsylvStats)."""
        name = "subspacecond_batch"
        inp = self._bsylv_inputs(name, problems, m, lr, schurindex)
        self.subspacecond_batch_stats = BsylvStats()
        if inp is None:
            if infos_out is not None:
                infos_out[:] = []
            return (np.zeros((0, 0)), np.zeros(0), []) if want_x else (np.zeros((0, 0)), np.zeros(0))
        fam, dev, nb, n, p, T, orient, si, mm, xb, keep = inp
        s, sep = np.zeros((nb, p)), np.zeros(nb)
        X = bufs = Xarg = None
        if dev:
            import torch

            if want_x:
                X = torch.zeros((nb, p, xb), dtype=getattr(torch, np.dtype(fam.dtype).name), device=problems.device)
                Xarg = C.c_void_p(X.data_ptr())
            if nb == 0:
                if infos_out is not None:
                    infos_out[:] = []
                return (s, sep, X) if want_x else (s, sep)
            torch.cuda.synchronize(problems.device)
        elif want_x:
            bufs = [np.zeros(xb, dtype=fam.dtype) for _ in range(nb * p)]
            Xarg = self._ptrs(bufs)
        infos, st, info = (C.c_int * nb)(), BsylvStats(), C.c_int(0)
        dp = C.POINTER(C.c_double)
        fn = getattr(self.lib, f"psd_{fam.tag}_subcond_batch{'_dev' if dev else ''}")
        fn(self.ctx, nb, n, p, T, orient.encode(), si, mm.ctypes.data_as(C.POINTER(C.c_int)), s.ctypes.data_as(dp),
           sep.ctypes.data_as(dp), Xarg, xb, infos, C.byref(st), C.byref(info))
        self.subspacecond_batch_stats = st

        def result():
            if not want_x:
                return s, sep
            if dev:
                return s, sep, self._bsylv_dev_x(X, mm, n)
            return s, sep, [self._bsylv_blocks(bufs[q * p:(q + 1) * p], mm, n, q) for q in range(nb)]

        return self._batch_finish(info.value, infos, infos_out, self._raise_ord, True, result)

    # ---- the same for one form of any order ------------------------------------------------------------------------
    def _sylv_inputs(self, name, P, m, lr, schurindex, dev):
        """(fam, n, p, T argument, orient, schurindex, m, keep-alive) of a single-problem call: `P` a PeriodicSchur, or
        with `dev` a GPU tensor [p, n, n]"""
        if dev:
            if not hasattr(P, "data_ptr") or P.dim() != 3:
                raise DimensionMismatch(f"{name}: one [p, n, n] GPU tensor of square factors")
            P = P.unsqueeze(0)
        elif hasattr(P, "data_ptr"):
            raise TypeError(f"{name}: a PeriodicSchur (GPU tensors: {name}_dev)")
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)):
            raise DimensionMismatch(f"{name}: m must be an int")
        fam, _, _, n, p, T, orient, si, mm, _, keep = self._bsylv_inputs(name, P if dev else [P], int(m), lr, schurindex)
        return fam, n, p, T, orient, si, int(mm[0]), keep

    def _sylv_finish(self, info, info_out, result):
        """a fatal code raises; the singular code goes to the list `info_out` with the result (X = NaN, s = 0, sep = 0),
        or raises, as the per-problem codes of the batch wrappers do"""
        return self._batch_finish(info, [info if info == 3000 else 0], info_out, self._raise_ord, True, result)

    def _psylvester(self, name, P, m, C, trans, lr, schurindex, dev, info_out):
        fam, n, p, T, orient, si, m, keep = self._sylv_inputs(name, P, m, lr, schurindex, dev)
        k = n - m if 0 <= m <= n else 0
        mq = m if 0 <= m <= n else 0
        if dev:
            import torch

            dt = getattr(torch, np.dtype(fam.dtype).name)
            X = torch.zeros((p, k, mq), dtype=dt, device=P.device)  # (column-major m x k blocks)
            if C is not None:
                if not hasattr(C, "data_ptr") or tuple(C.shape) != (p, mq, k):
                    raise DimensionMismatch(f"{name}: C must be a [p, m, k] GPU tensor")
                X.copy_(C.to(dt).transpose(1, 2))
            torch.cuda.synchronize(P.device)
            Xarg = _ct.c_void_p(X.data_ptr())
        else:
            bufs = [np.zeros((mq, k), dtype=fam.dtype, order="F") for _ in range(p)]
            if C is not None:
                C = list(C)
                if len(C) != p or any(np.shape(c) != (mq, k) for c in C):
                    raise DimensionMismatch(f"{name}: the right-hand sides are p matrices m x k")
                if fam is _D and any(np.iscomplexobj(c) for c in C):
                    raise TypeError(f"{name}: complex right-hand sides for a Float64 form")
                for b, c in zip(bufs, C):
                    b[...] = c
            Xarg = self._ptrs(bufs)
        st, info = SylvStats(), _ct.c_int(0)
        fn = getattr(self.lib, f"psd_{fam.tag}_psylv{'_dev' if dev else ''}")
        fn(self.ctx, n, p, T, orient.encode(), si, m, Xarg, int(bool(trans)), int(C is None), _ct.byref(st),
           _ct.byref(info))
        self.psylvester_stats = st
        return self._sylv_finish(info.value, info_out, lambda: X.transpose(1, 2) if dev else bufs)

    def psylvester(self, P, m, C=None, trans=False, info_out=None):
        """The periodic Sylvester solve of `psylvester_batch` for ONE PeriodicSchur of any order (psd_?_psylv): with
        the split m, S(X)_l = T11_l X_b - X_a T22_l, solves S(X) = C, with trans=True S^H(Y) = C; C=None: C_l = -T12_l,
        whose solution block-diagonalises the form.  Float64 or ComplexF64 from the dtype; a signed
        GeneralizedPeriodicSchur: NotImplementedPSD.  `C`: p matrices m x k (not written); returns the p matrices X_l.

        The solve is a tiled walk (tile width PSD_SYL_TILE, default 16): for one tile width the result is the same
        bits on every run.  A form whose T11 and T22 share an eigenvalue of the product, or whose solution is not
        finite: X = NaN and SingularException, or with a list `info_out` the code [3000] there.  Stats:
        `self.psylvester_stats` (SylvStats)."""
        return self._psylvester("psylvester", P, m, C, trans, "R", 1, False, info_out)

    def psylvester_dev(self, T, m, C=None, trans=False, lr="R", schurindex=1, info_out=None):
        """`psylvester` on a GPU tensor T [p, n, n] (only read); C and the result are GPU tensors [p, m, k]."""
        return self._psylvester("psylvester_dev", T, m, C, trans, lr, schurindex, True, info_out)

    def _subspacecond(self, name, P, m, want_x, lr, schurindex, dev, info_out):
        fam, n, p, T, orient, si, m, keep = self._sylv_inputs(name, P, m, lr, schurindex, dev)
        k = n - m if 0 <= m <= n else 0
        mq = m if 0 <= m <= n else 0
        s, sep = np.zeros(p), np.zeros(1)
        X = bufs = Xarg = None
        if dev and want_x:
            import torch

            X = torch.zeros((p, k, mq), dtype=getattr(torch, np.dtype(fam.dtype).name), device=P.device)
            Xarg = C.c_void_p(X.data_ptr())
        elif want_x:
            bufs = [np.zeros((mq, k), dtype=fam.dtype, order="F") for _ in range(p)]
            Xarg = self._ptrs(bufs)
        if dev:
            import torch

            torch.cuda.synchronize(P.device)
        st, info = SylvStats(), C.c_int(0)
        dp = C.POINTER(C.c_double)
        fn = getattr(self.lib, f"psd_{fam.tag}_subcond{'_dev' if dev else ''}")
        fn(self.ctx, n, p, T, orient.encode(), si, m, s.ctypes.data_as(dp), sep.ctypes.data_as(dp), Xarg, C.byref(st),
           C.byref(info))
        self.subspacecond_stats = st

        def result():
            if not want_x:
                return s, float(sep[0])
            return s, float(sep[0]), (X.transpose(1, 2) if dev else bufs)

        return self._sylv_finish(info.value, info_out, result)

    def subspacecond(self, P, m, want_x=False, info_out=None):
        """How well separated the leading invariant periodic subspace of ONE PeriodicSchur of any order is
        (psd_?_subcond): s[l] = 1 / sqrt(1 + ||X_l||_F^2) and sep = 1 / est(||S^-1||_1) as `subspacecond_batch` defines
        them, X the solution of S(X) = -T12.  m = 0 or m = n: s = 1, sep = inf, X empty.  Returns (s, sep), s a numpy
        array [p] and sep a float, with want_x also the p matrices X_l.  A singular form: s = 0, sep = 0, X = NaN and
        SingularException, or with a list `info_out` the code [3000] there.  Stats: `self.subspacecond_stats`
        (SylvStats), the estimator's solves among them."""
        return self._subspacecond("subspacecond", P, m, want_x, "R", 1, False, info_out)

    def subspacecond_dev(self, T, m, want_x=False, lr="R", schurindex=1, info_out=None):
        """`subspacecond` on a GPU tensor T [p, n, n] (only read); with want_x X is a GPU tensor [p, m, k]."""
        return self._subspacecond("subspacecond_dev", T, m, want_x, lr, schurindex, True, info_out)

    def syl_update(self, ps, m, X, tile, d, trans=False, from_t12=False):
        """Test plumbing (psd_?_syl_update, include/psd_mi355x.h): ONE launch of the update kernel of the walk of
        `psylvester`, at the tile width `tile` (2 ... 128, whatever the engine's own) on anti-diagonal `d` of the
        partition of `ps` split at m.  `X`: p matrices m x k (not written), every entry meaningful.  Returns (Y, geom):
        the p matrices after the launch and a dict with nI, nJ, nsb, ndtiles and the boundaries rb (rows of T11) and cb
        (local columns of T22).  `d` outside 1 ... nI + nJ - 2: ValueError (argument 11), nothing is launched."""
        name = "syl_update"
        fam, n, p, T, orient, si, m, keep = self._sylv_inputs(name, ps, m, "R", 1, False)
        if not 0 < m < n:
            raise ValueError(f"{name}: a split 0 < m < n (m = 0 or n has no update)")
        X = list(X)
        if len(X) != p or any(np.shape(x) != (m, n - m) for x in X):
            raise DimensionMismatch(f"{name}: X is p matrices m x k")
        if fam is _D and any(np.iscomplexobj(x) for x in X):
            raise TypeError(f"{name}: complex X for a Float64 form")
        bufs = [np.array(x, dtype=fam.dtype, order="F") for x in X]
        geom, info = SylGeom(), _ct.c_int(0)
        bounds = np.zeros(n + 2, dtype=np.int32)
        fn = getattr(self.lib, f"psd_{fam.tag}_syl_update")
        fn(self.ctx, n, p, T, orient.encode(), si, m, self._ptrs(bufs), int(tile), int(d), int(bool(trans)),
           int(bool(from_t12)), _ct.byref(geom), bounds.ctypes.data_as(_ct.POINTER(_ct.c_int32)), _ct.byref(info))
        self._raise(info.value)
        g = geom.asdict()
        g["rb"] = [int(b) for b in bounds[:g["nI"] + 1]]
        g["cb"] = [int(b) for b in bounds[g["nI"] + 1:g["nI"] + g["nJ"] + 2]]
        return bufs, g

    def eigvecs_batch(self, problems, *args, shifted=True, lr="R", schurindex=1, side="R"):
        """eigvecs(ps, select; shifted) by periodic back-substitution for MANY small decompositions of one shape in ONE
        call (psd_d_eigvecs_batch): the follow-up of pschur_batch.  Float64, all-true signature.  Per problem the result
        contract is that of `_eigvecs_backsub`; a problem's vectors do not depend on its place in the batch.

        eigvecs_batch(problems, select, shifted=True): `problems` a list of PeriodicSchur of equal order, period,
        orientation and schurindex; returns a list of what eigvecs(ps, select, method="backsub") returns for each.
        eigvecs_batch(T, Z, values, select, lr=..., schurindex=..., shifted=True): the torch outputs of the
        device-resident pschur_batch_ ([nb, p, n, n] tensors, values [nb, n]); returns (V, nvec) with V a complex128
        device tensor viewed as [nb, nmat, n, maxvec] (nmat = p if shifted else 1, maxvec = max(nvec); the columns of
        problem q at and beyond nvec[q] are zero) and nvec an int array [nb].

        `select`: [nb][n] flags, or one [n] row used for every problem; completed to conjugate pairs per problem.  A
        problem whose row is all false costs nothing and gets no columns: that is how to skip the problems whose
        pschur_batch info was non-zero.  The stats of the call are left in `self.eigvecs_batch_stats` (BevecStats), the
        per-problem counters (perturbed pivots, rescaled columns, zero eigenvalues) in `self.eigvecs_batch_counts`
        ([nb, 3]).

        `side`: "R" the right eigenvectors (A_l v_l = mu v_{l+1} for lr "L", A_l v_{l+1} = mu v_l for lr "R"); "L" the
        left eigenvectors W in the same shapes (psd_d_leigvecs_batch: w_{l+1}' A_l = mu w_l' for lr "L",
        w_l' A_l = mu w_{l+1}' for lr "R", with the same root mu and the same contract otherwise; column j of W belongs
        to the eigenvalue of column j of V, and w_l' v_l does not depend on l); "B" both: (V, W) for the list form,
        (V, W, nvec) for the device form, the stats and counters those of the left call."""
        wrong = NotImplementedPSD("eigvecs_batch: Float64 only (ComplexF64 problems: zeigvecs_batch)")
        return self._eigvecs_batch(_D, "eigvecs_batch", wrong, problems, args, shifted, lr, schurindex, side)

    def zeigvecs_batch(self, problems, *args, shifted=True, lr="R", schurindex=1, side="R"):
        """eigvecs(ps, select; shifted) by periodic back-substitution for MANY small ComplexF64 decompositions of one
        shape in ONE call (psd_z_eigvecs_batch): the follow-up of zpschur_batch, the complex counterpart of
        eigvecs_batch.  All-true signature.  Per problem the result contract is that of `_eigvecs_backsub`; a problem's
        vectors do not depend on its place in the batch.

        zeigvecs_batch(problems, select, shifted=True): `problems` a list of complex PeriodicSchur (or
        GeneralizedPeriodicSchur with S all true) of equal order, period, orientation and schurindex; returns a list of
        what eigvecs(ps, select, method="backsub") returns for each.
        zeigvecs_batch(T, Z, values, select, lr=..., schurindex=..., shifted=True): the torch outputs of the
        device-resident zpschur_batch_ ([nb, p, n, n] complex128 tensors, values [nb, n]); returns (V, nvec) shaped as
        eigvecs_batch returns them.

        `select`: [nb][n] flags, or one [n] row used for every problem, used as given.  A problem whose row is all false
        costs nothing and gets no columns.  Stats and counters are left in `self.eigvecs_batch_stats` and
        `self.eigvecs_batch_counts`, as by eigvecs_batch.  `side`: "R", "L" (psd_z_leigvecs_batch) or "B", as for
        eigvecs_batch."""
        wrong = TypeError("zeigvecs_batch: ComplexF64 only (Float64 problems: eigvecs_batch)")
        return self._eigvecs_batch(_Z, "zeigvecs_batch", wrong, problems, args, shifted, lr, schurindex, side)

    def _geigvecs_batch(self, fam, name, wrong, problems, args, shifted, lr, schurindex, S):
        """zgeigvecs_batch / dgeigvecs_batch."""
        nmat_of = lambda p: p if shifted else 1  # noqa: E731
        if hasattr(problems, "data_ptr"):
            if len(args) != 2:
                raise TypeError(f"{name}(T, Z, select, S=..., lr=..., schurindex=...)")
            import torch

            T, Z, select = problems, args[0], args[1]
            if Z is None:
                raise ValueError("geigvecs requires Schur vectors in the PSD")
            nb, p, n = self._dev_batch(fam, name, wrong, T, Z, mixed=True)
            S = [True] * p if S is None else [bool(x) for x in S]
            if len(S) != p:
                raise DimensionMismatch("length of S must match the period")
            nmat = nmat_of(p)
            if nb == 0:
                self.eigvecs_batch_stats = BevecStats()
                self.eigvecs_batch_counts = np.zeros((0, 3), dtype=np.int32)
                return (torch.zeros((0, nmat, n, 0), dtype=torch.complex128, device=T.device),
                        np.zeros((0, p, 0), dtype=np.complex128), np.zeros(0, dtype=np.int32))
            sel = self._batch_select(select, nb, n)
            dT, dZ = _dev_blocks(T, fam, "readonly"), _dev_blocks(Z, fam, "readonly")
            call = (fam, True, nb, n, p, C.c_void_p(dT.data_ptr()), C.c_void_p(dZ.data_ptr()), S, char_lr(lr), schurindex,
                    sel, shifted)
            torch.cuda.synchronize(T.device)
            maxvec = max(self._geigvecs_batch_call(*call)[0])
            dV = torch.empty((nb, nmat, max(maxvec, 1), n), dtype=torch.complex128, device=T.device)
            if maxvec == 0:
                dV.zero_()
            torch.cuda.synchronize(T.device)
            nvec, a = self._geigvecs_batch_call(*call, C.c_void_p(dV.data_ptr()), max(maxvec, 1))
            return (dV[:, :, :maxvec, :].transpose(2, 3), np.ascontiguousarray(a[:, :maxvec, :].transpose(0, 2, 1)),
                    np.array(list(nvec), dtype=np.int32))
        if len(args) != 1:
            raise TypeError(f"{name}(problems, select, shifted=True)")
        problems = list(problems)
        nb = len(problems)
        if nb == 0:
            self.eigvecs_batch_stats = BevecStats()
            self.eigvecs_batch_counts = np.zeros((0, 3), dtype=np.int32)
            return []
        n, p, orient, si, Ts, Zs, S = self._batch_decomps(fam, name, wrong, problems, needZ=True, work=False, signed=True)
        if len(S) != p:
            raise DimensionMismatch("length of S must match the period")
        sel = self._batch_select(args[0], nb, n)
        call = (fam, False, nb, n, p, self._ptrs(Ts), self._ptrs(Zs), S, orient, si, sel, shifted)
        maxvec = max(self._geigvecs_batch_call(*call)[0])
        nmat = nmat_of(p)
        Vs = [np.zeros((n, maxvec), dtype=np.complex128, order="F") for _ in range(nb * nmat)]
        nvec, a = self._geigvecs_batch_call(*call, self._ptrs(Vs), maxvec)
        return [([np.asfortranarray(Vs[q * nmat + l][:, :nvec[q]]) for l in range(nmat)],
                 np.asfortranarray(a[q, :nvec[q], :].T)) for q in range(nb)]

    def zgeigvecs_batch(self, problems, *args, shifted=True, lr="R", schurindex=1, S=None):
        """geigvecs(P, select; shifted) for MANY small signed ComplexF64 decompositions of one shape and ONE signature in
        ONE call (psd_z_geigvecs_batch): the follow-up of zgpschur_batch / gpschur_batch and zgordschur_batch_, the signed
        counterpart of zeigvecs_batch.  Per problem the result contract is that of `geigvecs` — the relations of its
        table, a_l = T_l[k, k], a zero or infinite eigenvalue a valid finite column — and a problem's vectors do not depend
        on its place in the batch.  An all-true signature runs this path too (a zero eigenvalue is no NaN column here).

        zgeigvecs_batch(problems, select, shifted=True): `problems` a list of complex GeneralizedPeriodicSchur of equal
        order, period, orientation, schurindex and S (complex PeriodicSchur count as all true); returns a list of
        (Vs, a), each what geigvecs(P, select) returns.
        zgeigvecs_batch(T, Z, select, S=..., lr=..., schurindex=..., shifted=True): the torch outputs of the
        device-resident zgpschur_batch_ / zgordschur_batch_ ([nb, p, n, n] complex128 tensors) and the signature of that
        call (None: all true); returns (V, a, nvec) with V shaped as zeigvecs_batch returns it, a a complex numpy array
        [nb, p, maxvec] (the columns of problem q at and beyond nvec[q] are zero) and nvec an int array [nb].

        `select`: [nb][n] flags, or one [n] row used for every problem, used as given.  A problem whose row is all false
        costs nothing and gets no columns.  Stats and counters (perturbed pivots, rescaled columns, columns with a zero
        or infinite eigenvalue) are left in `self.eigvecs_batch_stats` and `self.eigvecs_batch_counts`."""
        wrong = TypeError("zgeigvecs_batch: ComplexF64 only (use geigvecs per problem for a Float64 decomposition)")
        return self._geigvecs_batch(_Z, "zgeigvecs_batch", wrong, problems, args, shifted, lr, schurindex, S)

    def dgeigvecs_batch(self, problems, *args, shifted=True, lr="R", schurindex=1, S=None):
        """geigvecs(P, select; shifted) for MANY small signed Float64 decompositions of one shape and ONE signature in
        ONE call (psd_d_geigvecs_batch): the follow-up of dgpschur_batch / gpschur_batch(..., real=True) and
        dgordschur_batch_, the real counterpart of zgeigvecs_batch.  T and Z stay real: the quasi-triangular factor keeps
        its 2x2 blocks, a conjugate pair gives two columns (the partner and its scalars the exact conjugates).  Per
        problem the result contract is that of `geigvecs` — a_l = T_l[k, k] on a 1x1 row, sqrt|det B_l| on a pair (times
        e^(+-i arg lambda) at schurindex), a zero or infinite eigenvalue a valid finite column — and a problem's vectors
        and scalars do not depend on its place in the batch.  An all-true signature runs this path too.

        dgeigvecs_batch(problems, select, shifted=True): `problems` a list of real GeneralizedPeriodicSchur of equal
        order, period, orientation, schurindex and S (real PeriodicSchur count as all true); returns a list of (Vs, a),
        each what geigvecs(P, select) returns.
        dgeigvecs_batch(T, Z, select, S=..., lr=..., schurindex=..., shifted=True): the torch outputs of the
        device-resident dgpschur_batch_ / dgordschur_batch_ ([nb, p, n, n] float64 tensors) and the signature of that
        call (None: all true); returns (V, a, nvec) shaped as zgeigvecs_batch returns them (V complex128
        [nb, nmat, n, maxvec], a [nb, p, maxvec]); nvec counts completed pairs.

        `select`: [nb][n] flags, or one [n] row used for every problem, completed to whole conjugate pairs per problem.
        A problem whose row is all false costs nothing and gets no columns.  Stats and counters (perturbed pivots,
        rescaled columns, columns with a zero or infinite eigenvalue) are left in `self.eigvecs_batch_stats` and
        `self.eigvecs_batch_counts`."""
        wrong = TypeError("dgeigvecs_batch: Float64 only (ComplexF64 problems: zgeigvecs_batch)")
        return self._geigvecs_batch(_DG, "dgeigvecs_batch", wrong, problems, args, shifted, lr, schurindex, S)


    def geigvecs(self, P, select, shifted=True):
        """Eigenvectors of a signed or singular periodic product (psd_d_geigvecs / psd_z_geigvecs): periodic
        back-substitution with homogeneous recurrences, the periodic form of xTGEVC.  P: a PeriodicSchur or a
        GeneralizedPeriodicSchur (its signature S honoured).  Returns (Vs, a): Vs a list of p (shifted) or one complex
        n x nvec matrices, a a complex p x nvec array, such that for every column, l + 1 cyclic,
            'L': A_l v_l = a_l v_{l+1} if S[l], else A_l v_{l+1} = a_l v_l;
            'R': A_l v_{l+1} = a_l v_l if S[l], else A_l v_l = a_l v_{l+1}.
        a_l = T_l[k, k] at the eigenvalue's own row k (a zero a_l: a zero or infinite eigenvalue, still a valid vector);
        a conjugate pair of a real decomposition takes sqrt|det B_l|, times e^(i arg lambda_k) at schurindex.  select is
        completed to whole pairs; the normalisation is that of eigvecs(method="backsub").  The counters go to
        self.eigvecs_stats (nzero: columns with a zero or infinite eigenvalue)."""
        if isinstance(P, PartialPeriodicSchur):
            raise TypeError("geigvecs: a PartialPeriodicSchur is not supported")
        if len(P.Z) == 0 or P.Z[0].shape[0] == 0:
            raise ValueError("geigvecs requires Schur vectors in the PSD")
        n, m = P.Z[0].shape
        if len(select) != m:
            raise ValueError("length of `select` must correspond to rank of Schur (sub-)space")
        p = len(P.Ts)
        S = P.S if isinstance(P, GeneralizedPeriodicSchur) else None
        if S is not None and len(S) != p:
            raise DimensionMismatch("length of S must match the period")
        cplx = np.iscomplexobj(P.Ts[0])
        if any(np.iscomplexobj(t) != cplx for t in P.Ts) or any(np.iscomplexobj(z) != cplx for z in P.Z):
            raise TypeError("geigvecs: the factors T and the Schur vectors Z must be all real or all complex")
        dt = np.complex128 if cplx else np.float64
        Ts = [np.asfortranarray(t, dtype=dt) for t in P.Ts]  # (read only)
        Zs = [np.asfortranarray(z, dtype=dt) for z in P.Z]
        Sarr = None if S is None else (C.c_uint8 * p)(*[1 if x else 0 for x in S])
        sel = (C.c_uint8 * m)(*[1 if x else 0 for x in select])
        st = EvecStats()
        info = C.c_int(0)
        fn = self.lib.psd_z_geigvecs if cplx else self.lib.psd_d_geigvecs
        args = [self.ctx, n, p, self._ptrs(Ts), self._ptrs(Zs), Sarr, P.orientation.encode(), P.schurindex, sel, m,
                int(bool(shifted))]
        fn(*args, None, 0, None, C.byref(st), C.byref(info))  # size query: select completed, st.nvec
        self._raise(info.value)
        nvec = st.nvec
        Vs = [np.zeros((n, nvec), dtype=np.complex128, order="F") for _ in range(p if shifted else 1)]
        abuf = np.zeros(2 * p * max(nvec, 1))  # (p x nvec complex, column-major)
        fn(*args, self._ptrs(Vs), nvec, abuf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st), C.byref(info))
        self._raise(info.value)
        self.eigvecs_stats = st
        return Vs, abuf.view(np.complex128)[:p * nvec].reshape((p, nvec), order="F")

    def geigvecs_dev(self, dT, dZ, select, lr, schurindex, S=None, shifted=True):
        """Device-resident geigvecs (psd_d_geigvecs_dev / psd_z_geigvecs_dev): dT, dZ torch device tensors holding the
        [p][n][n] column-major blocks of the factors in user order (float64 or complex128), S the signature (None: all
        true).  Returns (Vs, a): (p if shifted else 1) torch device tensors n x nvec (complex128) and a complex p x nvec
        numpy array; the counters go to self.eigvecs_stats."""
        import torch

        if dZ is None:
            raise ValueError("geigvecs requires Schur vectors in the PSD")
        p, n = dT.shape[0], dT.shape[1]
        if S is not None and len(S) != p:
            raise DimensionMismatch("length of S must match the period")
        cplx = dT.is_complex()
        if dZ.dtype != dT.dtype:
            raise TypeError("geigvecs_dev: dT and dZ must have the same dtype (float64 or complex128)")
        if len(select) != n:
            raise ValueError("length of `select` must correspond to rank of Schur (sub-)space")
        Sarr = None if S is None else (C.c_uint8 * p)(*[1 if x else 0 for x in S])
        sel = (C.c_uint8 * n)(*[1 if x else 0 for x in select])
        st = EvecStats()
        info = C.c_int(0)
        fn = self.lib.psd_z_geigvecs_dev if cplx else self.lib.psd_d_geigvecs_dev
        args = [self.ctx, n, p, C.c_void_p(dT.data_ptr()), C.c_void_p(dZ.data_ptr()), Sarr, char_lr(lr).encode(),
                int(schurindex), sel, n, int(bool(shifted))]
        fn(*args, None, 0, None, C.byref(st), C.byref(info))
        self._raise(info.value)
        nvec = st.nvec
        nmat = p if shifted else 1
        dV = torch.empty((nmat, max(nvec, 1), n), dtype=torch.complex128, device=dT.device)
        abuf = np.zeros(2 * p * max(nvec, 1))
        torch.cuda.synchronize(dT.device)
        fn(*args, C.c_void_p(dV.data_ptr()), nvec, abuf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st),
           C.byref(info))
        self._raise(info.value)
        self.eigvecs_stats = st
        a = abuf.view(np.complex128)[:p * nvec].reshape((p, nvec), order="F")
        return [dV[l, :nvec, :].transpose(0, 1) for l in range(nmat)], a

    def _partial_eigvecs(self, ps0, select, shifted, method="ordschur"):
        """eigvecs(ps::PartialPeriodicSchur, select; shifted) — src/krylov.jl:996-1022: the eigenvectors of the k x k
        problem (identity Schur vectors), then Z_l times them."""
        p = ps0.period
        k = ps0.Z[0].shape[1]
        real = not np.iscomplexobj(ps0.Ts[0])
        dt = np.float64 if real else np.complex128
        small = PeriodicSchur([np.array(t, dtype=dt, order="F") for t in ps0.Ts],
                              [np.asfortranarray(np.eye(k, dtype=dt)) for _ in range(p)],
                              np.array(ps0.values, dtype=complex), ps0.orientation, ps0.schurindex)
        V0 = self.eigvecs(small, select, shifted=shifted, method=method)
        out = []
        for l, v in enumerate(V0):
            z = ps0.Z[l]
            if not isinstance(z, np.ndarray):  # device-resident Schur vectors (torch): the product stays there
                import torch

                out.append(z.to(torch.complex128) @ torch.as_tensor(v, device=z.device))
            else:
                out.append(np.asarray(z) @ v)
        return out

    @staticmethod
    def _csr_factors(As):
        """The sparse forms of partial_pschur's `As`: None when no factor is sparse, else (dev, n, p, cplx, (indptr list,
        indices list, data list)) as the CSR entry points take them — numpy arrays (host entry) or torch device tensors
        (device-resident entry), int64 / int32 / Float64 or ComplexF64."""
        if not isinstance(As, (list, tuple)) or isinstance(As, CSR):
            return None
        tor = [_is_torch_csr(a) for a in As]
        host = [None if t or isinstance(a, np.ndarray) else _host_csr(a) for a, t in zip(As, tor)]
        nsp = sum(tor) + sum(h is not None for h in host)
        if nsp == 0:
            return None
        if nsp != len(As) or (any(tor) and not all(tor)):
            raise TypeError("partial_pschur takes dense factors or sparse factors of one kind, not a mix")
        if all(tor):
            import torch

            if not all(a.is_cuda for a in As):
                raise TypeError("device-resident partial_pschur needs GPU tensors (use CSR tuples for host input)")
            n = As[0].shape[0]
            if any(a.dim() != 2 or tuple(a.shape) != (n, n) for a in As):
                raise DimensionMismatch("all As must have the same (square) size")  # krylov.jl:460-464
            cplx = any(a.is_complex() for a in As)
            vt = torch.complex128 if cplx else torch.float64
            # (column indices int32 cannot hold go to -1 / n: the structure check reports them)
            parts = ([a.crow_indices().to(torch.int64).contiguous() for a in As],
                     [a.col_indices().clamp(-1, n).to(torch.int32).contiguous() for a in As],
                     [a.values().to(vt).contiguous() for a in As])
            return True, n, len(As), cplx, parts
        n = host[0].n
        if any(h.n != n for h in host):
            raise DimensionMismatch("all As must have the same (square) size")  # krylov.jl:460-464
        cplx = any(np.iscomplexobj(h.data) for h in host)
        arrs = [_csr_arrays(h, np.complex128 if cplx else np.float64) for h in host]
        return False, n, len(As), cplx, tuple([a[i] for a in arrs] for i in range(3))

    def csr_matvec(self, A, x, group=0):
        """y = A x for one sparse factor (a host form of partial_pschur's) through the driver's own SpMV kernel, run
        once: `group` pins the lanes per row (a power of two <= 64; 0: the automatic width), so the result has the
        rounding of the driver's products."""
        h = _host_csr(A)
        if h is None:
            raise TypeError("csr_matvec needs a CSR tuple or a scipy sparse matrix")
        cplx = np.iscomplexobj(h.data) or np.iscomplexobj(x)
        dt = np.complex128 if cplx else np.float64
        indptr, ind, data = _csr_arrays(h, dt)
        xa = np.ascontiguousarray(np.asarray(x, dtype=dt).reshape(-1))
        if xa.shape[0] != h.n:
            raise DimensionMismatch("x must have length matching the matrix")
        y = np.zeros(h.n, dtype=dt)
        info = C.c_int(0)
        dp = C.POINTER(C.c_double)
        fn = self.lib.psd_z_csr_matvec if cplx else self.lib.psd_d_csr_matvec
        fn(self.ctx, h.n, indptr.ctypes.data, ind.ctypes.data, data.ctypes.data, xa.view(np.float64).ctypes.data_as(dp),
           y.view(np.float64).ctypes.data_as(dp), int(group), C.byref(info))
        if info.value in _CSR_ERRORS:
            raise ValueError(_CSR_ERRORS[info.value])
        if info.value == -8:
            raise ValueError(f"group must be 0 or a power of two <= 64, got {group}")
        self._raise(info.value)
        return y

    # ---- diagnostic entries of the dense Krylov kernels (test plumbing, include/psd_mi355x.h) ----
    def dense_matvec(self, A, x, in_place=False):
        """y = A x through the dense driver's own matvec kernels, run once.  `A`: a numpy n x n matrix (copied to the
        device), or a torch device tensor holding the matrix column-major (`A.t()` contiguous), which the kernel reads in
        place at whatever address the view has.  in_place: hand the memory of a column-major numpy array to the kernel as
        it is (meaningful only where host memory is device memory: the serial simulation).  Returns (y, geom): geom the
        launch geometry used, a dict with rp, tiles, nchunk, ccols, nblk, ldp."""
        keep = None
        if hasattr(A, "data_ptr"):
            if A.dim() != 2 or A.shape[0] != A.shape[1] or not A.t().is_contiguous() or not A.is_cuda:
                raise TypeError("dense_matvec needs a column-major square device tensor (A.t() contiguous)")
            cplx = A.is_complex()
            if A.element_size() != (16 if cplx else 8):
                raise TypeError("dense_matvec needs float64 or complex128")
            import torch

            torch.cuda.synchronize(A.device)
            n, aptr, a_dev = A.shape[0], A.data_ptr(), 1
            cplx = cplx or np.iscomplexobj(x)
            if cplx and not A.is_complex():
                raise TypeError("a complex x needs a complex A")
        else:
            A = np.asarray(A)
            n = _check_square([A])
            cplx = np.iscomplexobj(A) or np.iscomplexobj(x)
            if in_place:
                if not A.flags.f_contiguous or A.dtype != (np.complex128 if cplx else np.float64):
                    raise TypeError("in_place needs a column-major array of the element type")
                keep = A
            else:
                keep = np.asfortranarray(A, dtype=np.complex128 if cplx else np.float64)
            aptr, a_dev = keep.ctypes.data, 1 if in_place else 0
        dt = np.complex128 if cplx else np.float64
        xa = np.ascontiguousarray(np.asarray(x, dtype=dt).reshape(-1))
        if xa.shape[0] != n:
            raise DimensionMismatch("x must have length matching the matrix")
        y = np.zeros(n, dtype=dt)
        geom, info = KrylovGeom(), C.c_int(0)
        dp = C.POINTER(C.c_double)
        fn = self.lib.psd_z_dense_matvec if cplx else self.lib.psd_d_dense_matvec
        fn(self.ctx, n, C.c_void_p(aptr), a_dev, xa.view(np.float64).ctypes.data_as(dp),
           y.view(np.float64).ctypes.data_as(dp), C.byref(geom), C.byref(info))
        self._raise(info.value)
        return y, geom.asdict()

    def kr_orth(self, U, v, unew=None):
        """One orthogonalisation stage of the dense driver: v against the orthonormal columns of U (n x ncols).  Returns
        (h, hjj, unew, state, U_after): the coefficients, the norm, column ncols of the basis after the stage (`unew` on
        entry: what the column holds before, zeros by default), state = dict(stop, kind, reorth, nblk), and the first
        ncols columns as the stage left them."""
        U = np.asarray(U)
        v = np.asarray(v).reshape(-1)
        n, ncols = v.shape[0], (U.shape[1] if U.ndim == 2 else 0)
        if ncols and U.shape[0] != n:
            raise DimensionMismatch("U must have as many rows as v has elements")
        cplx = np.iscomplexobj(U) or np.iscomplexobj(v)
        dt = np.complex128 if cplx else np.float64
        Ua = np.array(U.reshape(n, ncols), dtype=dt, order="F")
        va = np.ascontiguousarray(v, dtype=dt)
        un = np.zeros(n, dtype=dt) if unew is None else np.array(np.asarray(unew).reshape(-1), dtype=dt)
        if un.shape[0] != n:
            raise DimensionMismatch("unew must have as many elements as v")
        h = np.zeros(ncols, dtype=dt)
        hjj, info = C.c_double(0.0), C.c_int(0)
        st = (C.c_int32 * 4)()
        dp = C.POINTER(C.c_double)

        def ptr(a):
            return a.ctypes.data_as(dp) if a.size else None

        fn = self.lib.psd_z_kr_orth if cplx else self.lib.psd_d_kr_orth
        fn(self.ctx, n, ncols, ptr(Ua), ptr(va), ptr(h), C.byref(hjj), ptr(un), st, C.byref(info))
        self._raise(info.value)
        state = dict(stop=int(st[0]), kind=int(st[1]), reorth=int(st[2]), nblk=int(st[3]))
        return h, float(hjj.value), un, state, Ua

    def kr_basis(self, V, Q, a0):
        """The dense driver's in-place basis update V_l[:, a0:a0+m) <- V_l[:, a0:a0+m) Q_l.  V: p matrices n x ncols,
        Q: p matrices m x m.  Returns (list of the updated matrices, R): R the rows per workgroup the launch chose."""
        p = len(V)
        if p < 1 or len(Q) != p:
            raise DimensionMismatch("V and Q must hold the same number (>= 1) of matrices")
        cplx = any(np.iscomplexobj(a) for a in list(V) + list(Q))
        dt = np.complex128 if cplx else np.float64
        n, cols = np.asarray(V[0]).shape
        m = np.asarray(Q[0]).shape[0]
        if any(np.asarray(a).shape != (n, cols) for a in V) or any(np.asarray(q).shape != (m, m) for q in Q):
            raise DimensionMismatch("all V_l must be n x ncols and all Q_l m x m")
        Va = np.stack([np.asarray(a, dtype=dt).T for a in V]).copy()  # [p][cols][n]: block l column-major n x cols
        Qa = np.stack([np.asarray(q, dtype=dt).T for q in Q]).copy()
        R, info = C.c_int32(0), C.c_int(0)
        dp = C.POINTER(C.c_double)
        fn = self.lib.psd_z_kr_basis if cplx else self.lib.psd_d_kr_basis
        fn(self.ctx, n, p, cols, int(a0), m, Va.view(np.float64).ctypes.data_as(dp),
           Qa.view(np.float64).ctypes.data_as(dp), C.byref(R), C.byref(info))
        self._raise(info.value)
        return [np.asfortranarray(Va[l].T) for l in range(p)], int(R.value)

    def diag_scalar(self, op_name, X):
        """The scalar device routine `op_name` (a key of DIAG_SCALAR_OPS) on every row of X, one lane per row, in one
        launch (test plumbing, include/psd_mi355x.h).  X: ncases x k operands, k <= 8 in the slot order of
        psd_diag_scalar_op.  Returns the ncases x 8 output rows."""
        if op_name not in DIAG_SCALAR_OPS:
            raise ValueError(f"unknown op {op_name!r}: one of " + ", ".join(DIAG_SCALAR_OPS))
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] > 8:
            raise DimensionMismatch("X must be ncases x k with ncases >= 1 and k <= 8")
        xin = np.zeros((X.shape[0], 8))
        xin[:, :X.shape[1]] = X
        out = np.full((X.shape[0], 8), np.nan)
        info = C.c_int(0)
        dp = C.POINTER(C.c_double)
        self.lib.psd_diag_scalar(self.ctx, DIAG_SCALAR_OPS[op_name], X.shape[0], xin.ctypes.data_as(dp),
                                 out.ctypes.data_as(dp), C.byref(info))
        self._raise(info.value)
        return out

    def partial_pschur(self, As, nev=None, which="LM", *, mindim=None, maxdim=None, u1=None, tol=None, tol1=None,
                       restarts=100, purgebuffer=2, seed=0):
        """partial_pschur(As, nev, which; mindim, maxdim, u1, tol, tol1, restarts, purgebuffer) — src/krylov.jl:446-487,
        for dense or sparse factors on the device.  `As`: a list of p numpy n x n matrices (host entry) or of torch device
        tensors / one torch [p, n, n] device tensor (device-resident entry: the Schur vectors come back as torch tensors
        on the same device); or a list of p sparse factors, all `CSR` tuples / scipy sparse matrices (host entry) or all
        torch sparse-CSR device tensors (device-resident entry).  Dense and sparse factors do not mix.  `which`: "LM", "LR", "SR", "LI" or "SI".  `seed` replaces the reference's `vrand!`: without `u1`
        the start vector comes from a counter-based generator seeded by it.  Returns (PartialPeriodicSchur, History);
        the counters of the call are in `P.stats` (KrylovStats)."""
        if which not in KRYLOV_TARGETS:
            raise ValueError(f"unknown target {which!r}: one of LM, LR, SR, LI, SI")
        sparse = self._csr_factors(As)
        dev = not (isinstance(As, (list, tuple)) and all(isinstance(a, np.ndarray) for a in As))
        if sparse:
            dev, n, p, cplx, csr = sparse
        elif dev:
            import torch

            dA = As if isinstance(As, torch.Tensor) else torch.stack(list(As))
            if dA.dim() != 3 or dA.shape[1] != dA.shape[2]:
                raise DimensionMismatch("all As must have the same (square) size")
            if not dA.is_cuda:
                raise TypeError("device-resident partial_pschur needs GPU tensors (use numpy arrays for host input)")
            cplx = dA.is_complex()
            # factor-major [p][n][n] blocks of column-major matrices: the transpose of each factor, contiguous
            dA = dA.to(torch.complex128 if cplx else torch.float64).transpose(1, 2).contiguous()
            p, n = dA.shape[0], dA.shape[1]
        else:
            n = _check_square(As)
            p = len(As)
            cplx = self._is_complex(As)
        if p < 1:
            raise DimensionMismatch("empty sequence")
        dt = np.complex128 if cplx else np.float64
        if nev is None:
            nev = min(6, n)
        if mindim is None:
            mindim = min(max(10, nev), n)
        if maxdim is None:
            maxdim = min(max(20, 2 * nev), n)
        if tol is None:
            tol = float(np.sqrt(np.finfo(np.float64).eps))
        if tol1 is None:
            tol1 = 100 * float(np.finfo(np.float64).eps)
        if nev < 1:
            raise ValueError("nev cannot be less than 1")  # krylov.jl:462
        if not (nev <= mindim <= maxdim <= p * n):
            raise ValueError(f"nev ≤ mindim ≤ maxdim does not hold, got {nev} ≤ {mindim} ≤ {maxdim}")  # :465-466
        uarr = None
        if u1 is not None:
            if hasattr(u1, "detach"):
                u1 = u1.detach().cpu().numpy()
            uarr = np.ascontiguousarray(np.asarray(u1, dtype=dt).reshape(-1))
            if uarr.shape[0] != n:
                raise ValueError("u1 must have length matching first matrix/operator")  # krylov.jl:538-540
        kmax = maxdim
        Ts = [np.zeros(kmax * kmax, dtype=dt) for _ in range(p)]  # (nconv x nconv, ld nconv: reshaped below)
        wr, wi = np.zeros(kmax), np.zeros(kmax)
        nconv, info = C.c_int(0), C.c_int(0)
        st = KrylovStats()
        dp = C.POINTER(C.c_double)
        up = uarr.view(np.float64).ctypes.data_as(dp) if uarr is not None else None
        common = (int(nev), KRYLOV_TARGETS[which].encode(), int(mindim), int(maxdim), up, int(seed) & (2 ** 64 - 1),
                  float(tol), float(tol1), int(restarts), int(purgebuffer), C.byref(nconv), self._ptrs(Ts))
        if sparse:
            sfx = "_csr_dev" if dev else "_csr"
            fn = getattr(self.lib, ("psd_z_partial_pschur" if cplx else "psd_d_partial_pschur") + sfx)
            if dev:
                import torch

                vals = csr[2]
                dZ = torch.zeros((p, kmax, n), dtype=vals[0].dtype, device=vals[0].device)
                torch.cuda.synchronize(vals[0].device)
                ptrs = [(C.c_void_p * p)(*[t.data_ptr() for t in part]) for part in csr]
                zarg = C.c_void_p(dZ.data_ptr())
            else:
                Zs = [np.zeros((n, kmax), dtype=dt, order="F") for _ in range(p)]
                ptrs = [self._ptrs(part) for part in csr]
                zarg = self._ptrs(Zs)
            fn(self.ctx, n, p, *ptrs, *common, zarg, wr.ctypes.data_as(dp), wi.ctypes.data_as(dp), C.byref(st),
               C.byref(info))
            if info.value in _CSR_ERRORS:
                raise ValueError(_CSR_ERRORS[info.value])
        elif dev:
            import torch

            dZ = torch.zeros((p, kmax, n), dtype=dA.dtype, device=dA.device)  # block l: n x kmax column-major
            fn = self.lib.psd_z_partial_pschur_dev if cplx else self.lib.psd_d_partial_pschur_dev
            torch.cuda.synchronize(dA.device)
            fn(self.ctx, n, p, C.c_void_p(dA.data_ptr()), *common, C.c_void_p(dZ.data_ptr()), wr.ctypes.data_as(dp),
               wi.ctypes.data_as(dp), C.byref(st), C.byref(info))
        else:
            Aw = [np.asfortranarray(a, dtype=dt) for a in As]
            Zs = [np.zeros((n, kmax), dtype=dt, order="F") for _ in range(p)]
            fn = self.lib.psd_z_partial_pschur if cplx else self.lib.psd_d_partial_pschur
            fn(self.ctx, n, p, self._ptrs(Aw), *common, self._ptrs(Zs), wr.ctypes.data_as(dp), wi.ctypes.data_as(dp),
               C.byref(st), C.byref(info))
        iv = info.value
        if iv == 5000:
            raise PKSFailure("Arnoldi reinitialization failed")
        if 2000 <= iv < 3000:
            raise IllConditionedException(iv - 2000)
        self._raise(iv)
        k = nconv.value
        Tk = [np.asfortranarray(t[: k * k].reshape(k, k, order="F")) for t in Ts]
        if dev:
            Zk = [dZ[l, :k, :].transpose(0, 1) for l in range(p)]
        else:
            Zk = [np.asfortranarray(z[:, :k]) for z in Zs]
        lam = (wr + 1j * wi)[:k]
        P = PartialPeriodicSchur(Tk, Zk, lam, st)
        return P, History(int(st.nprods), int(st.nconverged), bool(st.converged), int(st.nev))

    def checkpsd(self, P, As, thresh=100, strict=True, S=None, details=False):
        """checkpsd(P, As; thresh, strict) — src/diagnostics.jl:190-263 — evaluated on the device (matrix cores).
        Returns (ok, err) like the reference; with details=True also the orthogonality and triangularity norms."""
        p = len(As)
        if P.period != p:
            raise DimensionMismatch("length of Hs vector must match period of P")  # diagnostics.jl:194-196
        n = P.Ts[0].shape[0]
        for a in As:
            if a.ndim != 2 or a.shape[0] != n or a.shape[1] != n:
                raise DimensionMismatch("size of Hs matrices must match P")  # diagnostics.jl:197-202
        if S is None and isinstance(P, GeneralizedPeriodicSchur):
            S = P.S
        cplx = self._is_complex(P.Ts) or self._is_complex(As) or self._is_complex(P.Z)
        dt = np.complex128 if cplx else np.float64
        Tw = [np.asfortranarray(t, dtype=dt) for t in P.Ts]
        Zw = [np.asfortranarray(z, dtype=dt) for z in P.Z]
        Aw = [np.asfortranarray(a, dtype=dt) for a in As]
        sig = (C.c_uint8 * p)(*[1 if x else 0 for x in S]) if S is not None else None
        err, orth, tri = np.zeros(p), np.zeros(p), np.zeros(p)
        ok, info = C.c_int(0), C.c_int(0)
        dp = C.POINTER(C.c_double)
        if cplx:
            self.lib.psd_z_checkpsd(self.ctx, n, p, self._ptrs(Tw), self._ptrs(Zw), self._ptrs(Aw), sig,
                                    P.orientation.encode(), P.schurindex, float(thresh), int(strict),
                                    err.ctypes.data_as(dp), orth.ctypes.data_as(dp), tri.ctypes.data_as(dp),
                                    C.byref(ok), C.byref(info))
        else:
            wi = np.ascontiguousarray(np.asarray(P.values).imag, dtype=np.float64)
            self.lib.psd_d_checkpsd(self.ctx, n, p, self._ptrs(Tw), self._ptrs(Zw), self._ptrs(Aw), sig,
                                    P.orientation.encode(), P.schurindex, wi.ctypes.data_as(dp), float(thresh),
                                    int(strict), err.ctypes.data_as(dp), orth.ctypes.data_as(dp),
                                    tri.ctypes.data_as(dp), C.byref(ok), C.byref(info))
        self._raise(info.value)
        if details:
            return bool(ok.value), err, orth, tri
        return bool(ok.value), err

    def checkpsd_dev(self, dT_ptr, dZ_ptr, dA_ptr, n, p, lr="R", schurindex=1, thresh=100, strict=True, S=None,
                     cplx=False):
        """checkpsd on operands already resident in HBM ([p][n][n] Float64 blocks in user order; `cplx`: ComplexF64
        blocks of interleaved (re, im) doubles, psd_z_checkpsd_dev)."""
        sig = (C.c_uint8 * p)(*[1 if x else 0 for x in S]) if S is not None else None
        err, orth, tri = np.zeros(p), np.zeros(p), np.zeros(p)
        ok, info = C.c_int(0), C.c_int(0)
        dp = C.POINTER(C.c_double)
        entry = self.lib.psd_z_checkpsd_dev if cplx else self.lib.psd_d_checkpsd_dev
        entry(self.ctx, n, p, C.c_void_p(dT_ptr), C.c_void_p(dZ_ptr), C.c_void_p(dA_ptr), sig, char_lr(lr).encode(),
              schurindex, float(thresh), int(strict), err.ctypes.data_as(dp), orth.ctypes.data_as(dp),
              tri.ctypes.data_as(dp), C.byref(ok), C.byref(info))
        self._raise(info.value)
        return bool(ok.value), err, orth, tri

    def _checkpsd_batch_call(self, cplx, dev, nb, n, p, T, Z, A, S, orient, si, thresh, strict, details):
        """psd_?_checkpsd_batch[_dev] on packed factors (flat pointer lists, or with `dev` device blocks); the stats of
        the call are left in `self.checkpsd_batch_stats`."""
        if S is not None and len(S) != p:
            raise DimensionMismatch("length of S must match the period")
        sig = (C.c_uint8 * p)(*[1 if x else 0 for x in S]) if S is not None else None
        err, orth, tri = np.zeros((nb, p)), np.zeros((nb, p)), np.zeros((nb, p))
        ok = np.zeros(nb, dtype=np.int32)
        st, info = BcheckStats(), C.c_int(0)
        dp = C.POINTER(C.c_double)
        entry = getattr(self.lib, f"psd_{'z' if cplx else 'd'}_checkpsd_batch{'_dev' if dev else ''}")
        entry(self.ctx, nb, n, p, T, Z, A, sig, orient.encode(), si, float(thresh), int(strict), err.ctypes.data_as(dp),
              orth.ctypes.data_as(dp), tri.ctypes.data_as(dp), ok.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st),
              C.byref(info))
        self.checkpsd_batch_stats = st
        self._raise(info.value)
        return (ok != 0, err, orth, tri) if details else (ok != 0, err)

    def checkpsd_batch(self, Ps, *args, thresh=100, strict=True, S=None, details=False, lr="R", schurindex=1):
        """checkpsd(P, As; thresh, strict) — src/diagnostics.jl:190-263 — for MANY small decompositions of one shape in
        ONE call (psd_?_checkpsd_batch): the follow-up of every *pschur_batch / *ordschur_batch.  Real or complex
        follows the data; the signature is an argument, so the one method serves all four batch families.

        checkpsd_batch(Ps, As_list, thresh=100, strict=True, S=None, details=False): `Ps` a list of PeriodicSchur /
        GeneralizedPeriodicSchur of equal order, period, orientation, schurindex and signature (`S`: None takes that of
        the decompositions), `As_list` the factors each was computed from.
        checkpsd_batch(T, Z, A, lr=..., schurindex=..., S=...): three GPU tensors [nb, p, n, n] of one dtype (float64 or
        complex128), the outputs of a device-resident *pschur_batch_ and the factors it started from; they are only
        read, and tensors in the layout those entries return are not copied.

        Returns (ok, err): ok a bool array [nb] (the reference's verdict per problem), err [nb, p]; with details=True
        also orth and tri [nb, p].  Up to order 64 a problem's numbers do not depend on its place in the batch (bit for
        bit).  The stats of the call are left in `self.checkpsd_batch_stats` (BcheckStats)."""
        if hasattr(Ps, "data_ptr"):
            if len(args) != 2:
                raise TypeError("checkpsd_batch(T, Z, A, lr=..., schurindex=..., S=...)")
            import torch

            T, Z, A = Ps, args[0], args[1]
            if any(x.dtype not in (torch.float64, torch.complex128) for x in (T, Z, A)):
                raise TypeError("checkpsd_batch: float64 or complex128 tensors")
            fam = _Z if T.is_complex() else _D
            wrong = TypeError("checkpsd_batch: the tensors T, Z and A must be of one dtype")
            nb, p, n = self._dev_batch(fam, "checkpsd_batch", wrong, T, Z, A)
            if nb == 0:
                self.checkpsd_batch_stats = BcheckStats()
                empty = (np.zeros(0, dtype=bool),) + (np.zeros((0, p)),) * 3
                return empty if details else empty[:2]
            dT, dZ, dA = (_dev_blocks(x, fam, "readonly") for x in (T, Z, A))
            torch.cuda.synchronize(T.device)
            return self._checkpsd_batch_call(fam is _Z, True, nb, n, p, C.c_void_p(dT.data_ptr()),
                                             C.c_void_p(dZ.data_ptr()), C.c_void_p(dA.data_ptr()), S, char_lr(lr),
                                             schurindex, thresh, strict, details)
        if len(args) != 1:
            raise TypeError("checkpsd_batch(Ps, As_list, thresh=100, strict=True)")
        Ps, As_list = list(Ps), [list(As) for As in args[0]]
        nb = len(Ps)
        if len(As_list) != nb:
            raise DimensionMismatch("checkpsd_batch: one list of factors per decomposition")
        if nb == 0:
            self.checkpsd_batch_stats = BcheckStats()
            empty = (np.zeros(0, dtype=bool),) + (np.zeros((0, 0)),) * 3
            return empty if details else empty[:2]
        shape = kind = sig0 = None
        Tw, Zw, Aw = [], [], []
        for P, As in zip(Ps, As_list):
            p = len(As)
            if P.period != p:
                raise DimensionMismatch("length of Hs vector must match period of P")  # diagnostics.jl:194-196
            n = P.Ts[0].shape[0]
            if any(np.ndim(a) != 2 or a.shape != (n, n) for a in As):
                raise DimensionMismatch("size of Hs matrices must match P")  # diagnostics.jl:197-202
            if shape is None:
                shape, orient, si = (n, p), P.orientation, P.schurindex
            if (n, p) != shape:
                raise DimensionMismatch("the problems of a batch must have equal order and period")
            if (P.orientation, P.schurindex) != (orient, si) or len(P.Z) != p:
                raise DimensionMismatch("the problems of a batch must have equal order, period, orientation and schurindex")
            sig = [bool(x) for x in getattr(P, "S", [True] * p)]
            sig0 = sig if sig0 is None else sig0
            if sig != sig0:
                raise DimensionMismatch("the problems of a batch must have equal signatures S")
            cplx = self._is_complex(P.Ts) or self._is_complex(As) or self._is_complex(P.Z)
            kind = cplx if kind is None else kind
            if cplx != kind:
                raise TypeError("checkpsd_batch: the problems of a batch must be all real or all complex")
            Tw += list(P.Ts)
            Zw += list(P.Z)
            Aw += As
        dt = np.complex128 if kind else np.float64
        Tw, Zw, Aw = ([np.asfortranarray(x, dtype=dt) for x in M] for M in (Tw, Zw, Aw))
        n, p = shape
        return self._checkpsd_batch_call(kind, False, nb, n, p, self._ptrs(Tw), self._ptrs(Zw), self._ptrs(Aw),
                                         sig0 if S is None else S, orient, si, thresh, strict, details)

    def pschur_dev(self, dA_ptr, n, p, lr="R", dZ_ptr=None, wantT=True, maxitfac=30):
        """Device-resident pschur!: dA_ptr / dZ_ptr are device addresses of [p][n][n] column-major blocks."""
        orient = char_lr(lr)
        wantZ = dZ_ptr is not None
        wr = np.zeros(n)
        wi = np.zeros(n)
        si = C.c_int(0)
        st = Stats()
        maxlog = 2 * maxitfac * n + n + 16
        log = np.zeros(3 * maxlog, dtype=np.int32)
        info = C.c_int(0)
        dp = C.POINTER(C.c_double)
        self.lib.psd_d_pschur_dev(self.ctx, n, p, C.c_void_p(dA_ptr), orient.encode(), int(wantT), int(wantZ),
                                  int(maxitfac), C.c_void_p(dZ_ptr) if wantZ else None, wr.ctypes.data_as(dp),
                                  wi.ctypes.data_as(dp), C.byref(si), C.byref(st),
                                  log.ctypes.data_as(C.POINTER(C.c_int32)), maxlog, C.byref(info))
        self._raise(info.value)
        nl = min(st.nlog, maxlog)
        return wr + 1j * wi, si.value, st, log[: 3 * nl].reshape(-1, 3).copy()


    def zpschur_dev(self, dA_ptr, n, p, lr="R", dZ_ptr=None, wantT=True, maxitfac=30):
        """Device-resident pschur! for ComplexF64 (psd_z_pschur_dev): dA_ptr / dZ_ptr are device addresses of [p][n][n]
        column-major blocks of interleaved (re, im) doubles.  Returns (values, schurindex, stats, sweep log)."""
        orient = char_lr(lr)
        wantZ = dZ_ptr is not None
        alpha = np.zeros(n, dtype=np.complex128)
        beta = np.zeros(n)
        sc = np.zeros(n, dtype=np.int32)
        si = C.c_int(0)
        st = Stats()
        maxlog = 2 * maxitfac * n + n + 16
        log = np.zeros(3 * maxlog, dtype=np.int32)
        info = C.c_int(0)
        dp = C.POINTER(C.c_double)
        i32p = C.POINTER(C.c_int32)
        self.lib.psd_z_pschur_dev(self.ctx, n, p, C.c_void_p(dA_ptr), orient.encode(), int(wantT), int(wantZ),
                                  int(maxitfac), C.c_void_p(dZ_ptr) if wantZ else None, alpha.ctypes.data_as(dp),
                                  beta.ctypes.data_as(dp), sc.ctypes.data_as(i32p), C.byref(si), C.byref(st),
                                  log.ctypes.data_as(i32p), maxlog, C.byref(info))
        self._raise(info.value)
        lam = _scaled_values(alpha, beta, sc)
        nl = min(st.nlog, maxlog)
        return lam, si.value, st, log[: 3 * nl].reshape(-1, 3).copy()


_default_engine = None


def default_engine():
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine()
    return _default_engine


def pschur(A, lr="R", **kw):
    return default_engine().pschur(A, lr, **kw)


def pschur_(A, lr="R", **kw):
    return default_engine().pschur_(A, lr, **kw)


def phessenberg_(A):
    return default_engine().phessenberg_(A)


def partial_pschur(As, nev=None, which="LM", **kw):
    return default_engine().partial_pschur(As, nev, which, **kw)
