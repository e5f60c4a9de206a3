"""The engine's scalar device routines one call at a time (psd_diag_scalar), against exact rational arithmetic: tables,
exact references, float64 restatements of the reference's formulas (which set the gates) and the checks, shared by the
simulated and the GPU tier.

Reference.  Every input is a double, hence a rational: the exact outputs are computed with fractions.Fraction, plus one
square root per routine taken with `decimal` at 120 digits (relative error 1e-119, nothing beside an ulp of 1.1e-16).

Error measure.  Real outputs: |computed - exact| in ulps of the double nearest the exact value (math.ulp), in units of
2^-1074 where the exact value is below DBL_MIN.  Complex outputs (sn and r of the complex rotation, tau and mult of the
complex reflector scalars): the modulus of the difference in ulps of the larger component of the exact value; a complex
product is accurate only normwise (its real part a b - c d can cancel), so a componentwise ulp count is unbounded for the
reference's own formula as well.  Outputs with a conventional value (tau = 0 exits, cs = 1, sn = 0, r = f, the integer of
psd_c3_expo) are compared bit for bit, the sign of a zero included.

Gate.  For each op the file restates the REFERENCE's formula in plain float64 (householder.jl:66-108 and :110-156, stdlib
givensAlgorithm for Float64 and ComplexF64, 1.0 / x, sqrt(s), 1.0 / sqrt(s), libm's ldexp).  E_ieee is the worst error of
that restatement over the op's table; the engine's routine must stay within B = 2 E_ieee + 1 ulp on the same table: the
fast forms chain two or three rounded operations where the IEEE form chains one or two (factor 2), and an uncorrected
final Newton step may cost one rounding of its own (+ 1).  The backward properties are gated by the same rule in units of
eps = 2^-52.  Nothing in a gate comes from what the engine returns.

Domains.  The guarded routines take every finite input, zeros and subnormals included, whose exact outputs are doubles:
exponents reach up to 2^1022 (2^1021 for the complex rotation), so that no exact norm exceeds DBL_MAX, and the two larfg
forms that return mult = 1 / (alpha - beta) keep max(|alpha|, xnorm) >= DBL_MIN: below 2^-1024 the exact mult is larger
than DBL_MAX (no double holds it), and the reference's own _hypot3 overflows in 1 / w.  The three raw forms promise their
accuracy only where their callers' guards let them run; RAW_DOMAINS derives that from the call sites."""
import decimal
import math
from fractions import Fraction as Fr

import numpy as np

EPS = 2.0 ** -52
DBL_MIN = 2.0 ** -1022
DBL_MAX = float(np.finfo(np.float64).max)
TINY = 2.0 ** -1074
SAFMN2 = 2.0 ** -485  # floatmin2(Float64) = 1.0010415475915505e-146 (psd_givens, psd_zgivens)
SAFMX2 = 2.0 ** 485
SFMIN = 2.0 * DBL_MIN / EPS  # dlarfg tails of psd_reflector_small and psd_h2_larfg (2^-969)
ZSFMIN = DBL_MIN / EPS  # psd_zh2_larfg (householder.jl:116)
MAXCASES = 2000

assert SAFMN2 == 1.0010415475915505e-146 and SAFMX2 == 9.989595361011175e+145

# ---- the arguments the callers' guards admit to the raw forms -----------------------------------------------------------
# psd_sqrt_pair_fast(s):
#   psd_refl2 / psd_refl3 (psd_scalar.h): max |x_i| < 1e140 and max |tail| > 1e-140         -> s in (1e-280, 3e280)
#   psd_refl32_pair and the _lean forms: run on anything, USED only when s < 1e280 and the tail's sum > 1e-280
#   psd_givens: max(|f|, |g|) in (safmn2, safmx2)                                           -> (safmn2^2, 2 safmx2^2)
#   psd_zgivens (psd_complex.h): every component below safmx2, f2 > max(g2, 1) DBL_MIN; roots of f2 and of f2 + g2
#                                                                                           -> (DBL_MIN, 4 safmx2^2)
#   psd_h2_larfg (psd_hess2.h:163-168): max in (1e-140, 1e140)                              -> (1e-280, 2e280)
#   the pipe form's norm (psd_hess2.h:568-571, psd_zhess2.h:369-371): largest tail entry in (1e-140, 1e140), at most
#   2048 entries (complex: 4096 squares)                                                    -> (1e-280, 4.1e283)
#   psd_rord.h:144,229,502: after the ldexp normalisation the largest entry is in [0.5, 1)   -> [0.25, 8)
#   union: DBL_MIN < s < 4 safmx2^2 = 3.99e292
# psd_rcp_fast(x):
#   the reflectors and psd_h2_larfg: x = +-(|x0| + nrm), nrm in (1e-140, sqrt(3) 1e140)     -> |x| in (1e-140, 2.74e140)
#   psd_rord.h:147,231,507: nrm (nrm + |alpha|), nrm in [0.5, sqrt(8))                       -> [0.25, 16)
#   union: 1e-140 < |x| < (1 + sqrt(3)) 1e140, either sign
# psd_rsqrt2_fast(a, b): psd_zgivens_lean only, a = f2, b = f2 + g2 behind the guard of psd_zgivens
#                                                  -> DBL_MIN < a < 2 safmx2^2, a <= b < 4 safmx2^2
RAW_DOMAINS = {
    "sqrt_pair": (float(np.nextafter(DBL_MIN, 1.0)), float(np.nextafter(4.0 * SAFMX2 * SAFMX2, 0.0))),
    "rcp": (float(np.nextafter(1e-140, 1.0)), float(np.nextafter((1.0 + math.sqrt(3.0)) * 1e140, 0.0))),
    "rsqrt2_a": (float(np.nextafter(DBL_MIN, 1.0)), float(np.nextafter(2.0 * SAFMX2 * SAFMX2, 0.0))),
}

_CTX = decimal.Context(prec=120, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)


def fsqrt(q):
    """sqrt of a non-negative Fraction to 120 digits, as a Fraction."""
    if q == 0:
        return Fr(0)
    d = _CTX.divide(decimal.Decimal(q.numerator), decimal.Decimal(q.denominator))
    return Fr(_CTX.sqrt(d))


def _unit(exact_abs):
    if exact_abs < Fr(DBL_MIN):
        return Fr(TINY)
    return Fr(math.ulp(float(exact_abs)))  # (int / int is correctly rounded in Python)


def _bits(x):
    return np.float64(x).tobytes()


def err_ulps(got, exact):
    """Error of one output.  exact: a Fraction, a (re, im) pair of Fractions with got a (re, im) pair of floats, or a
    float (a conventional value: bit for bit)."""
    if isinstance(exact, float):
        return 0.0 if _bits(got) == _bits(exact) else math.inf
    if isinstance(exact, tuple):
        if isinstance(exact[0], float):
            return max(err_ulps(got[0], exact[0]), err_ulps(got[1], exact[1]))
        if not all(math.isfinite(g) for g in got):
            return math.inf
        d2 = (Fr(got[0]) - exact[0]) ** 2 + (Fr(got[1]) - exact[1]) ** 2
        u = _unit(max(abs(exact[0]), abs(exact[1])))
        return math.sqrt(_flt(d2 / (u * u)))
    if not math.isfinite(got):
        return math.inf
    return _flt(abs(Fr(float(got)) - exact) / _unit(abs(exact)))


def _sgn(x):
    return -1 if math.copysign(1.0, x) < 0 else 1


_EPS2, _TINY2 = Fr(EPS) ** 2, Fr(TINY) ** 2


def _flt(q):
    """float(q) for a Fraction, inf where it is past DBL_MAX (a wrong output can put a property anywhere)."""
    try:
        return float(q)
    except OverflowError:
        return math.inf


def _rel(num2, den2):
    """sqrt(num2) in units of eps sqrt(den2) for two non-negative Fractions — of 2^-1074 where that is larger: below it
    no double can follow (the rule of the error measure: subnormal values are counted in units of 2^-1074)."""
    if num2 == 0:
        return 0.0
    return math.sqrt(_flt(num2 / max(den2 * _EPS2, _TINY2)))


def _fin(vals):
    return all(math.isfinite(v) for v in vals)


# ---- exact references ---------------------------------------------------------------------------------------------------
def exact_refl(x):
    """(beta, v..., tau) of the reflector of x (householder.jl:66-108): beta = -copysign(||x||, x0)."""
    if all(t == 0.0 for t in x[1:]):
        return [float(v) for v in x] + [0.0]  # H = I: x untouched, tau = 0
    X = [Fr(v) for v in x]
    beta = -_sgn(x[0]) * fsqrt(sum(v * v for v in X))
    den = X[0] - beta
    return [beta] + [v / den for v in X[1:]] + [(beta - X[0]) / beta]


def exact_larfg(alpha, xnorm):
    """(tau, beta, mult) from the tail's norm."""
    if xnorm == 0.0:
        return [0.0, float(alpha), 0.0]
    a, n = Fr(alpha), Fr(xnorm)
    beta = -_sgn(alpha) * fsqrt(a * a + n * n)
    return [(beta - a) / beta, beta, 1 / (a - beta)]


def exact_zlarfg(ar, ai, xnorm):
    """(tau, beta, mult), tau and mult complex (householder.jl:110-156): tau = 0 only for a zero tail and a real alpha."""
    if xnorm == 0.0 and ai == 0.0:
        return [(0.0, 0.0), float(ar), (0.0, 0.0)]
    a, b, n = Fr(ar), Fr(ai), Fr(xnorm)
    beta = -_sgn(ar) * fsqrt(a * a + b * b + n * n)
    d = (a - beta) ** 2 + b * b
    return [((beta - a) / beta, -b / beta), beta, ((a - beta) / d, -b / d)]


def exact_givens(f, g):
    """stdlib givensAlgorithm(f::Float64, g): r > 0 unless |f| > |g|, where r takes the sign of f."""
    if g == 0.0:
        return [1.0, 0.0, float(f)]
    if f == 0.0:
        return [0.0, 1.0, float(g)]
    F, G = Fr(f), Fr(g)
    r = fsqrt(F * F + G * G)
    if abs(f) > abs(g) and f < 0:
        r = -r
    return [F / r, G / r, r]


def exact_zgivens(fr, fi, gr, gi):
    """(cs, sn, r): cs = |f| / N, sn = (f / |f|) conj(g) / N, r = (f / |f|) N, N^2 = |f|^2 + |g|^2 — with the one root
    q = |f| N: cs = |f|^2 / q, sn = f conj(g) / q, r = f N^2 / q.  f = 0: cs = 0, sn = conj(g) / |g|, r = |g|."""
    a, b, c, d = Fr(fr), Fr(fi), Fr(gr), Fr(gi)
    f2, g2 = a * a + b * b, c * c + d * d
    if g2 == 0:
        return [Fr(1), (Fr(0), Fr(0)), (a, b)]
    if f2 == 0:
        ng = fsqrt(g2)
        return [Fr(0), (c / ng, -d / ng), (ng, Fr(0))]
    n2 = f2 + g2
    q = fsqrt(f2 * n2)
    return [f2 / q, ((a * c + b * d) / q, (b * c - a * d) / q), (a * n2 / q, b * n2 / q)]


# ---- float64 restatements of the reference's formulas (they set the gates) -------------------------------------------
def _f(x):
    return np.float64(x)


def ieee_norm2(x):  # householder.jl:5-24
    if len(x) < 1:
        return _f(0.0)
    if len(x) == 1:
        return abs(x[0])
    scale, ssq = _f(0.0), _f(0.0)
    for xi in x:
        if xi != 0.0:
            a = abs(xi)
            if scale < a:
                q = scale / a
                ssq = _f(1.0) + ssq * (q * q)
                scale = a
            else:
                q = a / scale
                ssq += q * q
    return scale * np.sqrt(ssq)


def ieee_reflector(x):
    """householder.jl:66-108.  Returns ([beta, v..., tau], mult): mult the factor the tail was multiplied by in all."""
    x = [_f(v) for v in x]
    n = len(x)
    sfmin = _f(SFMIN)
    alpha = x[0]
    xnorm = ieee_norm2(x[1:])
    if xnorm == 0.0:
        return x + [_f(0.0)], _f(0.0)
    beta = -np.copysign(np.hypot(alpha, xnorm), alpha)
    kount = 0
    scl = _f(1.0)
    if abs(beta) < sfmin:
        rsfmin = _f(1.0) / sfmin
        small = True
        while small:
            kount += 1
            for j in range(1, n):
                x[j] *= rsfmin
            scl *= rsfmin
            beta *= rsfmin
            alpha *= rsfmin
            small = abs(beta) < sfmin and kount < 20
        xnorm = ieee_norm2(x[1:])
        beta = -np.copysign(np.hypot(alpha, xnorm), alpha)
    tau = (beta - alpha) / beta
    t = _f(1.0) / (alpha - beta)
    for j in range(1, n):
        x[j] *= t
    for _ in range(kount):
        beta *= sfmin
    return [beta] + x[1:] + [tau], scl * t


def ieee_larfg(alpha, xnorm):
    out, mult = ieee_reflector([alpha, xnorm])
    return [out[2], out[0], mult]


def _hypot3(x, y, z):  # householder.jl:161-169
    xa, ya, za = abs(x), abs(y), abs(z)
    w = max(xa, ya, za)
    rw = _f(1.0) / w
    a, b, c = rw * xa, rw * ya, rw * za
    return w * np.sqrt(a * a + b * b + c * c)


def ieee_zlarfg(ar, ai, xnorm):
    """householder.jl:110-156 on x = (alpha, xnorm): a one-element tail is its own norm."""
    ar, ai, xnorm = _f(ar), _f(ai), _f(xnorm)
    if xnorm == 0.0 and ai == 0.0:
        return [(0.0, 0.0), ar, (0.0, 0.0)]
    sfmin = _f(ZSFMIN)
    beta = -np.copysign(_hypot3(ar, ai, xnorm), ar)
    kount = 0
    scl = _f(1.0)
    if abs(beta) < sfmin:
        rsfmin = _f(1.0) / sfmin
        small = True
        while small:
            kount += 1
            xnorm *= rsfmin
            scl *= rsfmin
            beta *= rsfmin
            ar *= rsfmin
            ai *= rsfmin
            small = abs(beta) < sfmin and kount < 20
        beta = -np.copysign(_hypot3(ar, ai, xnorm), ar)
    tau = ((beta - ar) / beta, -ai / beta)
    t = np.complex128(1.0) / np.complex128(complex(ar - beta, ai))
    for _ in range(kount):
        beta *= sfmin
    return [tau, beta, (scl * t.real, scl * t.imag)]


def ieee_givens(f, g):
    """stdlib LinearAlgebra.givensAlgorithm(f::Float64, g::Float64) (a port of LAPACK dlartg)."""
    f, g = _f(f), _f(g)
    safmn2, safmx2 = _f(SAFMN2), _f(SAFMX2)
    if g == 0.0:
        return [_f(1.0), _f(0.0), f]
    if f == 0.0:
        return [_f(0.0), _f(1.0), g]
    f1, g1 = f, g
    scale = max(abs(f1), abs(g1))
    count = 0
    if scale >= safmx2:
        while True:
            count += 1
            f1 *= safmn2
            g1 *= safmn2
            scale = max(abs(f1), abs(g1))
            if scale < safmx2 or count >= 20:
                break
        r = np.sqrt(f1 * f1 + g1 * g1)
        cs, sn = f1 / r, g1 / r
        for _ in range(count):
            r *= safmx2
    elif scale <= safmn2:
        while True:
            count += 1
            f1 *= safmx2
            g1 *= safmx2
            scale = max(abs(f1), abs(g1))
            if scale > safmn2:
                break
        r = np.sqrt(f1 * f1 + g1 * g1)
        cs, sn = f1 / r, g1 / r
        for _ in range(count):
            r *= safmn2
    else:
        r = np.sqrt(f1 * f1 + g1 * g1)
        cs, sn = f1 / r, g1 / r
    if abs(f) > abs(g) and cs < 0.0:
        cs, sn, r = -cs, -sn, -r
    return [cs, sn, r]


def _cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def ieee_zgivens(fr, fi, gr, gi):
    """stdlib LinearAlgebra.givensAlgorithm(f::ComplexF64, g::ComplexF64) (a port of LAPACK 3.x zlartg)."""
    f, g = (_f(fr), _f(fi)), (_f(gr), _f(gi))
    safmin, safmn2, safmx2 = _f(DBL_MIN), _f(SAFMN2), _f(SAFMX2)
    scale = max(abs(f[0]), abs(f[1]), abs(g[0]), abs(g[1]))
    fs, gs = f, g
    count = 0
    if scale >= safmx2:
        while True:
            count += 1
            fs = (fs[0] * safmn2, fs[1] * safmn2)
            gs = (gs[0] * safmn2, gs[1] * safmn2)
            scale *= safmn2
            if scale < safmx2 or count >= 20:
                break
    elif scale <= safmn2:
        if g[0] == 0.0 and g[1] == 0.0:
            return [_f(1.0), (_f(0.0), _f(0.0)), f]
        while True:
            count -= 1
            fs = (fs[0] * safmx2, fs[1] * safmx2)
            gs = (gs[0] * safmx2, gs[1] * safmx2)
            scale *= safmx2
            if scale > safmn2:
                break
    f2 = fs[0] * fs[0] + fs[1] * fs[1]
    g2 = gs[0] * gs[0] + gs[1] * gs[1]
    if f2 <= max(g2, _f(1.0)) * safmin:
        if f[0] == 0.0 and f[1] == 0.0:
            d = np.hypot(gs[0], gs[1])
            return [_f(0.0), (gs[0] / d, -gs[1] / d), (np.hypot(g[0], g[1]), _f(0.0))]
        f2s = np.hypot(fs[0], fs[1])
        g2s = np.sqrt(g2)
        cs = f2s / g2s
        if max(abs(f[0]), abs(f[1])) > 1.0:
            d = np.hypot(f[0], f[1])
            ff = (f[0] / d, f[1] / d)
        else:
            dr, di = safmx2 * f[0], safmx2 * f[1]
            d = np.hypot(dr, di)
            ff = (dr / d, di / d)
        sn = _cmul(ff, (gs[0] / g2s, -gs[1] / g2s))
        t = _cmul(sn, g)
        return [cs, sn, (cs * f[0] + t[0], cs * f[1] + t[1])]
    f2s = np.sqrt(_f(1.0) + g2 / f2)
    r = (f2s * fs[0], f2s * fs[1])
    cs = _f(1.0) / f2s
    d = f2 + g2
    sn = _cmul((r[0] / d, r[1] / d), (gs[0], -gs[1]))
    for _ in range(abs(count)):
        m = safmx2 if count > 0 else safmn2
        r = (r[0] * m, r[1] * m)
    return [cs, sn, r]


# ---- backward properties, in exact arithmetic on the COMPUTED outputs, in units of eps ---------------------------------
def prop_refl(x, out):
    """out = (beta, v..., tau).  resid: ||(I - tau v v') x - beta e1|| / ||x||;  orth: |tau (1 + ||v_tail||^2) - 2|
    (tau = 0 is H = I: both are zero when the tail is)."""
    if not _fin(out):
        return {"resid": math.inf, "orth": math.inf}
    X = [Fr(v) for v in x]
    beta, tau = Fr(float(out[0])), Fr(float(out[-1]))
    v = [Fr(1)] + [Fr(float(t)) for t in out[1:-1]]
    if tau == 0:
        return {"resid": _rel(sum(t * t for t in X[1:]) + (X[0] - beta) ** 2, sum(t * t for t in X)), "orth": 0.0}
    w = tau * sum(a * b for a, b in zip(v, X))
    res = [a - w * b for a, b in zip(X, v)]
    res[0] -= beta
    return {"resid": _rel(sum(t * t for t in res), sum(t * t for t in X)),
            "orth": _flt(abs(tau * sum(t * t for t in v) - 2)) / EPS}


def prop_larfg(x, out):
    """inv: |mult (alpha - beta) - 1| (tau = 0: mult = 0, H = I)."""
    tau, beta, mult = out
    if not _fin(out):
        return {"inv": math.inf}
    if tau == 0.0 and mult == 0.0 and x[1] == 0.0:
        return {"inv": 0.0}
    return {"inv": _flt(abs(Fr(float(mult)) * (Fr(x[0]) - Fr(float(beta))) - 1)) / EPS}


def prop_zlarfg(x, out):
    tau, beta, mult = out
    if not _fin(list(tau) + [beta] + list(mult)):
        return {"inv": math.inf}
    if x[2] == 0.0 and x[1] == 0.0 and tau == (0.0, 0.0) and mult == (0.0, 0.0):
        return {"inv": 0.0}
    dr, di = Fr(x[0]) - Fr(float(beta)), Fr(x[1])
    mr, mi = Fr(float(mult[0])), Fr(float(mult[1]))
    return {"inv": _rel((mr * dr - mi * di - 1) ** 2 + (mr * di + mi * dr) ** 2, Fr(1))}


def prop_givens(x, out):
    """unit: |cs^2 + sn^2 - 1|;  zero: |-sn f + cs g| / |(f, g)|."""
    if not _fin(out):
        return {"unit": math.inf, "zero": math.inf}
    f, g = Fr(x[0]), Fr(x[1])
    cs, sn = Fr(float(out[0])), Fr(float(out[1]))
    return {"unit": _flt(abs(cs * cs + sn * sn - 1)) / EPS, "zero": _rel((cs * g - sn * f) ** 2, f * f + g * g)}


def prop_zgivens(x, out):
    """unit: |cs^2 + |sn|^2 - 1|;  zero: |-conj(sn) f + cs g| / |(f, g)|."""
    cs, sn, r = out
    if not _fin([cs] + list(sn) + list(r)):
        return {"unit": math.inf, "zero": math.inf}
    a, b, c, d = (Fr(v) for v in x)
    cs, sr, si = Fr(float(cs)), Fr(float(sn[0])), Fr(float(sn[1]))
    zr = cs * c - (sr * a + si * b)  # -conj(sn) f + cs g
    zi = cs * d - (sr * b - si * a)
    return {"unit": _flt(abs(cs * cs + sr * sr + si * si - 1)) / EPS,
            "zero": _rel(zr * zr + zi * zi, a * a + b * b + c * c + d * d)}


# ---- conventions that hold exactly ---------------------------------------------------------------------------------------
def conv_refl(x, out):
    bad = []
    beta, tau = out[0], out[-1]
    if any(t != 0.0 for t in x[1:]):
        if not (beta != 0.0 and _sgn(beta) == -_sgn(x[0])):
            bad.append("beta does not have the sign of -x0")
        if not 1.0 <= tau <= 2.0:
            bad.append(f"tau = {tau!r} outside [1, 2]")
    elif _bits(tau) != _bits(0.0):
        bad.append("zero tail without tau = 0")
    return bad


def conv_larfg(x, out):
    tau, beta, _ = out
    return conv_refl([x[0], x[1]], [beta, 0.0, tau])


def conv_zlarfg(x, out):
    tau, beta, _ = out
    bad = []
    if x[2] == 0.0 and x[1] == 0.0:
        if tau != (0.0, 0.0):
            bad.append("zero tail and real alpha without tau = 0")
    else:
        if tau == (0.0, 0.0):
            bad.append("tau = 0 although H is not the identity")
        if not 1.0 <= tau[0] <= 2.0:
            bad.append(f"Re tau = {tau[0]!r} outside [1, 2]")
        if not (beta != 0.0 and _sgn(beta) == -_sgn(x[0])):
            bad.append("beta does not have the sign of -Re alpha")
    return bad


def conv_givens(x, out):
    f, g = x
    cs, _, r = out
    bad = []
    if f != 0.0 and g != 0.0:
        if abs(f) > abs(g) and not cs > 0.0:
            bad.append("|f| > |g| without cs > 0")
        if abs(f) <= abs(g) and not r > 0.0:
            bad.append("|f| <= |g| without r > 0")
    return bad


def conv_zgivens(x, out):
    cs = out[0]
    return [] if cs >= 0.0 else [f"cs = {cs!r} is not >= 0"]


# ---- tables -----------------------------------------------------------------------------------------------------------
def around(c):
    """The largest double below c, c, the smallest double above c."""
    return [float(np.nextafter(c, -math.inf)), float(c), float(np.nextafter(c, math.inf))]


def _signed(rs, shape, elo, ehi):
    """m 2^e with m uniform in [1, 2), e a uniform integer in [elo, ehi] drawn per entry, random sign."""
    m = 1.0 + rs.random_sample(shape)
    return np.ldexp(m, rs.randint(elo, ehi + 1, shape)) * rs.choice([-1.0, 1.0], shape)


class Table:
    def __init__(self, ncols):
        self.ncols = ncols
        self.rows = []
        self.labels = []

    def add(self, row, label=None):
        row = [float(v) for v in row]
        assert len(row) == self.ncols and _fin(row)
        self.rows.append(row)
        self.labels.append(label)

    def bulk(self, arr):
        for r in np.asarray(arr):
            self.add(r)

    def done(self):
        assert 0 < len(self.rows) <= MAXCASES, len(self.rows)
        return np.array(self.rows), self.labels


def _put(n, k, v, rest):
    row = list(rest)
    row.insert(k, v)
    assert len(row) == n
    return row


def table_refl(nv):
    """psd_refl2 / psd_refl3, their _lean forms and psd_reflector_small."""
    rs = np.random.RandomState(1000 + nv)
    T = Table(nv)
    T.bulk(_signed(rs, (350, nv), -1074, 1022))  # the whole domain, every ratio |x0| / |tail|
    T.bulk(_signed(rs, (350, nv), -464, 464))    # inside the window of the fast paths (1e-140, 1e140)
    T.bulk(_signed(rs, (60, nv), -3, 3))
    pad = [0.0] * (nv - 2)
    lo, hi = around(1e-140), around(1e140)
    tiny_in, big_in = lo[2], hi[0]
    for side, v in zip(("below", "at", "above"), hi):
        # 1e140 on the largest magnitude: in x0 and in each tail entry, the others moderate and extreme
        for mate in (1.0, big_in, tiny_in, -3e-300):
            T.add([v, mate] + pad, f"1e140 {side} in x0, tail {mate:.3g}")
            T.add([-v, mate] + pad, f"1e140 {side} in -x0, tail {mate:.3g}")
        for k in range(1, nv):
            for x0 in (0.0, -0.0, 1.0, -big_in, 1e-300):
                T.add(_put(nv, k, v, [x0] + pad), f"1e140 {side} in x{k}, x0 {x0:.3g}")
    for side, v in zip(("below", "at", "above"), lo):
        # 1e-140 on the largest tail magnitude
        for k in range(1, nv):
            for x0 in (0.0, 1.0, -1e139, 1e-300, TINY, -big_in):
                T.add(_put(nv, k, v, [x0] + pad), f"1e-140 {side} in x{k}, x0 {x0:.3g}")
        if nv == 3:
            T.add([1.0, v, -v], f"1e-140 {side} in x1 and x2")
    # 1e280 / 1e-280 on the sums of squares (psd_refl32_pair, _lean): spread evenly over two entries
    for side, v in zip(("below", "at", "above"), around(1e140 / math.sqrt(2.0))):
        T.add([v, -v] + pad, f"1e280 {side} as x0^2 + x1^2")
        if nv == 3:
            T.add([tiny_in, v, v], f"1e280 {side} as x1^2 + x2^2")
    for side, v in zip(("below", "at", "above"), around(1e-140 / math.sqrt(2.0))):
        if nv == 3:
            T.add([1.0, v, v], f"1e-280 {side} as x1^2 + x2^2, x0 1")
            T.add([-1e139, v, -v], f"1e-280 {side} as x1^2 + x2^2, x0 -1e139")
    # sfmin on |beta| (dlarfg tail; one pass of the kount loop: a second is unreachable in double, the smallest
    # subnormal times 1 / sfmin = 2^-105 is above sfmin)
    for side, v in zip(("below", "at", "above"), around(SFMIN)):
        T.add([0.0, v] + pad, f"sfmin {side} as |beta|, x0 0")
        T.add([-0.0, -v] + pad, f"sfmin {side} as |beta|, x0 -0")
        T.add([v, TINY] + pad, f"sfmin {side} in x0, tail 2^-1074")
        T.add([-0.6 * v, 0.8 * v] + pad, f"sfmin {side} as |beta|, (0.6, 0.8) split")
    for x0, t in ((1e-300, 1e-310), (TINY, TINY), (-3 * TINY, 4 * TINY), (0.0, TINY), (1e-310, -1e-300), (2e-292, 1e-292)):
        T.add([x0, t] + pad, "kount loop")
    # degenerate: zero tails (tau = 0, x untouched); x0 = +-0 with a tail; one-element and subnormal tails
    for x0 in (1.5, -2.0, 0.0, -0.0, 1e300, -TINY, 1e-140, 1e140):
        T.add([x0] + [0.0] * (nv - 1), "zero tail")
        T.add([x0] + [-0.0] * (nv - 1), "zero tail (-0)")
    for z in (0.0, -0.0):
        for t in (1.0, -1e-300, TINY, 1e200, 3e-141, -1e141):
            for k in range(1, nv):
                T.add(_put(nv, k, t, [z] + pad), f"x0 {z!r}, one-element tail")
        if nv == 3:
            T.add([z, 3.0, -4.0], f"x0 {z!r}")
    for x0, t in ((1.0, TINY), (1e-300, 2e-310), (-3.0, 1e-320), (1e139, -4e-322), (-1e-139, 2e-308)):
        for k in range(1, nv):
            T.add(_put(nv, k, t, [x0] + pad), "subnormal one-element tail")
    if nv == 3:
        T.add([-3.0, 1e-320, -4e-322], "subnormal tail")
        T.add([2.0, 0.0, 1.0], "one-element tail")
        T.add([2.0, 1.0, -0.0], "one-element tail")
    return T.done()


def table_refl32_pair():
    """Both reflectors of one call: a 3-vector and a 2-vector, each from its own table, in range and out of range in
    every combination (one combined range test decides for both)."""
    r3, l3 = table_refl(3)
    r2, l2 = table_refl(2)
    T = Table(5)
    rs = np.random.RandomState(1032)
    fast3 = [i for i in range(len(r3)) if path_refl(r3[i]) == "fast"]
    fast2 = [i for i in range(len(r2)) if path_refl(r2[i]) == "fast"]
    for i in rs.choice(fast3, 300):  # both in range
        T.add(list(r3[i]) + list(r2[rs.choice(fast2)]))
    for i in rs.choice(len(r3), 250):  # anything with anything
        T.add(list(r3[i]) + list(r2[rs.choice(len(r2))]))
    e3 = [i for i in range(len(r3)) if l3[i]]
    e2 = [i for i in range(len(r2)) if l2[i]]
    for i in e3:  # every edge of one with a moderate and with an edge case of the other
        T.add(list(r3[i]) + [1.5, -0.75], "x: " + l3[i])
        T.add(list(r3[i]) + list(r2[e2[i % len(e2)]]), "x: " + l3[i] + "; y: " + l2[e2[i % len(e2)]])
    for i in e2:
        T.add([0.5, -2.0, 1.25] + list(r2[i]), "y: " + l2[i])
    return T.done()


def table_reflector_small():
    r3, l3 = table_refl(3)
    r2, l2 = table_refl(2)
    T = Table(4)
    for r, l in zip(r3[250:], l3[250:]):
        T.add([3.0] + list(r), l)
    for r, l in zip(r2[250:], l2[250:]):
        T.add([2.0] + list(r) + [7.0], l)  # (the fourth slot is not part of a 2-vector)
    return T.done()


def table_larfg():
    """psd_h2_larfg(alpha, xnorm), xnorm >= 0 a norm; max(|alpha|, xnorm) >= DBL_MIN (module docstring)."""
    rs = np.random.RandomState(1009)
    T = Table(2)
    for arr in (_signed(rs, (450, 2), -1074, 1022), _signed(rs, (350, 2), -464, 464), _signed(rs, (60, 2), -3, 3)):
        arr[:, 1] = np.abs(arr[:, 1])
        T.bulk(arr[np.max(np.abs(arr), axis=1) >= DBL_MIN])
    lo, hi = around(1e-140), around(1e140)
    for side, v in zip(("below", "at", "above"), hi):
        for mate in (1.0, hi[0], lo[2], 3e-300, 0.0):
            T.add([-v, mate], f"1e140 {side} in alpha, xnorm {mate:.3g}")
            if mate:
                T.add([mate, v], f"1e140 {side} in xnorm, alpha {mate:.3g}")
        T.add([0.0, v], f"1e140 {side} in xnorm, alpha 0 (mn == 0)")
        T.add([-0.0, v], f"1e140 {side} in xnorm, alpha -0 (mn == 0)")
    for side, v in zip(("below", "at", "above"), lo):
        for mate in (1.0, -hi[0], 1e-139):
            T.add([mate, v], f"1e-140 {side} in mn = xnorm, alpha {mate:.3g}")
            T.add([-v, abs(mate)], f"1e-140 {side} in mn = |alpha|, xnorm {abs(mate):.3g}")
        T.add([v, 0.5 * v], f"1e-140 {side} in ww = |alpha|")
        T.add([-0.5 * v, v], f"1e-140 {side} in ww = xnorm")
        T.add([0.0, v], f"1e-140 {side} in ww = xnorm, alpha 0 (mn == 0)")
    for z in (0.0, -0.0):
        for t in (1.0, 1e-139, 1e139, 1e-300, 1e300, DBL_MIN):
            T.add([z, t], f"alpha {z!r} (mn == 0), xnorm {t:.3g}")
    for side, v in zip(("below", "at", "above"), around(SFMIN)):
        T.add([0.0, v], f"sfmin {side} as |beta|, alpha 0")
        T.add([-0.6 * v, 0.8 * v], f"sfmin {side} as |beta|, (0.6, 0.8) split")
        T.add([v, TINY], f"sfmin {side} in alpha, xnorm 2^-1074")
    for a, t in ((1e-300, 1e-310), (DBL_MIN, TINY), (-3e-308, 4e-308), (0.0, DBL_MIN), (1e-310, 1e-300), (-TINY, 3e-308)):
        T.add([a, t], "kount loop")
    for a in (1.5, -2.0, 0.0, -0.0, 1e300, -TINY, 1e-140):
        T.add([a, 0.0], "zero tail")
    for a, t in ((1.0, TINY), (-3.0, 1e-320), (1e139, 4e-322), (-1e-139, 2e-309)):
        T.add([a, t], "subnormal xnorm")
    return T.done()


def table_zlarfg():
    """psd_zh2_larfg(alpha, xnorm): no range guard, the dlapy3 norm for every input; sfmin = DBL_MIN / eps."""
    rs = np.random.RandomState(1010)
    T = Table(3)
    for arr in (_signed(rs, (450, 3), -1074, 1022), _signed(rs, (300, 3), -464, 464), _signed(rs, (60, 3), -3, 3)):
        arr[:, 2] = np.abs(arr[:, 2])
        T.bulk(arr[np.max(np.abs(arr), axis=1) >= DBL_MIN])
    for side, v in zip(("below", "at", "above"), around(ZSFMIN)):
        T.add([0.0, 0.0, v], f"sfmin {side} as |beta|, alpha 0")
        T.add([0.0, -v, 0.0], f"sfmin {side} as |beta|, alpha imaginary, zero tail")
        T.add([-0.6 * v, 0.0, 0.8 * v], f"sfmin {side} as |beta|, (0.6, 0, 0.8) split")
        T.add([v, TINY, TINY], f"sfmin {side} in Re alpha")
    for row in ((1e-300, 1e-310, 1e-305), (DBL_MIN, TINY, 0.0), (-3e-308, 4e-308, 1e-308), (0.0, 0.0, DBL_MIN),
                (-0.0, 1e-320, 1e-300)):
        T.add(row, "kount loop")
    for a in (1.5, -2.0, 0.0, -0.0, 1e300, -TINY):
        T.add([a, 0.0, 0.0], "zero tail, real alpha: tau = 0")
        T.add([a, -0.0, 0.0], "zero tail, Im alpha -0: tau = 0")
    for a in (1.5, -2.0, 0.0, -0.0, 1e-200):
        for b in (1.0, -1e-300, 1e300, DBL_MIN):
            T.add([a, b, 0.0], "zero tail, Im alpha != 0: tau != 0")
    for z in (0.0, -0.0):
        for t in (1.0, 1e-300, 1e300):
            T.add([z, 0.0, t], f"Re alpha {z!r}, real")
            T.add([z, -t, t], f"Re alpha {z!r}")
    for row in ((1.0, -1.0, TINY), (-3.0, 1e-320, 4e-322), (1e-300, 2e-310, 3e-315)):
        T.add(row, "subnormal xnorm")
    return T.done()


def table_givens():
    rs = np.random.RandomState(1011)
    T = Table(2)
    T.bulk(_signed(rs, (400, 2), -1074, 1022))
    T.bulk(_signed(rs, (350, 2), -484, 484))  # the common case: max(|f|, |g|) in (safmn2, safmx2)
    T.bulk(_signed(rs, (60, 2), -3, 3))
    for nm, c in (("safmx2", SAFMX2), ("safmn2", SAFMN2)):
        cs = around(c)
        for side, v in zip(("below", "at", "above"), cs):
            for mate in (1.0, -1e-300, v, -cs[0], cs[2], TINY):
                if abs(mate) <= abs(v) or c == SAFMN2:
                    T.add([v, mate], f"{nm} {side} in f, g {mate:.3g}")
                    T.add([-mate, -v], f"{nm} {side} in g, f {-mate:.3g}")
    for f, g in ((1e300, 1.0), (-1e300, 1e299), (1e-320, 1e-322), (TINY, -TINY), (3e-300, -4e-300), (1.7e308, 1e-308)):
        T.add([f, g], "several rescaling passes")
        T.add([g, f], "several rescaling passes")
    for f in (2.0, -3.0, 0.0, -0.0, 1e300, TINY, -1e-200):
        T.add([f, 0.0], "g = 0")
        T.add([f, -0.0], "g = -0")
    for g in (2.0, -3.0, 1e300, -TINY, 1e-200):
        T.add([0.0, g], "f = 0")
        T.add([-0.0, g], "f = -0")
    for v in (1.0, -1.0, 3e-7, -1e200, 1e-200, TINY, SAFMX2, SAFMN2):
        T.add([v, v], "f = g")
        T.add([v, -v], "f = -g")
    for f, g in ((-2.0, 1.0), (-1e200, 1e100), (-3.0, -1.0), (-1e-200, 1e-250), (-1e300, 1e299), (-1e-310, 1e-312)):
        T.add([f, g], "|f| > |g|, f < 0: the sign rule")
    for f, g in ((-1.0, 2.0), (-1.0, -2.0), (-1.0, 1.0), (-1e-300, 1e300)):
        T.add([f, g], "|f| <= |g|, f < 0")
    return T.done()


def table_zgivens():
    rs = np.random.RandomState(1012)
    T = Table(4)
    T.bulk(_signed(rs, (350, 4), -1074, 1021))
    T.bulk(_signed(rs, (300, 4), -484, 484))  # the common case
    T.bulk(_signed(rs, (60, 4), -3, 3))
    # f negligible against g (f2 <= max(g2, 1) DBL_MIN) at a moderate scale
    T.bulk(np.hstack([_signed(rs, (100, 2), -700, -505), _signed(rs, (100, 2), -100, 100)]))
    T.bulk(np.hstack([_signed(rs, (100, 2), -540, -490), _signed(rs, (100, 2), -30, 1)]))
    for nm, c in (("safmx2", SAFMX2), ("safmn2", SAFMN2)):
        cs = around(c)
        for side, v in zip(("below", "at", "above"), cs):
            for k in range(4):
                for rest in ((0.5, -0.25, 0.125), (cs[0], -cs[0], cs[0]), (1e-300, 0.0, -TINY), (0.0, 0.0, 0.0)):
                    if c == SAFMN2 or max(abs(t) for t in rest) <= v:
                        T.add(_put(4, k, v, rest), f"{nm} {side} in slot {k}, others {rest[0]:.3g}..")
    # f2 = max(g2, 1) DBL_MIN +- 1 ulp: g2 <= 1 (f2 against DBL_MIN) and g2 > 1
    for side, v in zip(("below", "at", "above"), around(2.0 ** -511)):
        T.add([v, 0.0, 1e-3, 2e-3], f"f2 {side} DBL_MIN, g2 < 1")
        T.add([0.0, -v, 0.0, 1.0], f"f2 {side} DBL_MIN, g2 = 1")
        T.add([v, 0.0, 2e-146, 0.0], f"f2 {side} DBL_MIN, g just above safmn2")
    for side, v in zip(("below", "at", "above"), around(2.0 ** -411)):
        T.add([v, 0.0, 2.0 ** 100, 0.0], f"f2 {side} g2 DBL_MIN, g = 2^100")
        T.add([0.0, v, 0.0, -(2.0 ** 100)], f"f2 {side} g2 DBL_MIN, g = -2^100 i")
    for side, v in zip(("below", "at", "above"), around(2.0 ** -27)):
        T.add([v, 0.0, 2.0 ** 484, 0.0], f"f2 {side} g2 DBL_MIN, g = 2^484")
    for f in ((2.0, -1.0), (0.0, 3.0), (-1e300, 1e300), (1e-200, 0.0), (TINY, -TINY), (0.0, 0.0), (-0.0, 0.0)):
        T.add(list(f) + [0.0, 0.0], "g = 0")
    for g in ((2.0, -1.0), (0.0, 3.0), (-1e300, 1e300), (1e-200, 0.0), (TINY, -TINY), (-4e-310, 3e-310)):
        T.add([0.0, 0.0] + list(g), "f = 0")
        T.add([-0.0, 0.0] + list(g), "f = 0")
    for v in ((1.0, 0.0), (3.0, -4.0), (1e200, 1e199), (-1e-200, 1e-201), (TINY, 0.0), (SAFMX2, SAFMX2)):
        T.add(list(v) + list(v), "f = g")
    for row in ((-2.0, 0.0, 1.0, 0.0), (-1e200, 0.0, 0.0, 1e100), (0.0, -3.0, -1.0, 0.0), (1e300, -1e300, 1e299, 0.0),
                (1e-310, -1e-312, 1e-311, 0.0), (1.7e307, 1e-308, -1e307, 1.0)):
        T.add(row, "several rescaling passes / signs")
    return T.done()


def _log_uniform(rs, n, lo, hi):
    """m 2^e as in _signed (positive), kept inside [lo, hi]."""
    elo, ehi = math.frexp(lo)[1] - 1, math.frexp(hi)[1] - 1
    v = np.abs(_signed(rs, 4 * n, elo, ehi))
    v = v[(v >= lo) & (v <= hi)]
    assert len(v) >= n
    return v[:n]


def table_rcp():
    rs = np.random.RandomState(1001)
    lo, hi = RAW_DOMAINS["rcp"]
    T = Table(1)
    T.bulk((_log_uniform(rs, 1400, lo, hi) * rs.choice([-1.0, 1.0], 1400)).reshape(-1, 1))
    T.bulk(_signed(rs, (300, 1), -2, 2))
    for v in (lo, hi, 0.25, float(np.nextafter(16.0, 0.0)), 1.0, 3.0):
        T.add([v], "domain edge")
        T.add([-v], "domain edge")
    for e in (-460, -100, -1, 0, 1, 7, 100, 460):
        for v in around(2.0 ** e):
            T.add([v], "power of two +- 1 ulp")
    return T.done()


def table_sqrt_pair():
    rs = np.random.RandomState(1002)
    lo, hi = RAW_DOMAINS["sqrt_pair"]
    T = Table(1)
    T.bulk(_log_uniform(rs, 1400, lo, hi).reshape(-1, 1))
    T.bulk(np.abs(_signed(rs, (300, 1), -2, 3)))
    for v in (lo, hi, 0.25, float(np.nextafter(8.0, 0.0)), 1.0, 2.0, 9.0, 1e-280, 1e280, 4.1e283, SAFMN2 ** 2):
        for w in around(v):
            if lo <= w <= hi:
                T.add([w], "domain edge / guard image")
    for e in (-1020, -1000, -500, -3, 0, 1, 2, 500, 960, 971):
        for v in around(2.0 ** e):
            T.add([v], "power of two +- 1 ulp")
    return T.done()


def table_rsqrt2():
    rs = np.random.RandomState(1003)
    lo, hi = RAW_DOMAINS["rsqrt2_a"]
    T = Table(2)
    a = _log_uniform(rs, 1400, lo, hi)
    g2 = _log_uniform(rs, 1400, TINY, hi)
    g2[::7] = 0.0
    T.bulk(np.stack([a, a + g2], axis=1))
    a = np.abs(_signed(rs, 300, -2, 3))
    T.bulk(np.stack([a, a + np.abs(_signed(rs, 300, -2, 3))], axis=1))
    for v in (lo, hi, 1.0, 2.0, 4.0):
        for w in around(v):
            if lo <= w <= hi:
                T.add([w, w], "domain edge")
                T.add([w, w + hi], "domain edge")
    return T.done()


def table_c3():
    """(m, x, e, bz, bin): psd_c3_expo(m), psd_c3_ldexp(x, e), psd_c3_beta(bz, bin, e); every result finite.  bz and bin
    are the betas of two chain vectors scaled to unit maximum: zero or of order one, so bz / bin is zero or normal (a
    subnormal quotient would be rounded before the exponent is applied, in the routine and in any float64 form of it)."""
    rs = np.random.RandomState(1014)
    T = Table(5)
    m = _signed(rs, 600, -1074, 1023)
    m[::5] = np.abs(m[::5])
    # one e serves psd_c3_ldexp and psd_c3_beta.  First rows: e over the whole range with a quotient of order one (beta
    # from below 2^-1074 up to 2^1018) and x such that x 2^e covers the same range; then e moderate, anything else
    e = rs.randint(-1080, 1019, 300)
    kx = np.array([rs.randint(max(-1074, -1080 - k), min(1023, 1018 - k) + 1) for k in e])
    x = np.ldexp(1.0 + rs.random_sample(300), kx) * rs.choice([-1.0, 1.0], 300)
    T.bulk(np.stack([m[:300], x, e.astype(float), _signed(rs, 300, -3, 3), _signed(rs, 300, -3, 3)], axis=1))
    x = _signed(rs, 600, -1074, 1023)
    eb = np.array([rs.randint(max(-400, -1080 - k), min(400, 1018 - k) + 1) for k in np.frexp(x)[1]])
    bz, bn = _signed(rs, 600, -300, 300), _signed(rs, 600, -300, 300)
    T.bulk(np.stack([m, x, eb.astype(float), bz, bn], axis=1)[300:])
    for v in (0.0, -0.0, -1.0, -TINY, -DBL_MAX, TINY, 3 * TINY, DBL_MIN, DBL_MAX, 1.7e308, 1.6e308):
        T.add([v, 1.0, 0.0, 1.0, 1.0], "expo: zero, negative, subnormal, largest")
    for k in (-1074, -1073, -1023, -1022, -1021, -1, 0, 1, 52, 53, 1022, 1023):
        for v in around(2.0 ** k):
            if v > 0.0:
                T.add([v, -v, -k, 0.0, 3.0], "expo: power of two +- 1 ulp; ldexp to about 1")
    for xx, ee in ((1.0, -1074), (1.0, -1075), (1.5, -1074), (1.5, -1075), (-1.25, -1023), (1.0 + EPS, -1022), (3.0, -1076),
                   (1.0 + EPS, -1023), (-(2.0 - EPS), -1023), (TINY, 1074), (-3 * TINY, 1000), (DBL_MIN, 1022 + 1023),
                   (-TINY, 2097), (1e-310, 40), (DBL_MAX, -2097), (DBL_MAX, -2098), (-1e300, -2060), (0.0, 5), (-0.0, -5)):
        T.add([1.0, xx, ee, 0.0, 7.0], "ldexp into and out of the subnormal range")
    for bz_, bin_, ee in ((1.0, 0.0, 3), (-2.0, -0.0, -3), (0.0, 0.0, 0), (0.0, 2.0, 4), (-0.0, 2.0, 4), (1.0, 3.0, -1074),
                          (1.0, 3.0, 1022), (1e-290, 1e10, -60), (1e300, 1e-5, -2060), (-7.0, 3.0, -1050)):
        T.add([1.0, 1.0, ee, bz_, bin_], "beta: bin = 0, signed zeros, subnormal results")
    return T.done()


# ---- which path the guards send a case down (float64 evaluation without contraction; the device forms its sums of squares
# with fused multiply-adds, so a case within an ulp of a guard on a SUM may sit on the other side there) ---------------
def path_refl(x):
    x = [float(v) for v in x]
    tmax = max(abs(t) for t in x[1:])
    if tmax == 0.0:
        return "tau0"
    if max(tmax, abs(x[0])) < 1e140 and tmax > 1e-140:
        return "fast"
    nrm = float(np.hypot(x[0], float(ieee_norm2([_f(t) for t in x[1:]]))))
    return "kount" if nrm < SFMIN else "dlarfg"


def path_lean(x):
    x = [_f(v) for v in x]
    tx2 = x[1] * x[1] + (x[2] * x[2] if len(x) == 3 else _f(0.0))
    nx2 = x[0] * x[0] + tx2
    return "fast" if nx2 < 1e280 and tx2 > 1e-280 else "full:" + path_refl(x)


def path_pair(x):
    a, b = path_lean(x[:3]), path_lean(x[3:])
    return "fast" if a == b == "fast" else "full:" + path_refl(x[:3]) + "+" + path_refl(x[3:])


def path_larfg(x):
    alpha, xnorm = float(x[0]), float(x[1])
    if xnorm == 0.0:
        return "tau0"
    ww, mn = max(abs(alpha), xnorm), min(abs(alpha), xnorm)
    if ww < 1e140 and ww > 1e-140 and (mn == 0.0 or mn > 1e-140):
        return "fast"
    return "kount" if float(np.hypot(alpha, xnorm)) < SFMIN else "dlarfg"


def path_zlarfg(x):
    if x[2] == 0.0 and x[1] == 0.0:
        return "tau0"
    return "kount" if float(_hypot3(_f(x[0]), _f(x[1]), _f(x[2]))) < ZSFMIN else "plain"


def path_givens(x):
    f, g = float(x[0]), float(x[1])
    if g == 0.0:
        return "g0"
    if f == 0.0:
        return "f0"
    s = max(abs(f), abs(g))
    return "down" if s >= SAFMX2 else ("up" if s <= SAFMN2 else "fast")


def path_zgivens(x):
    x = [_f(v) for v in x]
    s = max(abs(v) for v in x)
    f2, g2 = x[0] * x[0] + x[1] * x[1], x[2] * x[2] + x[3] * x[3]
    if SAFMN2 < s < SAFMX2 and f2 > max(g2, 1.0) * DBL_MIN:
        return "fast"
    if s <= SAFMN2 and x[2] == 0.0 and x[3] == 0.0:
        return "g0"
    sc = "down:" if s >= SAFMX2 else ("up:" if s <= SAFMN2 else "")
    k = 0
    while s >= SAFMX2 or s <= SAFMN2:
        m = SAFMN2 if s >= SAFMX2 else SAFMX2
        x = [v * m for v in x]
        s *= m
        k += 1
        if (m == SAFMN2 and s < SAFMX2) or (m == SAFMX2 and s > SAFMN2):
            break
    f2, g2 = x[0] * x[0] + x[1] * x[1], x[2] * x[2] + x[3] * x[3]
    if f2 <= max(g2, 1.0) * DBL_MIN:
        return sc + ("f0" if f2 == 0.0 and x[0] == 0.0 and x[1] == 0.0 else "rare")
    return sc + "plain"


# ---- the ops --------------------------------------------------------------------------------------------------------------
class Op:
    """outs: (name, slot) or (name, (slot_re, slot_im)) in the order exact / ieee return them."""

    def __init__(self, table, outs, exact, ieee, props=None, conv=None, path=None, table_of=None, need_paths=()):
        self.table, self.outs, self.exact, self.ieee = table, outs, exact, ieee
        self.props, self.conv, self.path = props, conv, path
        self.table_of = table_of  # the op whose table (and reference) this one shares
        self.need_paths = need_paths


def _refl_op(nv, table_of=None, path=path_refl, need=("tau0", "fast", "dlarfg", "kount")):
    outs = [("beta", 0)] + [(f"v{k}", k) for k in range(1, nv)] + [("tau", nv)]
    return Op(lambda: table_refl(nv), outs, lambda x: exact_refl(list(x)), lambda x: ieee_reflector(list(x))[0],
              prop_refl, conv_refl, path, table_of, need)


def _pair_exact(x):
    return exact_refl(list(x[:3])) + exact_refl(list(x[3:]))


def _pair_ieee(x):
    return ieee_reflector(list(x[:3]))[0] + ieee_reflector(list(x[3:]))[0]


def _pair_props(x, out):
    a, b = prop_refl(list(x[:3]), out[:4]), prop_refl(list(x[3:]), out[4:])
    return {k: max(a[k], b[k]) for k in a}


def _small_n(x):
    return 3 if x[0] == 3.0 else 2


def _small_pack(x, o):  # (beta, v1, v2, tau) with v2 = 0.0 for n = 2
    return o if _small_n(x) == 3 else [o[0], o[1], 0.0, o[2]]


def _small_unpack(x, out):
    return out if _small_n(x) == 3 else [out[0], out[1], out[3]]


def _c3_exact(x):
    m, xx, e, bz, bn = x
    e = int(e)
    ex = float(math.frexp(m)[1]) if 0.0 < m < 1.7e308 else 0.0
    ld = Fr(xx) * Fr(2) ** e
    be = 0.0 if bn == 0.0 else Fr(bz) / Fr(bn) * Fr(2) ** e
    return [ex, ld if ld != 0 else math.copysign(0.0, xx), be]


def _c3_ieee(x):
    m, xx, e, bz, bn = x
    e = int(e)
    with np.errstate(all="ignore"):
        return [float(math.frexp(m)[1]) if 0.0 < m < 1.7e308 else 0.0, math.ldexp(xx, e),
                0.0 if bn == 0.0 else math.ldexp(float(_f(bz) / _f(bn)), e)]


OPS = {
    "rcp": Op(table_rcp, [("rcp", 0)], lambda x: [1 / Fr(x[0])], lambda x: [_f(1.0) / _f(x[0])]),
    "sqrt_pair": Op(table_sqrt_pair, [("g", 0), ("rg", 1)], lambda x: [fsqrt(Fr(x[0])), 1 / fsqrt(Fr(x[0]))],
                    lambda x: [np.sqrt(_f(x[0])), _f(1.0) / np.sqrt(_f(x[0]))]),
    "rsqrt2": Op(table_rsqrt2, [("ra", 0), ("rb", 1)], lambda x: [1 / fsqrt(Fr(x[0])), 1 / fsqrt(Fr(x[1]))],
                 lambda x: [_f(1.0) / np.sqrt(_f(x[0])), _f(1.0) / np.sqrt(_f(x[1]))]),
    "refl2": _refl_op(2),
    "refl3": _refl_op(3),
    "refl2_lean": _refl_op(2, "refl2", path_lean, ("fast", "full:fast", "full:tau0", "full:dlarfg", "full:kount")),
    "refl3_lean": _refl_op(3, "refl3", path_lean, ("fast", "full:fast", "full:tau0", "full:dlarfg", "full:kount")),
    "refl32_pair": Op(table_refl32_pair,
                      [("beta", 0), ("v1", 1), ("v2", 2), ("tau", 3), ("beta'", 4), ("w1", 5), ("tau'", 6)],
                      _pair_exact, _pair_ieee, _pair_props,
                      lambda x, o: conv_refl(list(x[:3]), o[:4]) + conv_refl(list(x[3:]), o[4:]), path_pair,
                      None, ("fast", "full:fast+fast")),
    "reflector_small": Op(table_reflector_small, [("beta", 0), ("v1", 1), ("v2", 2), ("tau", 3)],
                          lambda x: _small_pack(x, exact_refl(list(x[1:1 + _small_n(x)]))),
                          lambda x: _small_pack(x, ieee_reflector(list(x[1:1 + _small_n(x)]))[0]),
                          lambda x, o: prop_refl(list(x[1:1 + _small_n(x)]), _small_unpack(x, o)),
                          lambda x, o: conv_refl(list(x[1:1 + _small_n(x)]), _small_unpack(x, o)),
                          lambda x: path_refl(x[1:1 + _small_n(x)]).replace("fast", "dlarfg"), None,
                          ("tau0", "dlarfg", "kount")),
    "h2_larfg": Op(table_larfg, [("tau", 0), ("beta", 1), ("mult", 2)], lambda x: exact_larfg(x[0], x[1]),
                   lambda x: ieee_larfg(x[0], x[1]), prop_larfg, conv_larfg, path_larfg, None,
                   ("tau0", "fast", "dlarfg", "kount")),
    "zh2_larfg": Op(table_zlarfg, [("tau", (0, 1)), ("beta", 2), ("mult", (3, 4))], lambda x: exact_zlarfg(*x),
                    lambda x: ieee_zlarfg(*x), prop_zlarfg, conv_zlarfg, path_zlarfg, None, ("tau0", "plain", "kount")),
    "givens": Op(table_givens, [("cs", 0), ("sn", 1), ("r", 2)], lambda x: exact_givens(*x), lambda x: ieee_givens(*x),
                 prop_givens, conv_givens, path_givens, None, ("g0", "f0", "fast", "up", "down")),
    "zgivens": Op(table_zgivens, [("cs", 0), ("sn", (1, 2)), ("r", (3, 4))], lambda x: exact_zgivens(*x),
                  lambda x: ieee_zgivens(*x), prop_zgivens, conv_zgivens, path_zgivens, None,
                  ("fast", "g0", "rare", "f0", "up:plain", "down:plain", "up:rare", "down:rare", "up:f0",
                   "down:f0")),
    "c3_scale": Op(table_c3, [("expo", 0), ("ldexp", 1), ("beta", 2)], _c3_exact, _c3_ieee),
}
OPS["zgivens_lean"] = Op(table_zgivens, OPS["zgivens"].outs, OPS["zgivens"].exact, OPS["zgivens"].ieee, prop_zgivens,
                         conv_zgivens, path_zgivens, "zgivens", OPS["zgivens"].need_paths)
OP_NAMES = ("rcp", "sqrt_pair", "rsqrt2", "refl2", "refl3", "refl2_lean", "refl3_lean", "refl32_pair", "reflector_small",
            "h2_larfg", "zh2_larfg", "givens", "zgivens", "zgivens_lean", "c3_scale")
assert set(OP_NAMES) == set(OPS)

_CACHE = {}


def _pick(row, outs):
    """The outputs of one row of 8 slots (or of a list in output order) as floats / (re, im) pairs."""
    return [(float(row[s[0]]), float(row[s[1]])) if isinstance(s, tuple) else float(row[s]) for _, s in outs]


def _flat(vals):
    return [t for v in vals for t in (v if isinstance(v, tuple) else (v,))]


def reference(name):
    """Table, exact outputs, and the gates from the restatement — computed once per session and never modified."""
    op = OPS[name]
    key = op.table_of or name
    if key in _CACHE:
        return _CACHE[key]
    rows, labels = op.table()
    exact, e_ieee, p_ieee = [], {nm: 0.0 for nm, _ in op.outs}, {}
    with np.errstate(all="ignore"):
        for x in rows:
            x = [float(v) for v in x]
            ex = op.exact(x)
            exact.append(ex)
            ie = [(float(v[0]), float(v[1])) if isinstance(v, tuple) else float(v) for v in op.ieee(x)]
            for (nm, _), g, e in zip(op.outs, ie, ex):
                e_ieee[nm] = max(e_ieee[nm], err_ulps(g, e))
            if op.props:
                for k, v in op.props(x, ie).items():
                    p_ieee[k] = max(p_ieee.get(k, 0.0), v)
    ref = dict(rows=rows, labels=labels, exact=exact, e_ieee=e_ieee, p_ieee=p_ieee,
               B={k: 2.0 * v + 1.0 for k, v in e_ieee.items()}, Bp={k: 2.0 * v + 1.0 for k, v in p_ieee.items()})
    _CACHE[key] = ref
    return ref


def check_op(engine, name):
    """Runs the op's table through psd_diag_scalar in one launch and applies every check to every case.  Prints E_ieee,
    B and the engine's worst error per output and property; returns them."""
    with np.errstate(all="ignore"):  # (the restated guards square out-of-range operands, as the routines do)
        return _check_op(engine, name)


def _check_op(engine, name):
    op, ref = OPS[name], reference(name)
    rows = ref["rows"]
    assert all(math.isfinite(b) for b in list(ref["B"].values()) + list(ref["Bp"].values())), (name, ref["B"], ref["Bp"])
    if op.path:
        seen = {op.path(x) for x in rows}
        assert set(op.need_paths) <= seen, (name, sorted(set(op.need_paths) - seen))
    out = engine.diag_scalar(name, rows)
    assert out.shape == (len(rows), 8)
    used = set(_flat([s for _, s in op.outs]))
    assert not np.any(out[:, [k for k in range(8) if k not in used]]), "unused output slots must be zero"
    worst, pworst, fails = {nm: (0.0, -1) for nm, _ in op.outs}, {}, []
    for i, x in enumerate(rows):
        x = [float(v) for v in x]
        got = _pick(out[i], op.outs)
        for (nm, _), g, e in zip(op.outs, got, ref["exact"][i]):
            err = err_ulps(g, e)
            if err > worst[nm][0]:
                worst[nm] = (err, i)
            if not err <= ref["B"][nm]:
                fails.append(f"case {i} {x}: {nm} = {g!r} is {err:.3g} ulp from exact (gate {ref['B'][nm]:.3g})")
        if op.props:
            for k, v in op.props(x, got).items():
                if v > pworst.get(k, (0.0, -1))[0]:
                    pworst[k] = (v, i)
                if not v <= ref["Bp"][k]:
                    fails.append(f"case {i} {x}: property {k} = {v:.3g} eps (gate {ref['Bp'][k]:.3g})")
        if op.conv:
            fails += [f"case {i} {x}: {msg}" for msg in op.conv(x, got)]
    for nm, _ in op.outs:
        print(f"{name:16s} {nm:6s} E_ieee {ref['e_ieee'][nm]:8.3f}  B {ref['B'][nm]:8.3f}  engine {worst[nm][0]:8.3f} ulp"
              f"  (case {worst[nm][1]})")
    for k in ref["Bp"]:
        w = pworst.get(k, (0.0, -1))
        print(f"{name:16s} {k:6s} E_ieee {ref['p_ieee'][k]:8.3f}  B {ref['Bp'][k]:8.3f}  engine {w[0]:8.3f} eps"
              f"  (case {w[1]})")
    assert not fails, f"{name}: {len(fails)} failures of {len(rows)} cases:\n" + "\n".join(fails[:20])
    return dict(worst=worst, pworst=pworst, ref=ref)


def edge_report(name):
    """The labelled edge cases of an op's table with the path the guards send each down (profiles/scalar/README.md)."""
    op, ref = OPS[name], reference(name)
    return [(lab, op.path(x) if op.path else "") for x, lab in zip(ref["rows"], ref["labels"]) if lab]


def check_argument_codes(engine):
    """The negative info values of psd_diag_scalar, as listed in psd_mi355x.h."""
    import ctypes as C

    import psd_amd
    import pytest

    lib, ctx = engine.lib, engine.ctx
    dp = C.POINTER(C.c_double)
    xin, out = np.zeros((2, 8)), np.full((2, 8), np.nan)
    xin[:, 0] = (4.0, -0.5)
    pin, pout = xin.ctypes.data_as(dp), out.ctypes.data_as(dp)
    info = C.c_int(0)

    def call(ctx=ctx, op=0, ncases=2, pin=pin, pout=pout):
        rc = lib.psd_diag_scalar(ctx, op, ncases, pin, pout, C.byref(info))
        assert rc == info.value
        return rc

    nops = len(OP_NAMES)
    assert [call(), call(ctx=None), call(op=-1), call(op=nops), call(ncases=0), call(ncases=-3), call(pin=None),
            call(pout=None)] == [0, -1, -2, -2, -3, -3, -4, -5]
    assert np.array_equal(out[:, 0], [0.25, -2.0]) and not np.any(out[:, 1:])
    assert lib.psd_diag_scalar(ctx, 0, 2, pin, pout, None) == 0  # info may be NULL
    assert psd_amd.DIAG_SCALAR_OPS == {nm: k for k, nm in enumerate(OP_NAMES)}
    with pytest.raises(ValueError):
        engine.diag_scalar("no_such_op", xin)
