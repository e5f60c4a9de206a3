#!/usr/bin/env python3
"""Timing of geigvecs (psd_?_geigvecs_dev) on device-resident factors.

  python tools/geigvecs_timing.py [--cases d512x16,z512x16,d1024x64,z1024x64] [--alltrue d1024x64,z1024x64]
                                  [--json out.json]

--cases (d = Float64, z = ComplexF64): a signed periodic Schur form with alternating S (triangular factors with random
diagonals, a 2x2 block every 37 rows in the real case, random orthogonal Z), all vectors: the call time (host clock
around a device synchronise; second of two calls) and the device times of the solve and of the back-transform (stats).
--alltrue: pschur_dev of bench factors in the left orientation, then all vectors by eigvecs_dev and by geigvecs_dev
(S = None) on the same factors.  The kernel split comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/geigvecs_timing.py ...` run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()
import psd_amd  # noqa: E402
import psdtest as pt  # noqa: E402


def parse(case):
    return case[0] == "z", *(int(x) for x in case[1:].split("x"))


def signed_factors(cplx, n, p, seed):
    """device blocks [p][n][n] (column-major) of a signed Schur form: T (schurindex p - 1) and Z"""
    rs = np.random.RandomState(seed)
    dt = torch.complex128 if cplx else torch.float64
    si = p - 1
    Ts, Zs = [], []
    for l in range(p):
        t = 0.2 * np.triu(rs.randn(n, n) + (1j * rs.randn(n, n) if cplx else 0), 1) / np.sqrt(n)
        np.fill_diagonal(t, (0.5 + rs.rand(n)) * np.where(rs.rand(n) < 0.3, -1, 1))
        Ts.append(t)
    for i in ([] if cplx else range(3, n - 1, 37)):
        T = Ts[si - 1]
        T[i, i + 1], T[i + 1, i], T[i + 1, i + 1] = 0.8, -0.6, T[i, i]
        for l in range(p):
            if l != si - 1:
                Ts[l][i, i] = Ts[l][i + 1, i + 1] = abs(Ts[l][i, i]) + 0.5
                Ts[l][i, i + 1] = 0.0
    for l in range(p):
        Zs.append(np.linalg.qr(rs.randn(n, n) + (1j * rs.randn(n, n) if cplx else 0))[0])
    up = lambda ms: torch.stack([torch.from_numpy(np.ascontiguousarray(m.T)) for m in ms]).to(dt).to("cuda:0")  # noqa
    return up(Ts), up(Zs), si


def timed(fn):
    for _ in range(2):  # the first call pays the code-object load and the allocations
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
    del out
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="d512x16,z512x16,d1024x64,z1024x64")
    ap.add_argument("--alltrue", default="d1024x64,z1024x64")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    eng = psd_amd.Engine(0)
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    for case in [c for c in a.cases.split(",") if c]:
        cplx, n, p = parse(case)
        dT, dZ, si = signed_factors(cplx, n, p, seed=700 + n + p)
        S = [l % 2 == 0 for l in range(p)]
        ms = timed(lambda: eng.geigvecs_dev(dT, dZ, [True] * n, "L", si, S=S))
        st = eng.eigvecs_stats
        emit(dict(case=case, S="alternating", method="geigvecs_dev", nvec=st.nvec, call_ms=round(ms, 2),
                  ms_solve=round(st.ms_solve, 2), ms_backtransform=round(st.ms_backtransform, 2),
                  nperturbed=st.nperturbed, nrescaled=st.nrescaled))
        del dT, dZ
    for case in [c for c in a.alltrue.split(",") if c]:
        cplx, n, p = parse(case)
        dt = np.complex128 if cplx else np.float64
        dT = torch.from_numpy(pt.pack(pt.bench_factors(n, p, seed=500 + n + p, dtype=dt), dt)).to("cuda:0")
        dZ = torch.zeros_like(dT)
        torch.cuda.synchronize()
        lam, si, _, _ = (eng.zpschur_dev if cplx else eng.pschur_dev)(dT.data_ptr(), n, p, "L", dZ_ptr=dZ.data_ptr())
        ms_e = timed(lambda: eng.eigvecs_dev(dT, dZ, lam, [True] * n, lr="L", schurindex=si))
        se = eng.eigvecs_stats
        ms_g = timed(lambda: eng.geigvecs_dev(dT, dZ, [True] * n, "L", si))
        sg = eng.eigvecs_stats
        emit(dict(case=case, S="all true", eigvecs_call_ms=round(ms_e, 2), eigvecs_ms_solve=round(se.ms_solve, 2),
                  eigvecs_ms_backtransform=round(se.ms_backtransform, 2), geigvecs_call_ms=round(ms_g, 2),
                  geigvecs_ms_solve=round(sg.ms_solve, 2), geigvecs_ms_backtransform=round(sg.ms_backtransform, 2),
                  ratio=round(ms_g / ms_e, 3)))
        del dT, dZ
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
