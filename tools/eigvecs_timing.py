#!/usr/bin/env python3
"""Timing of eigvecs by periodic back-substitution (psd_?_eigvecs_dev) on device-resident Schur factors.

  python tools/eigvecs_timing.py [--cases d512x16,z512x16,d1024x64,z1024x64] [--ordschur d128x8,d256x16]
                                 [--ordschur-few d1024x64:8] [--json out.json]

Per case (d = Float64, z = ComplexF64): pschur_dev of bench factors in the left orientation, then all eigenvectors from
the factors where pschur_dev left them: the call time (host clock around a device synchronise; second of two calls), the
device times of the solve and of the back-transform (stats), and the achieved f64 rate against the flop counts
solve ~ p n^3 / 3 and back-transform ~ 2 p n^3 real multiply-adds (times 2 for ComplexF64).  The kernel split per
kernel comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/eigvecs_timing.py ...` run.
--ordschur times the reordering method (Engine.eigvecs default, host entry) on all vectors of the given cases;
--ordschur-few times it and the back-substitution on the first k vectors of a case."""
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

SPEC_TFLOPS = 78.6  # MI355X FP64 matrix peak of the public spec sheet


def parse(case):
    return case[0] == "z", *(int(x) for x in case[1:].split("x"))


def decompose(eng, cplx, n, p):
    dt = np.complex128 if cplx else np.float64
    dA = torch.from_numpy(pt.pack(pt.bench_factors(n, p, seed=500 + n + p, dtype=dt), dt)).to("cuda:0")
    dZ = torch.zeros_like(dA)
    torch.cuda.synchronize()
    lam, si, _, _ = (eng.zpschur_dev if cplx else eng.pschur_dev)(dA.data_ptr(), n, p, "L", dZ_ptr=dZ.data_ptr())
    return dA, dZ, lam, si


def time_backsub(eng, dT, dZ, lam, si, sel):
    for _ in range(2):  # the first call pays the code-object load and the allocations
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Vs = eng.eigvecs_dev(dT, dZ, lam, sel, lr="L", schurindex=si)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
    del Vs
    return ms, eng.eigvecs_stats


def host_ps(dT, dZ, lam, si):
    return psd_amd.PeriodicSchur(pt.unpack(dT.cpu().numpy()), pt.unpack(dZ.cpu().numpy()), np.asarray(lam), "L", si)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="d512x16,z512x16,d1024x64,z1024x64")
    ap.add_argument("--ordschur", default="d128x8,d256x16")
    ap.add_argument("--ordschur-few", default="d1024x64:8")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    eng = psd_amd.Engine(0)
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    for case in [c for c in a.cases.split(",") if c]:
        cplx, n, p = parse(case)
        dT, dZ, lam, si = decompose(eng, cplx, n, p)
        ms, st = time_backsub(eng, dT, dZ, lam, si, [True] * n)
        f = 2 if cplx else 1
        solve_macs, back_macs = f * p * n ** 3 / 3, f * 2 * p * n ** 3
        emit(dict(case=case, method="backsub", nvec=st.nvec, call_ms=round(ms, 2), ms_solve=round(st.ms_solve, 2),
                  ms_backtransform=round(st.ms_backtransform, 2), nperturbed=st.nperturbed, nrescaled=st.nrescaled,
                  solve_tflops=round(2 * solve_macs / st.ms_solve * 1e-9, 2),
                  back_tflops=round(2 * back_macs / st.ms_backtransform * 1e-9, 2),
                  overall_fraction_of_spec=round(2 * (solve_macs + back_macs) / st.ms_kernels * 1e-9 / SPEC_TFLOPS, 4)))
        del dT, dZ
    for case in [c for c in a.ordschur.split(",") if c]:
        cplx, n, p = parse(case)
        dT, dZ, lam, si = decompose(eng, cplx, n, p)
        ms_b, _ = time_backsub(eng, dT, dZ, lam, si, [True] * n)
        ps = host_ps(dT, dZ, lam, si)
        t0 = time.perf_counter()
        eng.eigvecs(ps, [True] * n)
        emit(dict(case=case, nvec=n, ordschur_ms=round(1e3 * (time.perf_counter() - t0), 1), backsub_ms=round(ms_b, 2)))
    for spec in [c for c in a.ordschur_few.split(",") if c]:
        case, k = spec.split(":")
        cplx, n, p = parse(case)
        dT, dZ, lam, si = decompose(eng, cplx, n, p)
        sel = [i < int(k) for i in range(n)]
        ms_b, _ = time_backsub(eng, dT, dZ, lam, si, sel)
        ps = host_ps(dT, dZ, lam, si)
        t0 = time.perf_counter()
        eng.eigvecs(ps, sel)
        emit(dict(case=case, nvec=int(k), ordschur_ms=round(1e3 * (time.perf_counter() - t0), 1),
                  backsub_ms=round(ms_b, 2)))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
