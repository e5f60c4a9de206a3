#!/usr/bin/env python3
"""Timing of partial_pschur (periodic Krylov-Schur, psd_?_partial_pschur_dev) on device-resident dense factors.

  python tools/krylov_timing.py [--cases 4096x8,4096x16,8192x8,8192x16] [--full 4096x16] [--json out.json]

Per case: call time (host clock around a device synchronise), Krylov steps / products / restarts, and the share of
the call spent in the Arnoldi extensions.  The matvec kernel time comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/krylov_timing.py ...` run (kernel psd_kr_mv); the achieved bandwidth
is then bytes_per_product * products / kernel time, with bytes_per_product = n^2 * 8 printed here.  --full also runs the
full device pschur! (psd_d_pschur_dev) on the factors of that case, for comparison (a long call: give the step its own
time limit)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()
import psd_amd  # noqa: E402


def factors(n, p, seed):
    """Dense random factors with a few dominant diagonal entries (well separated dominant Floquet multipliers)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    dA = torch.randn((p, n, n), generator=g, device="cuda", dtype=torch.float64).mul_(0.3 / np.sqrt(n))
    d = torch.ones(n, device="cuda", dtype=torch.float64)
    d[:16] = torch.linspace(2.0, 1.3, 16, device="cuda", dtype=torch.float64)
    dA.diagonal(dim1=1, dim2=2).add_(d)
    return dA.transpose(1, 2).contiguous()  # column-major factor blocks, as the _dev entry takes them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="4096x8,4096x16,8192x8,8192x16")
    ap.add_argument("--full", default="")
    ap.add_argument("--nev", type=int, default=6)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    eng = psd_amd.Engine(0)
    rows = []
    for case in [c for c in a.cases.split(",") if c]:
        n, p = (int(x) for x in case.split("x"))
        dA = factors(n, p, 1000 + n + p)
        # (the tensor is already column-major per factor: hand the blocks over as they are)
        for rep in range(2):  # the first call pays the code-object load and the allocations
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P, h = eng.partial_pschur(dA.transpose(1, 2), a.nev, "LM", tol=1e-10, restarts=100, seed=1)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0)
        st = P.stats
        row = dict(n=n, p=p, nev=a.nev, call_ms=round(ms, 2), nconv=h.nconverged, products=h.mvproducts,
                   restarts=st.restarts, nreorth=st.nreorth, ms_arnoldi=round(st.ms_arnoldi, 2),
                   ms_proj=round(st.ms_proj, 2), ms_basis=round(st.ms_basis, 2), bytes_per_product=8 * n * n,
                   ms_per_product_upper=round(st.ms_arnoldi / max(h.mvproducts, 1), 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del dA
    if a.full:
        n, p = (int(x) for x in a.full.split("x"))
        dA = factors(n, p, 1000 + n + p)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lam, _, st, _ = eng.pschur_dev(dA.data_ptr(), n, p, "L")
        torch.cuda.synchronize()
        row = dict(full_pschur=f"{n}x{p}", call_ms=round(1e3 * (time.perf_counter() - t0), 1),
                   top=[str(x) for x in lam[np.argsort(-np.abs(lam))[:a.nev]]])
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
