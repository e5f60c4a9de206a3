#!/usr/bin/env python3
"""Timing of partial_pschur on sparse (CSR) factors and of its SpMV kernel (psd_kr_csr_mv).

  python tools/krylov_csr_timing.py call   [--json out.json]
  rocprofv3 --kernel-trace -f csv -d DIR -o csr -- python tools/krylov_csr_timing.py kernel --plan DIR/plan.json
  python tools/krylov_csr_timing.py summarise --plan DIR/plan.json --trace DIR/.../csr_kernel_trace.csv [--json out.json]

call: partial_pschur(…, 6, "LM", tol=1e-10, restarts=100, seed=1) on device-resident factors (torch sparse-CSR tensors),
host clock around a device synchronise, the median of the timed calls after one warm-up call per shape.  8192 x 16 with 32
entries per row runs through both operators: the CSR entry, and the same factors densified through the dense entry (the
only way to run them without the CSR entry).  2^20 x 8 with 16 entries per row runs through the CSR entry alone, with the
device memory the call holds at its peak.

kernel: psd_?_csr_matvec (one launch of the driver's kernel per call) for n in {8192, 2^17, 2^20} x k in {4, 16, 64}
entries per row at every group width; the launches are listed in order in the plan file.  The kernel times come from the
kernel trace of that run: summarise pairs the psd_kr_csr_mv dispatches with the plan in start order, takes the fastest
launch of each (shape, G) after the first, and reports the bytes the product needs over that time:
nnz * 12 + (n + 1) * 8 + n * 8 + n * 8 (ComplexF64: 20 and 16 for the value and the vector terms)."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

GROUPS = (1, 2, 4, 8, 16, 32, 64)
COPY_TBS = 6.3  # the device's achievable copy rate, TB/s (what matvec_bandwidth.json is quoted against)


def auto_group(n, nnz):
    g = 1
    while g < 64 and g * n < nnz:
        g *= 2
    return g


def spmv_bytes(n, nnz, cplx=False):
    return nnz * (20 if cplx else 12) + (n + 1) * 8 + 2 * n * (16 if cplx else 8)


def host_rows(n, k, seed):
    """k entries per row at random columns, as numpy CSR arrays."""
    rng = np.random.default_rng(seed)
    return (np.arange(n + 1, dtype=np.int64) * k, rng.integers(0, n, n * k, dtype=np.int32),
            rng.standard_normal(n * k))


def device_factors(torch, n, p, k, seed):
    """diag(d) + k entries per row of 0.3 / sqrt(k) times standard normal numbers (d: 16 leading entries from 2 to 1.3,
    the rest 1), generated on the device: p torch sparse-CSR tensors."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = torch.ones(n, device="cuda", dtype=torch.float64)
    d[:16] = torch.linspace(2.0, 1.3, 16, device="cuda", dtype=torch.float64)
    crow = torch.arange(n + 1, device="cuda", dtype=torch.int64) * (k + 1)
    out = []
    for _ in range(p):
        col = torch.randint(0, n, (n, k), generator=g, device="cuda", dtype=torch.int64)
        col = torch.cat([torch.arange(n, device="cuda", dtype=torch.int64)[:, None], col], dim=1)
        val = torch.randn((n, k), generator=g, device="cuda", dtype=torch.float64).mul_(0.3 / np.sqrt(k))
        val = torch.cat([d[:, None], val], dim=1)
        out.append(torch.sparse_csr_tensor(crow, col.reshape(-1), val.reshape(-1), size=(n, n)))
    return out


def timed_calls(torch, eng, As, nev, reps):
    ms, P, h = [], None, None
    for rep in range(reps + 1):  # the first call pays the code-object load and the allocations
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P, h = eng.partial_pschur(As, nev, "LM", tol=1e-10, restarts=100, seed=1)
        torch.cuda.synchronize()
        if rep:
            ms.append(1e3 * (time.perf_counter() - t0))
    st = P.stats
    return dict(call_ms=round(statistics.median(ms), 2), call_ms_min=round(min(ms), 2), call_ms_max=round(max(ms), 2),
                reps=reps, nconv=h.nconverged, products=h.mvproducts, restarts=st.restarts, nreorth=st.nreorth,
                ms_arnoldi=round(st.ms_arnoldi, 2), ms_proj=round(st.ms_proj, 2), ms_basis=round(st.ms_basis, 2))


def run_call(a):
    import torch

    torch.cuda.init()
    import psd_amd

    eng = psd_amd.Engine(0)
    rows = []
    n, p, k = 8192, 16, 32
    As = device_factors(torch, n, p, k, 1000 + n + p)
    row = dict(case=f"{n}x{p}", k=k, operator="csr", nev=a.nev, **timed_calls(torch, eng, As, a.nev, a.reps))
    print(json.dumps(row), flush=True)
    rows.append(row)
    dA = torch.stack([s.to_dense() for s in As])
    row = dict(case=f"{n}x{p}", k=k, operator="dense", nev=a.nev, **timed_calls(torch, eng, dA, a.nev, a.reps))
    print(json.dumps(row), flush=True)
    rows.append(row)
    del dA, As
    n, p, k = 1 << 20, 8, 16
    As = device_factors(torch, n, p, k, 1000 + p)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    factor_bytes = sum(s.values().numel() * 8 + s.col_indices().numel() * 8 + s.crow_indices().numel() * 8 for s in As)
    row = dict(case=f"{n}x{p}", k=k, operator="csr", nev=a.nev, **timed_calls(torch, eng, As, a.nev, a.reps))
    # the call's own device memory: the int32 column indices and the result block the mirror makes, and the driver's
    # bases and work vectors ((maxdim + 1) n p elements), from the shapes
    kmax = 20
    row["factor_bytes_torch"] = factor_bytes
    row["call_bytes_from_shapes"] = (sum(s.col_indices().numel() * 4 for s in As) + 8 * p * n * kmax
                                     + 8 * p * n * (kmax + 1) + 8 * n)
    row["device_free_before_bytes"] = free0
    print(json.dumps(row), flush=True)
    rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


def run_kernel(a):
    import torch

    torch.cuda.init()
    import psd_amd

    eng = psd_amd.Engine(0)
    plan = []
    for n in (8192, 1 << 17, 1 << 20):
        for k in (4, 16, 64):
            indptr, ind, data = host_rows(n, k, n + k)
            A = psd_amd.CSR(n, indptr, ind, data)
            x = np.random.default_rng(1).standard_normal(n)
            for g in GROUPS:
                for rep in range(a.reps + 1):
                    eng.csr_matvec(A, x, group=g)
                    plan.append(dict(n=n, k=k, nnz=n * k, group=g, rep=rep))
            print(f"n={n} k={k} done", flush=True)
    with open(a.plan, "w") as f:
        json.dump(plan, f)


def run_summarise(a):
    plan = json.load(open(a.plan))
    rows = [r for r in csv.DictReader(open(a.trace)) if "psd_kr_csr_mv" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(rows) != len(plan):
        raise SystemExit(f"{len(rows)} psd_kr_csr_mv dispatches in the trace, {len(plan)} launches in the plan")
    us = {}
    for item, r in zip(plan, rows):
        if item["rep"]:  # (the first launch of a (shape, G) is the warm-up)
            us.setdefault((item["n"], item["k"], item["group"]), []).append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = []
    for n, k in sorted({(key[0], key[1]) for key in us}):
        nnz = n * k
        by = spmv_bytes(n, nnz)
        per_g = {g: dict(us_min=round(min(us[(n, k, g)]), 2), us_max=round(max(us[(n, k, g)]), 2)) for g in GROUPS}
        ga = auto_group(n, nnz)
        gb = min(GROUPS, key=lambda g: per_g[g]["us_min"])
        t = per_g[ga]["us_min"]
        row = dict(n=n, k=k, nnz=nnz, bytes=by, auto_group=ga, auto_us=t, auto_TBs=round(by / t / 1e6, 3),
                   auto_of_copy_rate=round(by / t / 1e6 / COPY_TBS, 3), best_group=gb, best_us=per_g[gb]["us_min"],
                   per_group=per_g)
        print(json.dumps(row), flush=True)
        out.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["call", "kernel", "summarise"])
    ap.add_argument("--nev", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--plan", default="csr_plan.json")
    ap.add_argument("--trace", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    {"call": run_call, "kernel": run_kernel, "summarise": run_summarise}[a.mode](a)


if __name__ == "__main__":
    main()
