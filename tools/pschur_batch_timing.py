#!/usr/bin/env python3
"""Timing of the batched entries on the MI355X (profiles/batch/README.md).

  call   (default)  Engine.pschur_batch_ against a loop of Engine.pschur_ over the same problems on the same engine:
                    wall time around the call(s) and the device times of the stats (hess / formq / iterate / copy), the
                    second of two runs of each.
  --loop-only       the loop alone: what a commit without the batched entries can run (the baseline of record).
  --sweep           the batched reduction (phessenberg_batch_) against nb single reductions (phessenberg_) over the order,
                    nb = 64, p = 8: the measurement PSD_BH_NMAX is set from.  Runs on the diagnostic library with the cap
                    lifted (PSD_BH_NMAX in the environment), so that every order takes the batched kernel.

  --complex         the ComplexF64 family: Engine.zpschur_batch_ against the loop of Engine.pschur_ over the same complex
                    problems, in the same process and run, nb = 256, p = 8 over the orders of --orders: the
                    measurement PSD_ZB_NMAX is set from (the largest order at which the batched call still wins).

  --signed          the signed ComplexF64 family: Engine.zgpschur_batch_ against the loop of Engine.pschur_(..., S=S) over
                    the same problems with the alternating signature (T, F, T, F, ...), nb = 256, p = 8 over the orders of
                    --orders: the measurement the order cap of the signed batch kernels is set from.  Loop and
                    batch alternate, --reps times each after one warm-up pair; the row carries every repetition and the
                    ratio of the fastest ones, and the largest eigenvalue difference between the two on the first problem.

  --signed-real     the signed Float64 family: Engine.dgpschur_batch_ against the loop of Engine.pschur_(..., S=S) over the
                    same real problems over the orders of --orders (nb = --nb, p = 8), otherwise as --signed (same
                    process and run, alternating, repetition 0 the warm-up): the measurement the order cap of the real signed batch kernels (PSD_GB_NMAX) is set from.
                    Each row also carries the spread of the repetitions of either side.

One JSON line per shape on stdout; --json FILE collects them."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def parse_shapes(text):
    return [tuple(int(x) for x in s.split("x")) for s in text.split(",") if s]


def factors(nb, n, p, dtype=None):
    import numpy as np
    import psdtest as pt

    return [pt.bench_factors(n, p, seed=9000 + q, dtype=dtype or np.float64) for q in range(nb)]


def copies(probs):
    return [[a.copy(order="F") for a in A] for A in probs]


def time_loop(eng, probs, lr):
    best = None
    for _ in range(2):
        Ws = copies(probs)
        dev = dict(hess=0.0, formq=0.0, iter=0.0, copy=0.0, total=0.0)
        t0 = time.perf_counter()
        for W in Ws:
            st = eng.pschur_(W, lr).stats
            dev["hess"] += st.ms_hess
            dev["formq"] += st.ms_formq
            dev["iter"] += st.ms_iter
            dev["copy"] += st.ms_copy
            dev["total"] += st.ms_total
        best = dict(wall_ms=1e3 * (time.perf_counter() - t0), **{"ms_" + k: v for k, v in dev.items()})
    return best


def time_batch(eng, probs, lr, cplx=False):
    best = None
    for _ in range(2):
        Ws = copies(probs)
        t0 = time.perf_counter()
        out = eng.zpschur_batch_(Ws, lr) if cplx else eng.pschur_batch_(Ws, lr)
        wall = 1e3 * (time.perf_counter() - t0)
        st = out[0].stats
        best = dict(wall_ms=wall, ms_hess=st.ms_hess, ms_formq=st.ms_formq, ms_iter=st.ms_iter, ms_copy=st.ms_copy,
                    ms_total=st.ms_total, nsweeps=int(st.nsweeps), ticks=int(st.nlaunch_step))
    return best


def time_signed(eng, probs, S, lr, reps, real=False):
    """Loop of single signed calls and the batched call, alternating; repetition 0 is the warm-up."""
    import psdtest as pt

    loops, batches, diff = [], [], None
    for rep in range(reps + 1):
        Ws = copies(probs)
        dev = 0.0
        t0 = time.perf_counter()
        first = None
        for W in Ws:
            ps = eng.pschur_(W, lr, S=S)
            dev += ps.stats.ms_total
            first = first if first is not None else ps.values
        loop = dict(wall_ms=1e3 * (time.perf_counter() - t0), ms_total=dev)
        Ws = copies(probs)
        t0 = time.perf_counter()
        out = eng.dgpschur_batch_(Ws, S, lr) if real else eng.zgpschur_batch_(Ws, S, lr)
        wall = 1e3 * (time.perf_counter() - t0)
        st = out[0].stats
        batch = dict(wall_ms=wall, ms_hess=st.ms_hess, ms_iter=st.ms_iter, ms_copy=st.ms_copy, ms_total=st.ms_total,
                     nsweeps=int(st.nsweeps))
        diff = float(pt.match_eigs(first, out[0].values))
        if rep > 0:
            loops.append(loop)
            batches.append(batch)
    return loops, batches, diff


def time_sweep(eng, nb, n, p):
    probs = factors(nb, n, p)
    for _ in range(2):
        Ws = copies(probs)
        single = 0.0
        for W in Ws:
            single += eng.phessenberg_(W)[2].ms_hess
        Ws = copies(probs)
        batch = eng.phessenberg_batch_(Ws)[1].ms_hess
    return dict(nb=nb, n=n, p=p, ms_hess_single_sum=single, ms_hess_batch=batch, ratio=single / batch if batch else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="256x32x16,256x16x64,64x64x16,1024x8x32", help="nb x n x p, comma separated")
    ap.add_argument("--lr", default="R")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-orders", default="32,64,96,128,192,256")
    ap.add_argument("--complex", dest="cplx", action="store_true")
    ap.add_argument("--orders", "--complex-orders", dest="complex_orders", default="8,16,32,64,96,128",
                    help="orders of --complex, --signed and --signed-real (p = 8)")
    ap.add_argument("--nb", "--complex-nb", dest="complex_nb", type=int, default=256,
                    help="problems per batch of --complex, --signed and --signed-real")
    ap.add_argument("--signed", action="store_true")
    ap.add_argument("--signed-real", dest="signed_real", action="store_true")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--lib", default=None, help="library to load instead of the package's (a build of another commit)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import torch

    torch.cuda.init()
    import psd_amd

    if args.sweep:
        os.environ["PSD_BH_NMAX"] = "2048"
        eng = psd_amd.Engine(0, libpath=psd_amd.DIAG_LIB_PATH)
    else:
        eng = psd_amd.Engine(0, libpath=args.lib)
    rows = []
    if args.sweep:
        for n in [int(x) for x in args.sweep_orders.split(",") if x]:
            rows.append(time_sweep(eng, 64, n, 8))
            print(json.dumps(rows[-1]), flush=True)
    elif args.signed or args.signed_real:
        import numpy as np

        for n in [int(x) for x in args.complex_orders.split(",") if x]:
            nb, p = args.complex_nb, 8
            S = [q % 2 == 0 for q in range(p)]
            if args.lr == "L":
                S = S[::-1]
            dtype = np.float64 if args.signed_real else np.complex128
            probs = factors(nb, n, p, dtype)
            loops, batches, diff = time_signed(eng, probs, S, args.lr, args.reps, real=args.signed_real)
            row = dict(nb=nb, n=n, p=p, lr=args.lr, dtype=np.dtype(dtype).name, S="".join("T" if x else "F" for x in S),
                       loop=loops, batch=batches, eig_diff_problem0=diff)
            row["wall_ratio"] = min(r["wall_ms"] for r in loops) / min(r["wall_ms"] for r in batches)
            for side, runs in (("loop", loops), ("batch", batches)):  # (spread of the repetitions: max / min of the wall times)
                row[side + "_spread"] = max(r["wall_ms"] for r in runs) / min(r["wall_ms"] for r in runs)
            row["device_ratio"] = min(r["ms_total"] for r in loops) / min(r["ms_total"] for r in batches)
            rows.append(row)
            print(json.dumps(row), flush=True)
    elif args.cplx:
        import numpy as np

        for n in [int(x) for x in args.complex_orders.split(",") if x]:
            nb, p = args.complex_nb, 8
            probs = factors(nb, n, p, np.complex128)
            row = dict(nb=nb, n=n, p=p, lr=args.lr, dtype="complex128", loop=time_loop(eng, probs, args.lr),
                       batch=time_batch(eng, probs, args.lr, cplx=True))
            row["wall_ratio"] = row["loop"]["wall_ms"] / row["batch"]["wall_ms"]
            row["device_ratio"] = row["loop"]["ms_total"] / row["batch"]["ms_total"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    else:
        for (nb, n, p) in parse_shapes(args.shapes):
            probs = factors(nb, n, p)
            row = dict(nb=nb, n=n, p=p, lr=args.lr, loop=time_loop(eng, probs, args.lr))
            if not args.loop_only:
                row["batch"] = time_batch(eng, probs, args.lr)
                row["wall_ratio"] = row["loop"]["wall_ms"] / row["batch"]["wall_ms"]
                row["device_ratio"] = row["loop"]["ms_total"] / row["batch"]["ms_total"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(dict(engine=eng.version(), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
