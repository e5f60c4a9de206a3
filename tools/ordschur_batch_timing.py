#!/usr/bin/env python3
"""Timing of the batched reordering on the MI355X (profiles/batch/README.md).

For every shape nb x n x p: nb problems of pt.bench_factors go through Engine.pschur_batch, the eigenvalues at or below the
median modulus are selected per problem (the stable half of a Floquet spectrum), and

  call   (default)  one Engine.ordschur_batch_ call (host entry: wall time, device time of the kernels, copies) against
                    the loop of Engine.ordschur_ calls over the same problems on the same engine, and the device-resident
                    entry on torch tensors (wall time without any host copy of a matrix);
  --loop-only       the loop alone: what a commit without the batched entry can run (the baseline of record; --lib names
                    its library);
  --complex         the ComplexF64 family on the same shapes: Engine.zpschur_batch decomposes complex bench_factors, one
                    Engine.zordschur_batch_ call (psd_z_ordschur_batch) against the loop of Engine.ordschur_
                    (psd_z_ordschur) over the same problems, both host entries with their copies, and the device-resident
                    entry;
  --signed          the signed ComplexF64 family on the same shapes: Engine.zgpschur_batch decomposes complex bench_factors
                    under the alternating signature (T, F, T, F, ...) — a pencil sequence —, one Engine.zgordschur_batch_
                    call (psd_z_gordschur_batch) against the loop of Engine.ordschur_ (psd_z_gordschur) over the same
                    problems, and the device-resident entry;
  --signed-real     the signed Float64 family (family "dg") on the same shapes: Engine.dgpschur_batch decomposes real
                    bench_factors under the alternating signature, one Engine.dgordschur_batch_ call
                    (psd_d_gordschur_batch) against the loop of Engine.ordschur_ (psd_d_gordschur) over the same problems,
                    and the device-resident entry.

The second of two runs of each is reported.  One JSON line per shape on stdout; --json FILE collects them."""
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


def clones(pss):
    import psd_amd

    def mats(ps):
        return [t.copy(order="F") for t in ps.Ts], [z.copy(order="F") for z in ps.Z]

    if isinstance(pss[0], psd_amd.GeneralizedPeriodicSchur):
        return [psd_amd.GeneralizedPeriodicSchur(list(ps.S), *mats(ps), ps.alpha.copy(), ps.beta.copy(), ps.alphascale.copy(),
                                                 ps.orientation, ps.schurindex) for ps in pss]
    return [psd_amd.PeriodicSchur(*mats(ps), ps.values.copy(), ps.orientation, ps.schurindex) for ps in pss]


def entry(eng, family):
    """(the in-place batched method, the name of its stats attribute) of a family: "d", "z", "zg" or "dg"."""
    name = {"d": "ordschur_batch", "z": "zordschur_batch", "zg": "zgordschur_batch", "dg": "dgordschur_batch"}[family]
    return getattr(eng, name + "_"), name + "_stats"


def time_loop(eng, pss, sels):
    best = None
    for _ in range(2):
        work = clones(pss)
        dev = swaps = 0
        t0 = time.perf_counter()
        for ps, s in zip(work, sels):
            st = eng.ordschur_(ps, s).stats
            dev += st.ms_total
            swaps += st.nsweeps
        best = dict(wall_ms=1e3 * (time.perf_counter() - t0), ms_total=dev, nswaps=int(swaps))
    return best


def time_batch(eng, pss, sels, family="d"):
    fn, stats = entry(eng, family)
    best = None
    for _ in range(2):
        work = clones(pss)
        t0 = time.perf_counter()
        fn(work, sels)
        wall = 1e3 * (time.perf_counter() - t0)
        st = getattr(eng, stats)
        best = dict(wall_ms=wall, ms_total=st.ms_total, ms_copy=st.ms_copy, nswaps=int(st.nsweeps), nwindows=int(st.nwindows),
                    window=int(st.window), launches=int(st.nlaunch_step))
    return best


def time_dev(eng, pss, sels, lr, family="d"):
    import numpy as np
    import torch

    fn, stats = entry(eng, family)
    kw = dict(S=pss[0].S) if family in ("zg", "dg") else {}

    T0 = torch.from_numpy(np.array([[np.array(t) for t in ps.Ts] for ps in pss])).cuda().transpose(2, 3).contiguous().transpose(2, 3)
    Z0 = torch.from_numpy(np.array([[np.array(z) for z in ps.Z] for ps in pss])).cuda().transpose(2, 3).contiguous().transpose(2, 3)
    best = None
    for _ in range(2):
        T, Z = T0.clone(), Z0.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(T, Z, sels, lr=lr, schurindex=pss[0].schurindex, **kw)
        torch.cuda.synchronize()
        st = getattr(eng, stats)
        best = dict(wall_ms=1e3 * (time.perf_counter() - t0), ms_total=st.ms_total)
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="256x8x4,256x8x16,256x16x4,256x16x16,256x32x4,256x32x16,256x64x4,256x64x16",
                    help="nb x n x p, comma separated")
    ap.add_argument("--lr", default="R")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--complex", dest="cplx", action="store_true")
    ap.add_argument("--signed", action="store_true", help="signed ComplexF64 problems, alternating signature")
    ap.add_argument("--signed-real", dest="signed_real", action="store_true",
                    help="signed Float64 problems, alternating signature")
    ap.add_argument("--lib", default=None, help="library to load instead of the package's (a build of another commit)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    torch.cuda.init()
    import psd_amd
    import psdtest as pt

    eng = psd_amd.Engine(0, libpath=args.lib)
    rows = []
    family = "dg" if args.signed_real else "zg" if args.signed else "z" if args.cplx else "d"
    for (nb, n, p) in parse_shapes(args.shapes):
        if args.signed_real:
            S = [q % 2 == 0 for q in range(p)]
            pss = eng.dgpschur_batch([pt.bench_factors(n, p, seed=9000 + q) for q in range(nb)],
                                     S[::-1] if args.lr == "L" else S, args.lr)
        elif args.signed:
            S = [q % 2 == 0 for q in range(p)]
            pss = eng.zgpschur_batch([pt.bench_factors(n, p, seed=9000 + q, dtype=np.complex128) for q in range(nb)],
                                     S[::-1] if args.lr == "L" else S, args.lr)
        elif args.cplx:
            pss = eng.zpschur_batch([pt.bench_factors(n, p, seed=9000 + q, dtype=np.complex128) for q in range(nb)], args.lr)
        else:
            pss = eng.pschur_batch([pt.bench_factors(n, p, seed=9000 + q) for q in range(nb)], args.lr)
        sels = np.array([np.abs(ps.values) <= np.sort(np.abs(ps.values))[n // 2] for ps in pss])
        row = dict(nb=nb, n=n, p=p, lr=args.lr, dtype="float64" if family in ("d", "dg") else "complex128", family=family,
                   signed=args.signed or args.signed_real,
                   loop=time_loop(eng, pss, sels))
        if not args.loop_only:
            row["batch"] = time_batch(eng, pss, sels, family)
            row["dev"] = time_dev(eng, pss, sels, args.lr, family)
            row["wall_ratio"] = row["loop"]["wall_ms"] / row["batch"]["wall_ms"]
            row["device_ratio"] = row["loop"]["ms_total"] / row["batch"]["ms_total"] if row["batch"]["ms_total"] else None
            row["swaps_per_s"] = 1e3 * row["batch"]["nswaps"] / row["batch"]["wall_ms"]
            row["swaps_per_s_dev"] = 1e3 * row["batch"]["nswaps"] / row["dev"]["wall_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(dict(engine=eng.version(), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
