#!/usr/bin/env python3
"""Timing of Engine.psylvester_dev and Engine.subspacecond_dev — the periodic Sylvester solve and xTRSEN's two numbers
for ONE large periodic Schur form — on the MI355X, swept over the tile width (profiles/sylv/README.md).

For every shape n x p x m one synthetic periodic Schur form is made on the device as tools/psylvester_batch_timing.py
makes its batches — T_l = triu(Gaussian) * 0.1 with the diagonals of the product's rows in two groups, the leading m in
[1, 1.5] and the others in [3, 3.5] (ComplexF64: times random phases), so that the split is well conditioned at every
order; Float64: the last factor with 2 x 2 blocks at rows j, j + 1, j = 1, 5, 9, ... that the split does not cut — and,
with T left on the device, for every tile width of --tiles (PSD_SYL_TILE of a fresh Engine) timed
  solve     Engine.psylvester_dev (C = -T12): one warm-up, then --repeats calls, and
  subcond   Engine.subspacecond_dev: --cond-repeats calls (its kernels beyond the solve's are the norm and the
            estimator's vector kernel, a few launches of microseconds: they have no warm-up of their own).
Wall time is a host clock around the call with the device idle before and after; the device times of the solve, update
and estimator launches, the launch counts and the estimator's solves come from the call's stats.  Medians and extremes.

  (default)  Float64 1024 x 16 m = 256, Float64 512 x 16 m = 256, ComplexF64 512 x 8 m = 128; tiles 2 ... 64

Every shape runs in a process of its own under `timeout`; the tool stops at the first one that fails.  One JSON line
per (shape, tile) on stdout; --json FILE collects them.  There is no gate: nothing at these orders existed before."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_SHAPES = "d1024x16x256,d512x16x256,z512x8x128"


def parse_shapes(text):
    """[(ComplexF64, n, p, m)] from d1024x16x256,z512x8x128"""
    return [(s[0] == "z",) + tuple(int(x) for x in s[1:].split("x")) for s in text.split(",") if s]


def make_form(cplx, n, p, m):
    import numpy as np
    import torch

    gen = torch.Generator(device="cuda")
    gen.manual_seed(9100 + n + 1000 * p)
    dt = torch.complex128 if cplx else torch.float64
    T = 0.1 * torch.triu(torch.randn((p, n, n), dtype=dt, device="cuda", generator=gen), diagonal=1)
    d = torch.cat([torch.linspace(1.0, 1.5, m, dtype=torch.float64), torch.linspace(3.0, 3.5, n - m, dtype=torch.float64)])
    d = (d ** (1.0 / p)).to("cuda").expand(p, n).clone().to(dt)
    if cplx:
        d = d * torch.exp(1j * torch.rand((p, n), dtype=torch.float64, device="cuda", generator=gen) * (2 * np.pi))
    T = T + torch.diag_embed(d)
    if not cplx:
        for j in range(1, n - 1, 4):
            if j + 1 != m:  # (the split stays between two blocks)
                T[p - 1, j + 1, j] = -0.5
                T[p - 1, j, j + 1] = 0.7
                T[p - 1, j + 1, j + 1] = T[p - 1, j, j]
    return T.transpose(1, 2).contiguous().transpose(1, 2)  # the column-major blocks of the device entries


def run_shape(cplx, n, p, m, tiles, repeats, cond_repeats):
    import torch

    torch.cuda.init()
    import psd_amd

    T = make_form(cplx, n, p, m)
    for tile in tiles:
        os.environ["PSD_SYL_TILE"] = str(tile)  # (read when the context is created)
        eng = psd_amd.Engine(0)
        run_one(eng, T, cplx, n, p, m, repeats, cond_repeats)
        eng.close()


def run_one(eng, T, cplx, n, p, m, repeats, cond_repeats):
    import numpy as np
    import torch

    row = dict(n=n, p=p, m=m, complex=bool(cplx), repeats=repeats, cond_repeats=cond_repeats)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def solve():
        return eng.psylvester_dev(T, m, lr="R", schurindex=p)

    def subcond():
        return eng.subspacecond_dev(T, m, lr="R", schurindex=p)

    timed(solve)  # warm-up
    ts, tc, ds, dc = [], [], [], []
    for _ in range(repeats):
        ms, X = timed(solve)
        ts.append(ms)
        ds.append(eng.psylvester_stats.asdict())
    for _ in range(cond_repeats):
        ms, (s, sep) = timed(subcond)
        tc.append(ms)
        dc.append(eng.subspacecond_stats.asdict())

    def med(rows, key):
        return float(np.median([r[key] for r in rows]))

    st = ds[-1]
    row["tile"], row["ntiles"], row["ndiag"] = st["tile"], st["ntiles"], st["ndiag"]
    row["solve"] = dict(wall_ms=float(np.median(ts)), wall_ms_min=min(ts), wall_ms_max=max(ts), ms_solve=med(ds, "ms_solve"),
                        ms_update=med(ds, "ms_update"), nsolve=st["nsolve"], nupdate=st["nupdate"])
    st = dc[-1]
    row["subcond"] = dict(wall_ms=float(np.median(tc)), wall_ms_min=min(tc), wall_ms_max=max(tc), ms_solve=med(dc, "ms_solve"),
                          ms_update=med(dc, "ms_update"), ms_est=med(dc, "ms_est"), nsolve=st["nsolve"],
                          nupdate=st["nupdate"], nest_solves=st["nest_solves"], nest_steps=st["nest_steps"],
                          nest_iter=st["nest_iter"], nnorms=st["nnorms"])
    row["s_min"], row["sep"], row["x_max"] = float(s.min()), float(sep), float(X.abs().max())
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="[d|z] n x p x m, comma separated")
    ap.add_argument("--tiles", default="2,4,8,16,32,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cond-repeats", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per shape")
    ap.add_argument("--json", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    tiles = [int(t) for t in args.tiles.split(",") if t]
    if args.one:
        run_shape(*parse_shapes(args.one)[0], tiles, args.repeats, args.cond_repeats)
        return 0
    rows, code = [], 0
    for shape in args.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", shape,
               "--tiles", args.tiles, "--repeats", str(args.repeats), "--cond-repeats", str(args.cond_repeats)]
        pr = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(pr.stdout)
        sys.stdout.flush()
        rows += [json.loads(ln) for ln in pr.stdout.splitlines() if ln.startswith("{")]
        if pr.returncode != 0:  # a failure, a fault or a time limit: nothing more is started on the device
            print(json.dumps(dict(shape=shape, failed=pr.returncode)), flush=True)
            code = 1
            break
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(dict(rows=rows), fh, indent=1)
    return code


if __name__ == "__main__":
    sys.exit(main())
