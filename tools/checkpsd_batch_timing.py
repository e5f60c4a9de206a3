#!/usr/bin/env python3
"""Timing of Engine.checkpsd_batch on the MI355X (profiles/batch/README.md).

For every shape nb x n x p synthetic decompositions are made on the device — Z_l the Q factor of a Gaussian matrix,
T_l = triu(Gaussian) / sqrt(n) (Float64: the first factor with sub-diagonal entries 0.3 at rows j + 1, j = 0, 3, 6, ...),
A_l = Z_l T_l Z_{l+1}' — and, with T, Z, A left on the device, verified
  batch   by one Engine.checkpsd_batch call on the tensors (psd_?_checkpsd_batch_dev), and
  loop    by Engine.checkpsd_dev problem by problem on the slices of the same buffers (psd_?_checkpsd_dev: four launches
          per factor, the code that existed before this entry, unchanged): the baseline.
One warm-up of each, then `--repeats` timed runs of each, alternating: wall time around the call(s) with the device idle
before and after; the medians and the extremes are reported, with the device time and the launches of the batch stats
and the largest difference between the two paths' numbers.

  (default)  n in {8, 16, 24, 32, 48, 64}, p = 8, nb = 1024
  --complex  ComplexF64 decompositions

The sweep ends at PSD_BCK_NMAX = 64: the kernel keeps W = T_l Z_b' of a whole factor in LDS and has no form above that
order (above it the batch entry IS the loop).  Every shape runs in a process of its own under `timeout`; the tool stops
at the first one that fails.  One JSON line per shape on stdout; --json FILE collects them."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_shapes(text):
    return [tuple(int(x) for x in s.split("x")) for s in text.split(",") if s]


def default_shapes():
    return [(1024, n, 8) for n in (8, 16, 24, 32, 48, 64)]


def run_one(nb, n, p, cplx, repeats):
    import numpy as np
    import torch

    torch.cuda.init()
    import psd_amd

    eng = psd_amd.Engine(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9000 + n + 1000 * p)
    dt = torch.complex128 if cplx else torch.float64

    def gauss():
        return torch.randn((nb, p, n, n), dtype=dt, device="cuda", generator=gen)

    Z = torch.linalg.qr(gauss())[0]
    T = torch.triu(gauss()) / np.sqrt(n)
    if not cplx:
        for j in range(0, n - 1, 3):
            T[:, 0, j + 1, j] = 0.3
    A = Z @ T @ torch.roll(Z, -1, dims=1).mH  # 'R', all-true signature: (a, b) = (l, l + 1)
    # the [nb][p][n][n] column-major blocks of the device entries, and the tensors that view them as [nb, p, n, n]
    Tc, Zc, Ac = (x.transpose(2, 3).contiguous() for x in (T, Z, A))
    Tv, Zv, Av = (x.transpose(2, 3) for x in (Tc, Zc, Ac))
    del T, Z, A
    row = dict(nb=nb, n=n, p=p, complex=bool(cplx), repeats=repeats)

    def batch():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.checkpsd_batch(Tv, Zv, Av, lr="R", schurindex=1, details=True)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def loop():
        torch.cuda.synchronize()
        singles = []
        t0 = time.perf_counter()
        for q in range(nb):
            singles.append(eng.checkpsd_dev(Tc[q].data_ptr(), Zc[q].data_ptr(), Ac[q].data_ptr(), n, p, "R", 1, cplx=cplx))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), singles

    batch(), loop()  # warm-up
    tb, tl = [], []
    for _ in range(repeats):
        ms, out = batch()
        tb.append(ms)
        st = eng.checkpsd_batch_stats
        ms, singles = loop()
        tl.append(ms)
    assert Tv.data_ptr() == Tc.data_ptr()  # (the tensors were not copied on the way in)
    row["batch"] = dict(wall_ms=float(np.median(tb)), wall_ms_min=min(tb), wall_ms_max=max(tb), ms_kernels=st.ms_kernels,
                        nlaunch=int(st.nlaunch), ngroups=int(st.ngroups), nfail=int(st.nfail))
    row["loop"] = dict(wall_ms=float(np.median(tl)), wall_ms_min=min(tl), wall_ms_max=max(tl), nlaunch=4 * p * nb,
                       nfail=int(sum(1 for s in singles if not s[0])))
    row["max_err"] = float(out[1].max())
    row["max_abs_diff_err"] = float(max(np.abs(out[1][q] - singles[q][1]).max() for q in range(nb)))
    row["max_abs_diff_orth"] = float(max(np.abs(out[2][q] - singles[q][2]).max() for q in range(nb)))
    row["wall_ratio"] = row["loop"]["wall_ms"] / row["batch"]["wall_ms"]
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=None, help="nb x n x p, comma separated (default: the grid above)")
    ap.add_argument("--complex", action="store_true", dest="cplx")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per shape")
    ap.add_argument("--json", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        run_one(*parse_shapes(args.one)[0], args.cplx, args.repeats)
        return 0
    shapes = parse_shapes(args.shapes) if args.shapes else default_shapes()
    rows = []
    for s in shapes:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one",
               "%dx%dx%d" % s, "--repeats", str(args.repeats)] + (["--complex"] if args.cplx else [])
        pr = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(pr.stdout)
        sys.stdout.flush()
        if pr.returncode != 0:  # a failure, a fault or a time limit: nothing more is started on the device
            print(json.dumps(dict(shape=s, failed=pr.returncode)), flush=True)
            break
        rows += [json.loads(ln) for ln in pr.stdout.splitlines() if ln.startswith("{")]
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(dict(rows=rows), fh, indent=1)
    return 0 if len(rows) == len(shapes) else 1


if __name__ == "__main__":
    sys.exit(main())
