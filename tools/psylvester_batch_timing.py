#!/usr/bin/env python3
"""Timing of Engine.psylvester_batch and Engine.subspacecond_batch on the MI355X (profiles/batch/README.md).

For every shape nb x n x p synthetic periodic Schur forms are made on the device — T_l = triu(Gaussian) * 0.1 with the
diagonals of the product's rows in two groups, the leading m = n / 2 in [1, 1.5] and the others in [3, 3.5] (ComplexF64:
times random phases), so that the split is well conditioned at every order; Float64: the last factor with 2 x 2 blocks
at rows j, j + 1, j = 1, 5, 9, ... that the split does not cut — and, with T left on the device, timed
  solve     one Engine.psylvester_batch call on the tensor (C = -T12: one launch of psd_bsyl_solve per group), and
  subcond   one Engine.subspacecond_batch call (the solve, the norms, and the estimator's solves and steps).
One warm-up of each, then `--repeats` timed runs of each: wall time around the call with the device idle before and
after; the medians and the extremes are reported with the device time and the launch counts of the stats.

For orientation only, a CPU figure stands next to them, of the first `--cpu` problems scaled to nb: at p = 1
scipy.linalg.lapack.?trsen(job='B') per problem, otherwise the dense Kronecker solve (numpy.linalg.solve on the
p m k x p m k matrix; only where p m k <= 4096).  There is no gate: nothing before this entry computed these numbers.

  (default)  n in {8, 16, 32, 64, 128}, p in {1, 4, 16}, m = n / 2, nb = 256, both dtypes

Every shape runs in a process of its own under `timeout`; the tool stops at the first one that fails.  One JSON line
per shape on stdout; --json FILE collects them."""
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
    return [(256, n, p) for p in (1, 4, 16) for n in (8, 16, 32, 64, 128)]


def cpu_figure(Th, m, p, cplx):
    """milliseconds per problem of the CPU stand-in on the host copies Th [ncpu, p, n, n]"""
    import numpy as np
    import scipy.linalg.lapack as la

    ncpu, n = Th.shape[0], Th.shape[2]
    k, mk = n - m, m * (n - m)
    if p == 1:
        sel = np.zeros(n, dtype=np.int32)
        sel[:m] = 1
        work = dict(lwork=2 * mk) if cplx else dict(lwork=2 * mk, liwork=mk)
        t0 = time.perf_counter()
        for q in range(ncpu):
            out = (la.ztrsen if cplx else la.dtrsen)(sel, np.asfortranarray(Th[q, 0]), np.eye(n, dtype=Th.dtype, order="F"),
                                                     job="B", wantq=0, **work)
            assert out[-1] == 0
        return "trsen", 1e3 * (time.perf_counter() - t0) / ncpu
    if p * mk > 4096:
        return "none", None
    t0 = time.perf_counter()
    for q in range(ncpu):
        K = np.zeros((p * mk, p * mk), dtype=Th.dtype)
        for l in range(p):  # 'R': (a, b) = (l, l + 1)
            a, b = l, (l + 1) % p
            K[l * mk:(l + 1) * mk, b * mk:(b + 1) * mk] += np.kron(np.eye(k), Th[q, l, :m, :m])
            K[l * mk:(l + 1) * mk, a * mk:(a + 1) * mk] -= np.kron(Th[q, l, m:, m:].T, np.eye(m))
        rhs = np.concatenate([-Th[q, l, :m, m:].reshape(-1, order="F") for l in range(p)])
        np.linalg.solve(K, rhs)
    return "kronecker", 1e3 * (time.perf_counter() - t0) / ncpu


def run_one(nb, n, p, cplx, repeats, ncpu):
    import numpy as np
    import torch

    torch.cuda.init()
    import psd_amd

    eng = psd_amd.Engine(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9100 + n + 1000 * p)
    dt = torch.complex128 if cplx else torch.float64
    m = n // 2
    T = 0.1 * torch.triu(torch.randn((nb, p, n, n), dtype=dt, device="cuda", generator=gen), diagonal=1)
    d = torch.cat([torch.linspace(1.0, 1.5, m, dtype=torch.float64), torch.linspace(3.0, 3.5, n - m, dtype=torch.float64)])
    d = (d ** (1.0 / p)).to("cuda").expand(nb, p, n).clone().to(dt)
    if cplx:
        ph = torch.rand((nb, p, n), dtype=torch.float64, device="cuda", generator=gen) * (2 * np.pi)
        d = d * torch.exp(1j * ph)
    T = T + torch.diag_embed(d)
    if not cplx:
        for j in range(1, n - 1, 4):
            if j + 1 != m:  # (the split stays between two blocks)
                T[:, p - 1, j + 1, j] = -0.5
                T[:, p - 1, j, j + 1] = 0.7
                T[:, p - 1, j + 1, j + 1] = T[:, p - 1, j, j]
    Tc = T.transpose(2, 3).contiguous()  # the [nb][p][n][n] column-major blocks of the device entries
    Tv = Tc.transpose(2, 3)
    row = dict(nb=nb, n=n, p=p, m=m, complex=bool(cplx), repeats=repeats)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def solve():
        return eng.psylvester_batch(Tv, m, lr="R", schurindex=p)

    def subcond():
        return eng.subspacecond_batch(Tv, m, lr="R", schurindex=p)

    timed(solve), timed(subcond)  # warm-up
    ts, tc = [], []
    for _ in range(repeats):
        ms, X = timed(solve)
        ts.append(ms)
        st_s = eng.psylvester_batch_stats
        ms, (s, sep) = timed(subcond)
        tc.append(ms)
        st_c = eng.subspacecond_batch_stats
    assert Tv.data_ptr() == Tc.data_ptr()  # (the tensor was not copied on the way in)
    row["solve"] = dict(wall_ms=float(np.median(ts)), wall_ms_min=min(ts), wall_ms_max=max(ts), ms_kernels=st_s.ms_kernels,
                        nsolve=int(st_s.nsolve), ngroups=int(st_s.ngroups))
    row["subcond"] = dict(wall_ms=float(np.median(tc)), wall_ms_min=min(tc), wall_ms_max=max(tc), ms_kernels=st_c.ms_kernels,
                          nsolve=int(st_c.nsolve), nnorms=int(st_c.nnorms), nest_steps=int(st_c.nest_steps),
                          nest_iter=int(st_c.nest_iter), ngroups=int(st_c.ngroups))
    row["s_min"], row["sep_min"], row["x_max"] = float(s.min()), float(sep.min()), float(X.abs().max())
    kind, ms = cpu_figure(Tv[:ncpu].cpu().numpy(), m, p, cplx)
    row["cpu"] = dict(kind=kind, ms_per_problem=ms, problems=ncpu, ms_scaled_to_nb=None if ms is None else ms * nb)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=None, help="nb x n x p, comma separated (default: the grid above)")
    ap.add_argument("--complex", action="store_true", dest="cplx", help="ComplexF64 only (default: both dtypes)")
    ap.add_argument("--real", action="store_true", help="Float64 only")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu", type=int, default=4, help="problems the CPU figure is taken from")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per shape")
    ap.add_argument("--json", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        run_one(*parse_shapes(args.one)[0], args.cplx, args.repeats, args.cpu)
        return 0
    shapes = parse_shapes(args.shapes) if args.shapes else default_shapes()
    kinds = [True] if args.cplx else [False] if args.real else [False, True]
    rows, want = [], len(shapes) * len(kinds)
    for cplx in kinds:
        for s in shapes:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one",
                   "%dx%dx%d" % s, "--repeats", str(args.repeats), "--cpu", str(args.cpu)] + (["--complex"] if cplx else [])
            pr = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(pr.stdout)
            sys.stdout.flush()
            if pr.returncode != 0:  # a failure, a fault or a time limit: nothing more is started on the device
                print(json.dumps(dict(shape=s, complex=cplx, failed=pr.returncode)), flush=True)
                if args.json:
                    with open(args.json, "w") as fh:
                        json.dump(dict(rows=rows), fh, indent=1)
                return 1
            rows += [json.loads(ln) for ln in pr.stdout.splitlines() if ln.startswith("{")]
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(dict(rows=rows), fh, indent=1)
    return 0 if len(rows) == want else 1


if __name__ == "__main__":
    sys.exit(main())
