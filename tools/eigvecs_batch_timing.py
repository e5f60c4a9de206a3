#!/usr/bin/env python3
"""Timing of Engine.eigvecs_batch on the MI355X (profiles/batch/README.md).

For every shape nb x n x p: random factors A_j = I + 0.5 G_j / sqrt(n) are made on the device, decomposed by the
device-resident pschur_batch_, and with T, Z left on the device all eigenvectors are computed
  batch   by one Engine.eigvecs_batch call (psd_d_eigvecs_batch_dev), and
  loop    by Engine.eigvecs_dev problem by problem on the same engine: the code that existed before, the baseline.
The second of two runs of each is reported: wall time around the call(s) with the device idle before and after, the
device times and the launches of the stats, and the largest difference between the two results.

  (default)  n in {8, 16, 32, 64, 128}, p in {2, 4, 16}, nb in {32, 1024}
  --sweep    n across the cap PSD_BEV_NMAX at nb = 64, p = 4, on the diagnostic library with the cap lifted
             (PSD_BEV_NMAX in the environment), so that every order takes the batched kernels
  --complex  ComplexF64 factors: zpschur_batch_, then Engine.zeigvecs_batch (psd_z_eigvecs_batch_dev) against the loop
             of Engine.eigvecs_dev on the complex T, Z
  --signed   signed ComplexF64 problems (alternating signature): zgpschur_batch_, then Engine.zgeigvecs_batch
             (psd_z_geigvecs_batch_dev) against the loop of Engine.geigvecs_dev on the same device tensors; nb = 256,
             n in {8, 16, 32, 64}, p in {4, 16}; one warm-up, then the median of five alternating runs of each
  --signed-real  the same for signed Float64 problems: dgpschur_batch_, then Engine.dgeigvecs_batch
             (psd_d_geigvecs_batch_dev) against the loop of Engine.geigvecs_dev on the real T, Z; n up to 128
  --left     the left eigenvectors beside the right ones at the shapes of the default grid: Engine.eigvecs_batch (with
             --complex: zeigvecs_batch) with side="L" (psd_?_leigvecs_batch_dev) against side="R" on the same device
             tensors, and Engine.eigcond_batch (both calls and psd_bev_cond); one warm-up, then the median of five
             alternating runs of each.  A record of what the flipped copies and the column reversal cost, not a gate

Every shape runs in a process of its own under `timeout`; the tool stops at the first one that fails.  One JSON line per
shape on stdout; --json FILE collects them."""
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
    return [(nb, n, p) for nb in (32, 1024) for n in (8, 16, 32, 64, 128) for p in (2, 4, 16)]


def run_one(nb, n, p, lr, sweep, cplx=False):
    import numpy as np
    import torch

    torch.cuda.init()
    import psd_amd

    if sweep:
        os.environ["PSD_BEV_NMAX"] = "2048"
        eng = psd_amd.Engine(0, libpath=psd_amd.DIAG_LIB_PATH)
    else:
        eng = psd_amd.Engine(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9000 + n + 1000 * p)
    dt = torch.complex128 if cplx else torch.float64  # (complex: real and imaginary parts N(0, 1/2) each)
    A = torch.eye(n, dtype=dt, device="cuda") + 0.5 * torch.randn(
        (nb, p, n, n), dtype=dt, device="cuda", generator=gen) / np.sqrt(n)
    infos = []
    T, Z, values, _ = (eng.zpschur_batch_ if cplx else eng.pschur_batch_)(A, lr, infos_out=infos)
    batched = eng.zeigvecs_batch if cplx else eng.eigvecs_batch
    si = p if lr == "L" else 1
    select = np.ones((nb, n), dtype=bool)
    select[[q for q in range(nb) if infos[q] != 0]] = False  # (a problem that did not converge is skipped)
    Tc, Zc = T.transpose(2, 3), Z.transpose(2, 3)  # the [nb][p][n][n] column-major blocks, contiguous
    assert Tc.is_contiguous() and Zc.is_contiguous()
    row = dict(nb=nb, n=n, p=p, lr=lr, nfailed=int(sum(1 for i in infos if i != 0)), sweep=bool(sweep), complex=bool(cplx))
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        V, nvec = batched(T, Z, values, select, lr=lr, schurindex=si)
        torch.cuda.synchronize()
        st = eng.eigvecs_batch_stats
        row["batch"] = dict(wall_ms=1e3 * (time.perf_counter() - t0), ms_solve=st.ms_solve,
                            ms_backtransform=st.ms_backtransform, nlaunch=int(st.nlaunch), ngroups=int(st.ngroups),
                            nvec=int(st.nvec_total))
    for _ in range(2):
        torch.cuda.synchronize()
        ms, singles = 0.0, []
        t0 = time.perf_counter()
        for q in range(nb):
            if not select[q, 0]:
                singles.append(None)
                continue
            singles.append(eng.eigvecs_dev(Tc[q], Zc[q], values[q], select[q], lr=lr, schurindex=si))
            ms += eng.eigvecs_stats.ms_kernels
        torch.cuda.synchronize()
        row["loop"] = dict(wall_ms=1e3 * (time.perf_counter() - t0), ms_kernels=ms)
    diff = 0.0
    for q in range(0, nb, max(1, nb // 8)):
        if singles[q] is not None:
            for l in range(p):
                d = (V[q, l][:, :nvec[q]] - singles[q][l]).abs().max().item()
                diff = max(diff, d if d == d else 0.0)  # (NaN columns of zero eigenvalues aside)
    row["max_abs_diff"] = diff
    row["wall_ratio"] = row["loop"]["wall_ms"] / row["batch"]["wall_ms"]
    print(json.dumps(row), flush=True)


def run_left(nb, n, p, lr, cplx=False, repeats=5):
    """--left: side="R", side="L" and eigcond_batch on the output of the device-resident [z]pschur_batch_."""
    import numpy as np
    import torch

    torch.cuda.init()
    import psd_amd

    eng = psd_amd.Engine(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9000 + n + 1000 * p)
    dt = torch.complex128 if cplx else torch.float64
    A = torch.eye(n, dtype=dt, device="cuda") + 0.5 * torch.randn(
        (nb, p, n, n), dtype=dt, device="cuda", generator=gen) / np.sqrt(n)
    infos = []
    T, Z, values, _ = (eng.zpschur_batch_ if cplx else eng.pschur_batch_)(A, lr, infos_out=infos)
    batched = eng.zeigvecs_batch if cplx else eng.eigvecs_batch
    si = p if lr == "L" else 1
    select = np.ones((nb, n), dtype=bool)
    select[[q for q in range(nb) if infos[q] != 0]] = False  # (a problem that did not converge is skipped)
    row = dict(nb=nb, n=n, p=p, lr=lr, nfailed=int(sum(1 for i in infos if i != 0)), left=True, complex=bool(cplx),
               repeats=repeats)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        st = eng.eigvecs_batch_stats
        return 1e3 * (time.perf_counter() - t0), out, dict(ms_solve=st.ms_solve, ms_backtransform=st.ms_backtransform,
                                                          nlaunch=int(st.nlaunch), ngroups=int(st.ngroups))

    calls = dict(right=lambda: batched(T, Z, values, select, lr=lr, schurindex=si),
                 left=lambda: batched(T, Z, values, select, lr=lr, schurindex=si, side="L"),
                 cond=lambda: eng.eigcond_batch(T, Z, values, select, lr=lr, schurindex=si))
    for call in calls.values():
        timed(call)  # warm-up
    ms = {k: [] for k in calls}
    for _ in range(repeats):
        for k, call in calls.items():
            t, out, st = timed(call)
            ms[k].append(t)
            row[k] = st
            if k == "cond":
                s, V, W, nvec = out
    for k in calls:
        row[k].update(wall_ms=float(np.median(ms[k])), wall_ms_min=min(ms[k]), wall_ms_max=max(ms[k]))
    # w_l' v_l over l: the largest relative spread over every eighth problem (NaN columns of zero eigenvalues aside)
    spread = 0.0
    for q in range(0, nb, max(1, nb // 8)):
        d = (W[q, :, :, :nvec[q]].conj() * V[q, :, :, :nvec[q]]).sum(dim=1)
        r = ((d - d[0]).abs() / d[0].abs()).max().item() if nvec[q] else 0.0
        spread = max(spread, r if r == r else 0.0)
    row["inner_product_spread"] = spread
    sv = s[s > 0]
    row["s_min"] = float(sv.min()) if sv.size else None
    row["left_over_right"] = row["left"]["wall_ms"] / row["right"]["wall_ms"]
    print(json.dumps(row), flush=True)


def signed_shapes(real=False):
    return [(256, n, p) for n in (8, 16, 32, 64) + ((128,) if real else ()) for p in (4, 16)]


def run_signed(nb, n, p, lr, repeats=5, real=False):
    """--signed: zgpschur_batch_ with the alternating signature, then Engine.zgeigvecs_batch against the loop of
    Engine.geigvecs_dev on the same device tensors; --signed-real (`real`): dgpschur_batch_ and Engine.dgeigvecs_batch on
    Float64 factors.  One warm-up of each, then `repeats` timed runs of each, alternating; the medians and the extremes
    are reported."""
    import numpy as np
    import torch

    torch.cuda.init()
    import psd_amd

    eng = psd_amd.Engine(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9000 + n + 1000 * p)
    dt = torch.float64 if real else torch.complex128
    A = torch.eye(n, dtype=dt, device="cuda") + 0.5 * torch.randn(
        (nb, p, n, n), dtype=dt, device="cuda", generator=gen) / np.sqrt(n)
    S = [l % 2 == 0 for l in range(p)]
    infos = []
    T, Z, values, _ = (eng.dgpschur_batch_ if real else eng.zgpschur_batch_)(A, S, lr, infos_out=infos)
    batched = eng.dgeigvecs_batch if real else eng.zgeigvecs_batch
    si = p if lr == "L" else 1
    select = np.ones((nb, n), dtype=bool)
    select[[q for q in range(nb) if infos[q] != 0]] = False  # (a problem that did not converge is skipped)
    Tc, Zc = T.transpose(2, 3), Z.transpose(2, 3)  # the [nb][p][n][n] column-major blocks, contiguous
    assert Tc.is_contiguous() and Zc.is_contiguous()
    row = dict(nb=nb, n=n, p=p, lr=lr, nfailed=int(sum(1 for i in infos if i != 0)), signed=True, real=bool(real),
               repeats=repeats)

    def batch():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = batched(T, Z, select, S=S, lr=lr, schurindex=si)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def loop():
        torch.cuda.synchronize()
        singles = []
        t0 = time.perf_counter()
        for q in range(nb):
            singles.append(eng.geigvecs_dev(Tc[q], Zc[q], select[q], lr, si, S=S) if select[q, 0] else None)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), singles

    batch(), loop()  # warm-up
    tb, tl = [], []
    for _ in range(repeats):
        ms, (V, a, nvec) = batch()
        tb.append(ms)
        st = eng.eigvecs_batch_stats
        ms, singles = loop()
        tl.append(ms)
    row["batch"] = dict(wall_ms=float(np.median(tb)), wall_ms_min=min(tb), wall_ms_max=max(tb), ms_solve=st.ms_solve,
                        ms_backtransform=st.ms_backtransform, nlaunch=int(st.nlaunch), ngroups=int(st.ngroups),
                        nvec=int(st.nvec_total), nzero=int(st.nzero), nperturbed=int(st.nperturbed),
                        nrescaled=int(st.nrescaled))
    row["loop"] = dict(wall_ms=float(np.median(tl)), wall_ms_min=min(tl), wall_ms_max=max(tl))
    diff = adiff = 0.0
    for q in range(0, nb, max(1, nb // 8)):
        if singles[q] is not None:
            Vs, aq = singles[q]
            for l in range(p):
                diff = max(diff, (V[q, l][:, :nvec[q]] - Vs[l]).abs().max().item())
            adiff = max(adiff, float(np.abs(a[q][:, :nvec[q]] - aq).max()))
    row["max_abs_diff"] = diff
    row["max_abs_diff_a"] = adiff
    row["wall_ratio"] = row["loop"]["wall_ms"] / row["batch"]["wall_ms"]
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=None, help="nb x n x p, comma separated (default: the grid above)")
    ap.add_argument("--lr", default="R")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-orders", default="64,96,128,160,192,256")
    ap.add_argument("--complex", action="store_true", dest="cplx")
    ap.add_argument("--signed", action="store_true")
    ap.add_argument("--signed-real", action="store_true", dest="signed_real")
    ap.add_argument("--left", action="store_true")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per shape")
    ap.add_argument("--json", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one and (args.signed or args.signed_real):
        run_signed(*parse_shapes(args.one)[0], args.lr, real=args.signed_real)
        return 0
    if args.one and args.left:
        run_left(*parse_shapes(args.one)[0], args.lr, args.cplx)
        return 0
    if args.one:
        run_one(*parse_shapes(args.one)[0], args.lr, args.sweep, args.cplx)
        return 0
    if args.shapes:
        shapes = parse_shapes(args.shapes)
    elif args.signed or args.signed_real:
        shapes = signed_shapes(args.signed_real)
    elif args.sweep:
        shapes = [(64, int(x), 4) for x in args.sweep_orders.split(",") if x]
    else:
        shapes = default_shapes()
    rows = []
    for s in shapes:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one",
               "%dx%dx%d" % s, "--lr", args.lr] + (["--sweep"] if args.sweep else []) + (
                   ["--complex"] if args.cplx else []) + (["--signed"] if args.signed else []) + (
                       ["--signed-real"] if args.signed_real else []) + (["--left"] if args.left else [])
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
