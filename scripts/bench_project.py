#!/usr/bin/env python3
"""Reduced-basis projection (hdd_operator_project) measured at the sizes of the BASELINE configurations against the
route there was before it: the loop of 8 x 8 hdd_operator_apply2 chunks per component.  bench.py is not involved.

  c2  SPE10 P1, 3200 x 640 Kuhn triangles (12.3 M rows, 147 M nnz)
  c3  OS2014, 1024^2 Kuhn triangles, two components
  c4  SPE10-like Q1, 3520 x 1200 quadrilaterals (16.9 M rows, 338 M nnz)

Variants per configuration: G_q = V^T A_q U for every component with N = 8 / 32 / 64 vectors a side on the tile
kernel and on the CSR kernel, and the Gramian V^T M V of the L2 product (volume pattern, CSR kernel, N = 32); next to
each the apply2 loop on the same operands, timed in the same process.  Timing: HIP events around `--reps` calls
(`--loop-reps` of the loop) after a warm-up, the variants ALTERNATING over `--rounds` rounds inside one process (so
clock and thermal drift hit all of them alike); the median over the rounds is reported with the minimum and maximum.
Every configuration runs in a child process of its own under a time limit (--timeout), and inside it a variant that
has used more than --variant-timeout seconds is dropped from the later rounds and reported as such.

Algorithmic bytes (what must cross HBM once): n_comp nnz 8 + (n_v rows + n_u cols) 8.
Prints one JSON line per configuration (per variant: ms, alg_bytes, alg_TBps, and for the projections loop_ms and
ratio_to_loop = loop_ms / ms); --out DIR also writes them to DIR/bench_project.jsonl."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dune-hdd_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_apply import build  # noqa: E402  (the configurations)


def run_config(args):
    import torch
    torch.cuda.set_device(0)
    H, ctx, loc, dm, dp, vals, label = build(args.config, args.n)
    n_rows, n_cols, nnz = dp.t.n_rows, dp.t.n_cols, dp.nnz
    sizes = [int(s) for s in args.sizes.split(",")]
    gen = torch.Generator(device="cuda").manual_seed(5)
    nmax = max(sizes + [32])
    V = torch.randn((nmax, n_rows), dtype=torch.float64, device="cuda", generator=gen)
    U = torch.randn((nmax, n_cols), dtype=torch.float64, device="cuda", generator=gen)

    def loop(pattern, arrays, mesh, n):
        """the route before hdd_operator_project: 8 x 8 apply2 chunks per component"""
        out = torch.empty((len(arrays), n, n), dtype=torch.float64, device="cuda")
        for q, a in enumerate(arrays):
            for i in range(0, n, H.MAX_VEC):
                for j in range(0, n, H.MAX_VEC):
                    out[q, i:i + H.MAX_VEC, j:j + H.MAX_VEC] = H.apply2(ctx, pattern, [a], V[i:min(i + H.MAX_VEC, n)],
                                                                        U[j:min(j + H.MAX_VEC, n)], dmesh=mesh)
        return out

    variants = {}

    def add(key, fn, reps, **info):
        variants[key] = dict(fn=fn, reps=reps, ms=[], wall=0.0, dropped=False, **info)

    def pair(key, pattern, arrays, mesh, n, p_nnz):
        nbytes = 8 * p_nnz * len(arrays) + 8 * n * (n_rows + n_cols)
        add(key, lambda: H.project(ctx, pattern, arrays, V[:n], U[:n], dmesh=mesh), args.reps, alg_bytes=nbytes, n=n,
            n_comp=len(arrays))
        add(key + "_apply2_loop", lambda: loop(pattern, arrays, mesh, n), args.loop_reps, alg_bytes=nbytes, n=n, n_comp=len(arrays))

    for tile in (True, False):
        for n in sizes:
            pair("%s_N%d" % ("tile" if tile else "csr", n), dp, vals, dm if tile else None, n, nnz)
    notes = []
    if not args.no_l2:
        dpv = H.DevicePattern(loc, volume=True)
        m = H.product(ctx, dm, H.PRODUCT_L2, dpv)
        torch.cuda.synchronize()
        pair("l2_gramian_N32", dpv, [m], None, 32, dpv.nnz)
    kernels = {}
    for r in range(args.rounds):
        for key, v in variants.items():
            if v["dropped"]:
                continue
            t0 = time.perf_counter()
            for _ in range(args.warmup if r == 0 else 1):
                v["fn"]()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(v["reps"]):
                v["fn"]()
            e1.record()
            torch.cuda.synchronize()
            v["ms"].append(e0.elapsed_time(e1) / v["reps"])
            v["wall"] += time.perf_counter() - t0
            kernels[key] = H.last_apply_kernel()
            if v["wall"] > args.variant_timeout:
                v["dropped"] = True
    res = dict(config=label, n_rows=n_rows, nnz=nnz, n_comp=len(vals), rounds=args.rounds, reps=args.reps,
               loop_reps=args.loop_reps, notes=notes, kernels=kernels, variants={})
    for key, v in variants.items():
        ms = float(np.median(v["ms"]))
        res["variants"][key] = dict(ms=ms, ms_min=float(min(v["ms"])), ms_max=float(max(v["ms"])), alg_bytes=v["alg_bytes"],
                                    alg_TBps=v["alg_bytes"] / ms / 1e9, n=v["n"], n_comp=v["n_comp"], rounds_timed=len(v["ms"]),
                                    dropped=v["dropped"])
    for key, v in res["variants"].items():
        lp = res["variants"].get(key + "_apply2_loop")
        if lp:
            v["loop_ms"] = lp["ms"]
            v["ratio_to_loop"] = lp["ms"] / v["ms"]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["c2", "c3", "c4"])
    ap.add_argument("--config", default=None, help="(child) run this one configuration in this process")
    ap.add_argument("--n", type=int, default=0, help="nx of the mesh (default: the configuration's size)")
    ap.add_argument("--sizes", default="8,32,64", help="basis sizes N (vectors a side)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-reps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-l2", action="store_true", help="skip the L2 Gramian (its volume pattern is built on the host)")
    ap.add_argument("--timeout", type=float, default=420.0, help="seconds per configuration (child process)")
    ap.add_argument("--variant-timeout", type=float, default=40.0, help="seconds per variant inside a configuration")
    ap.add_argument("--out", default=None, help="directory for bench_project.jsonl")
    args = ap.parse_args()
    if args.config:
        run_config(args)
        return 0
    lines = []
    for c in args.configs:
        cmd = [sys.executable, os.path.abspath(__file__), "--config", c, "--n", str(args.n), "--sizes", args.sizes,
               "--rounds", str(args.rounds), "--reps", str(args.reps), "--loop-reps", str(args.loop_reps),
               "--warmup", str(args.warmup), "--variant-timeout", str(args.variant_timeout)] + (["--no-l2"] if args.no_l2 else [])
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(config=c, error="timeout after %g s" % args.timeout)), flush=True)
            return 1   # a hung configuration: nothing more is started on the device
        if p.returncode != 0:
            print(json.dumps(dict(config=c, error="exit %d" % p.returncode, stderr=p.stderr[-2000:])), flush=True)
            return 1
        for ln in p.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(ln)
                print(ln, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_project.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
