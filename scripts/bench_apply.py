#!/usr/bin/env python3
"""Operator application (hdd_operator_apply / hdd_operator_apply2) measured at the sizes of the BASELINE
configurations.  bench.py is not involved.

  c2  SPE10 P1, 3200 x 640 Kuhn triangles (12.3 M rows, 147 M nnz)
  c3  OS2014, 1024^2 Kuhn triangles, two components: the theta-fused apply of A_aff + mu A_1 against
      hdd_affine_lincomb (A(mu) written to HBM) followed by a single-component apply
  c4  SPE10-like Q1, 3520 x 1200 quadrilaterals (16.9 M rows, 338 M nnz)

Variants per configuration: the tile kernel and the CSR kernel with 1 and 4 vectors, apply2 (4 x 4), and as the
outside baseline torch.sparse_csr_tensor(...) @ x on the same arrays (float64; logged and skipped when this torch
build refuses it).  Timing: HIP events around `--reps` calls after a warm-up, the variants ALTERNATING over `--rounds`
rounds inside one process (so clock and thermal drift hit all of them alike); the median over the rounds is
reported with the minimum and maximum.  Every configuration runs in a child process of its own under a time limit
(--timeout), and inside it a variant that has used more than --variant-timeout seconds is dropped from the later
rounds and reported as such.

Algorithmic bytes (what must cross HBM once):
  tile kernel   8 nnz n_comp + 8 n_vec (n_rows + n_cols) + 4 nf ne       (values, x and y, the neighbour ids)
  CSR kernel    the same + 4 nnz + 8 n_rows                              (col, row_ptr)
Prints one JSON line per configuration; --out DIR also writes them to DIR/bench_apply.jsonl."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dune-hdd_amd", "python"))


def build(name, n):
    import torch
    import hdd_amd as H
    ctx = H.Context(0)
    if name == "c3":
        n = n or 1024
        grid = H.Grid.structured(H.SIMPLEX, n, n, (-1, -1), (1, 1))
        kx, ky = 4 * math.pi, 2 * math.pi
        fns = [H.scalar_fn(H.FN_SINUSOID, 1.0, 0.75, kx, ky, order=3),
               H.scalar_fn(H.FN_SINUSOID, 0.0, -0.75, kx, ky, order=3)]
        loc = grid.local()
        ten = H.tensor_fn()
        label = "c3_os2014_kuhn%dx%d" % (n, n)
    else:
        et = H.SIMPLEX if name == "c2" else H.CUBE
        nx = n or (3200 if name == "c2" else 3520)
        ny = nx // 5 if name == "c2" else nx * 1200 // 3520
        grid = H.Grid.structured(et, nx, ny, (0, 0), (5, 1))
        loc = grid.local()
        k = loc.checkerboard((0, 0), (5, 1), 100, 20, 10.0 ** np.random.default_rng(10).uniform(-3, 3, 2000))
        fns = [H.scalar_fn(H.FN_CONST, 1.0)]
        ten = H.tensor_fn(H.TENSOR_ISO_PER_ELEM, per_elem=torch.from_numpy(k).cuda())
        label = "%s_spe10_%s_%dx%d" % (name, "p1" if name == "c2" else "q1", nx, ny)
    dm = H.DeviceMesh(loc)
    dp = H.DevicePattern(loc, ctx=ctx, dmesh=dm, on_device=True)
    vals = H.assemble(ctx, dm, dp, fns, ten)
    torch.cuda.synchronize()
    return H, ctx, loc, dm, dp, vals, label


def run_config(args):
    import torch
    torch.cuda.set_device(0)
    H, ctx, loc, dm, dp, vals, label = build(args.config, args.n)
    n_rows, n_cols, nnz, ne, nf = dp.t.n_rows, dp.t.n_cols, dp.nnz, loc.n_own, loc.nf
    gen = torch.Generator(device="cuda").manual_seed(5)
    X = torch.randn((4, n_cols), dtype=torch.float64, device="cuda", generator=gen)
    V = torch.randn((4, n_rows), dtype=torch.float64, device="cuda", generator=gen)
    Y = torch.empty((4, n_rows), dtype=torch.float64, device="cuda")
    theta = [1.0, 0.3][:len(vals)]

    def bytes_of(n_vec, n_comp, tile):
        b = 8 * nnz * n_comp + 8 * n_vec * (n_rows + n_cols) + 4 * nf * ne
        return b if tile else b + 4 * nnz + 8 * n_rows

    variants = {}

    def add(key, fn, nbytes, **info):
        variants[key] = dict(fn=fn, bytes=nbytes, ms=[], wall=0.0, dropped=False, **info)

    nc = len(vals)
    for tile in (True, False):
        for nv in (1, 4):
            add("%s_nvec%d" % ("tile" if tile else "csr", nv),
                (lambda tile=tile, nv=nv: H.apply(ctx, dp, vals, X[:nv], theta=theta, dmesh=dm if tile else None,
                                                  out=Y[:nv])), bytes_of(nv, nc, tile), n_vec=nv, n_comp=nc)
    add("apply2_4x4_tile", lambda: H.apply2(ctx, dp, vals, V, X, theta=theta, dmesh=dm),
        bytes_of(4, nc, True) + 8 * 8 * n_rows, n_vec=4, n_comp=nc)
    if nc > 1:   # A(mu) written out, then applied as one component
        A = torch.empty((1, nnz + (nnz & 1)), dtype=torch.float64, device="cuda")
        th = np.array([theta])

        def lincomb_then_apply():
            H.affine_lincomb(ctx, vals, th, out=A)
            H.apply(ctx, dp, [A[0, :nnz]], X[:1], dmesh=dm, out=Y[:1])
        add("lincomb_then_tile_nvec1", lincomb_then_apply, 8 * nnz * (nc + 1) + bytes_of(1, 1, True), n_vec=1, n_comp=nc)
    notes = []
    try:   # the outside baseline: torch's CSR product on the same arrays (A(theta) written out first)
        a = vals[0] if nc == 1 else sum(t * v for t, v in zip(theta, vals))
        S = torch.sparse_csr_tensor(dp.row_ptr, dp.col.to(torch.int64), a, size=(n_rows, n_cols))
        XT = {nv: X[:nv].t().contiguous() for nv in (1, 4)}
        S @ XT[1]
        torch.cuda.synchronize()
        # torch reads 8-byte column indices here (it wants crow and col of one dtype): 16 B per nonzero
        for nv in (1, 4):
            add("torch_csr_nvec%d" % nv, (lambda nv=nv: S @ XT[nv]),
                8 * nnz + 8 * nnz + 8 * nv * (n_rows + n_cols) + 8 * n_rows, n_vec=nv, n_comp=1)
    except Exception as e:   # noqa: BLE001 -- any refusal is logged, the CSR kernel stays the baseline
        notes.append("torch CSR f64 product refused: %s: %s" % (type(e).__name__, str(e)[:200]))
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
            for _ in range(args.reps):
                v["fn"]()
            e1.record()
            torch.cuda.synchronize()
            v["ms"].append(e0.elapsed_time(e1) / args.reps)
            v["wall"] += time.perf_counter() - t0
            if not key.startswith("torch") and not key.startswith("lincomb"):
                kernels[key] = H.last_apply_kernel()
            if v["wall"] > args.variant_timeout:
                v["dropped"] = True
    res = dict(config=label, n_rows=n_rows, nnz=nnz, n_comp=nc, rounds=args.rounds, reps=args.reps, notes=notes,
               kernels=kernels, variants={})
    for key, v in variants.items():
        ms = float(np.median(v["ms"]))
        res["variants"][key] = dict(ms=ms, ms_min=float(min(v["ms"])), ms_max=float(max(v["ms"])), alg_bytes=v["bytes"],
                                    alg_GBps=v["bytes"] / ms / 1e6, n_vec=v["n_vec"], n_comp=v["n_comp"],
                                    rounds_timed=len(v["ms"]), dropped=v["dropped"])
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["c2", "c3", "c4"])
    ap.add_argument("--config", default=None, help="(child) run this one configuration in this process")
    ap.add_argument("--n", type=int, default=0, help="nx of the mesh (default: the configuration's size)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per configuration (child process)")
    ap.add_argument("--variant-timeout", type=float, default=30.0, help="seconds per variant inside a configuration")
    ap.add_argument("--out", default=None, help="directory for bench_apply.jsonl")
    args = ap.parse_args()
    if args.config:
        run_config(args)
        return 0
    lines, rc = [], 0
    for c in args.configs:
        cmd = [sys.executable, os.path.abspath(__file__), "--config", c, "--n", str(args.n), "--rounds", str(args.rounds),
               "--reps", str(args.reps), "--warmup", str(args.warmup), "--variant-timeout", str(args.variant_timeout)]
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
        with open(os.path.join(args.out, "bench_apply.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
