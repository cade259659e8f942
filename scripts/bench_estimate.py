#!/usr/bin/env python3
"""The ESV2007 estimator (hdd_swipdg_estimate) measured at the size of BASELINE configuration C2: the SPE10 P1 mesh of
3200 x 640 Kuhn squares (4.1 M triangles, 12.3 M DoFs), kappa = 1, the checkerboard permeability as isotropic
per-element tensor, the ESV2007 force, a random vector.  bench.py is not involved.

Variants, alternating over --rounds rounds inside one (fresh) process after a warm-up: the sums alone (what a greedy
loop asks for), with the local arrays and the fluxes written, and the sums without a force (no residual term: what
the 41 force evaluations per element of the other two cost).  A call ends in its own stream synchronise, so the
host clock around --reps calls is the time a caller sees; HIP events around the same calls give the device side.  The
median over the rounds is reported with the minimum and the maximum.

Algorithmic bytes (what must cross HBM once; the neighbours' data and the shared vertex rows are re-reads):
  per element  12 elem_vertices + 12 neighbours + 4 face_info + 24 u + 8 n_per (per-element coefficient rows)
               + 12 patch DoFs + 24 u again (the vertex kernel)            [+ 32 local + 24 flux when written]
  per vertex   16 coordinates + 8 + 8 Oswald value written and read + 8 patch pointer + 1 boundary flag
--blocks PX,PY [PX,PY ...] adds the OS2014 block call (hdd_block_swipdg_estimate), one segment per subdomain, on the same
mesh partitioned into PX x PY subdomains (subdomain-major numbering), beside the ESV2007 call on that very mesh in the
same alternating rounds, with and without the force; one result per partitioning under "blocks", with the time of the
host table build (Estimator.set_segments) and the ratios block / ESV2007.
--host also times the path a user had before: the device-to-host copy of u and the numpy restatement
(tests/estimator_ref.py) on the same mesh, once.
Prints one JSON line; --out DIR also writes it to DIR/bench_estimate.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dune-hdd_amd", "python"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=3200, help="Kuhn squares in x (ny = nx / 5)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host", action="store_true", help="also time the host path (copy of u + numpy restatement)")
    ap.add_argument("--blocks", nargs="*", default=[], metavar="PX,PY", help="also measure the block call on PX x PY subdomains")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import hdd_amd as H
    torch.cuda.set_device(0)
    ctx = H.Context(0)
    res = measure(args, H, torch, ctx, 1, 1, False)
    if args.blocks:
        res["blocks"] = {}
    for spec in args.blocks:
        px, py = (int(v) for v in spec.split(","))
        res["blocks"]["%dx%d" % (px, py)] = measure(args, H, torch, ctx, px, py, True)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_estimate.json"), "w") as f:
            f.write(line + "\n")
    return 0


def measure(args, H, torch, ctx, px, py, blocks):
    """the variants on the mesh partitioned into px x py subdomains; blocks: the block call beside the ESV2007 call"""
    nx, ny = args.nx, max(args.nx // 5, 1)
    grid = H.Grid.structured(H.SIMPLEX, nx, ny, (0, 0), (5, 1), px=px, py=py)
    loc = grid.local()
    k = loc.checkerboard((0, 0), (5, 1), 100, 20, 10.0 ** np.random.default_rng(10).uniform(-3, 3, 2000))
    dm = H.DeviceMesh(loc)
    t0 = time.perf_counter()
    est = H.Estimator(ctx, loc)
    create_s = time.perf_counter() - t0
    kappas = [H.scalar_fn(H.FN_CONST, 1.0)]
    tensor = H.tensor_fn(H.TENSOR_ISO_PER_ELEM, per_elem=torch.from_numpy(k).cuda())
    force = H.esv2007_force()
    ne, nv = loc.n_local, int(dm.vertex_coords.shape[0])
    u = torch.randn(3 * ne, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    base = ne * (12 + 12 + 4 + 24 + 8 + 12 + 24) + nv * (16 + 8 + 8 + 8 + 1)
    variants = {
        "sums": dict(kw=dict(force=force), bytes=base),
        "sums_local_flux": dict(kw=dict(force=force, local=True, flux=True), bytes=base + ne * (32 + 24)),
        "sums_no_force": dict(kw=dict(), bytes=base),
    }
    set_segments_s = None
    if blocks:
        t0 = time.perf_counter()
        est.set_segments(subdomains=(0, px * py))
        set_segments_s = time.perf_counter() - t0
        del variants["sums_local_flux"]
        # the block call: no h_T, two more kappa roles, 4 partials per chunk and 4 values per segment in place of 4 per 256
        variants["blocks"] = dict(kw=dict(force=force), bytes=base, call=H.estimate_blocks)
        variants["blocks_no_force"] = dict(kw=dict(), bytes=base, call=H.estimate_blocks)
    for v in variants.values():
        v["wall_ms"], v["dev_ms"] = [], []
    sums, kernels = {}, {}
    for r in range(args.rounds):
        for key, v in variants.items():
            call = v.get("call", H.estimate)
            for _ in range(args.warmup if r == 0 else 1):
                e = call(ctx, est, dm, kappas, tensor, u, **v["kw"])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.reps):
                e = call(ctx, est, dm, kappas, tensor, u, **v["kw"])
            e1.record()
            torch.cuda.synchronize()
            v["wall_ms"].append((time.perf_counter() - t0) * 1e3 / args.reps)
            v["dev_ms"].append(e0.elapsed_time(e1) / args.reps)
            if "force" in v["kw"]:
                if key in sums and not np.array_equal(sums[key], e.sums):
                    raise SystemExit("sums differ between calls: %r %r" % (sums[key], e.sums))
                sums[key] = e.sums.copy()
                kernels[key] = H.last_estimate_kernels()
    res = dict(config="c2_spe10_p1_%dx%d" % (nx, ny), n_elements=ne, n_vertices=nv, kernels=kernels["sums"],
               rounds=args.rounds, reps=args.reps, estimator_create_s=create_s, sums=[float(s) for s in sums["sums"]],
               variants={})
    if blocks:
        res.update(subdomains=[px, py], set_segments_s=set_segments_s, block_kernels=kernels["blocks"],
                   block_sums=[float(s) for s in sums["blocks"]])
    for key, v in variants.items():
        ms = float(np.median(v["wall_ms"]))
        res["variants"][key] = dict(ms=ms, ms_min=float(min(v["wall_ms"])), ms_max=float(max(v["wall_ms"])),
                                    device_ms=float(np.median(v["dev_ms"])), alg_bytes=v["bytes"],
                                    alg_TBps=v["bytes"] / ms / 1e9)
    if blocks:
        res["ratio_blocks_over_sums"] = res["variants"]["blocks"]["ms"] / res["variants"]["sums"]["ms"]
        res["ratio_blocks_over_sums_no_force"] = (res["variants"]["blocks_no_force"]["ms"] /
                                                  res["variants"]["sums_no_force"]["ms"])
        if sums["blocks"][0] <= 0 or abs(sums["blocks"][0] - sums["sums"][0]) > 1e-12 * sums["sums"][0]:
            raise SystemExit("sum of eta_NC^2 of the block call is not the ESV2007 call's")
    if args.host and not blocks:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import estimator_ref as R
        ev, xy = loc.vertices()
        t0 = time.perf_counter()
        uh = u.cpu().numpy()
        copy_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref = R.estimate(xy, np.ascontiguousarray(ev.T), uh, kappa=np.ones((1, ne)), tensor=np.stack([k, np.zeros(ne), k]),
                         force=R.esv2007_force())
        host_s = time.perf_counter() - t0
        res["host"] = dict(copy_u_ms=copy_s * 1e3, estimator_ref_ms=host_s * 1e3,
                           rel_diff_of_sums=[float(abs(a - b) / abs(b)) for a, b in zip(sums["sums"], ref["sums"])])
    return res


if __name__ == "__main__":
    sys.exit(main())
