#!/usr/bin/env python3
"""The device solve (hdd_operator_solve: block-Jacobi PCG on the theta-fused operator) measured at the sizes of the
BASELINE configurations c2 / c3 / c4 (scripts/bench_apply.py builds them).  bench.py is not involved.

A fixed iteration count (rtol = 0, max_iter = --iters, check_every = --iters: one look of the host) of
  fused      H.solve: three launches per iteration, alpha and beta stay on the device
  composed   the same iteration from what the library offered before the solver: H.apply + torch vector operations,
             torch.bmm with the same inverse diagonal blocks, and .item() for alpha and beta (two host
             synchronisations per iteration)
alternating over --rounds rounds in one process, HIP events around each, median [min, max].  The fused time per
iteration is (solve(iters) - solve(0 iterations)) / iters, so the setup (inverse blocks, initial residual, one look)
is reported separately.  Bytes model per iteration: 8 nnz n_comp + (13 + (BS + 1) / 2) vector passes of 8 n bytes
(symmetric packed D^-1).  --converge also records the iterations to rtol = 1e-8 (a number, not a target).
Conjugate gradients need a positive definite matrix, which SWIPDG with the reference's penalties is not on every
configuration: the solve on the configuration's own matrix is recorded first ("reference_penalties"),
and when it breaks down the timing runs on the same mesh, pattern and coefficients with both penalties multiplied by
--sigma-scale (x4, x16, ... until 200 iterations pass): same bytes, same launches, a definite matrix.
--rhs N measures instead one hdd_operator_solve_batched call on N right-hand sides against N hdd_operator_solve calls
on the same columns (the unchanged single-solve path), alternating over the rounds in the same process, per iteration
as above; model per iteration 8 nnz n_comp + (BS + 1) / 2 8 n per group of four columns + 13 8 n per column.
--thetas N measures, by the same protocol, one hdd_operator_solve_multi call of N columns at N different thetas
against N hdd_operator_solve calls at those thetas: theta_j = (1, mu_j), mu_j spread over [0.3, 1], on the two
components of c3 (definite from mu = 0.3 up once it is at 0.3), a scalar theta_j in [1, 2] on the one component of c2 /
c4; model per iteration 8 nnz n_comp per group of four columns + (13 + (BS + 1) / 2) 8 n per column.
--blocks PX,PY measures, by the same protocol, one hdd_operator_solve_blocks call over all PX x PY subdomains of the
configuration's mesh against the loop of hdd_operator_solve with block=(ss, ss) over the same subdomains (one
subdomain per call: the path before), every segment checked for bit equality with its single solve in every round;
for comparison the record carries the model of the single whole-matrix iteration (the tile kernel streams the
coupling blocks of a row block, too, and skips them) and its rate at both times.
Prints one JSON line per configuration; --out DIR also writes them to DIR/bench_solve.jsonl (--rhs:
DIR/bench_solve_batched.jsonl, --thetas: DIR/bench_solve_multi.jsonl, --blocks: appended to
DIR/bench_solve_blocks.jsonl, one run per partition)."""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dune-hdd_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def inverse_blocks(torch, loc, dm, dp, vals, theta):
    """the inverse diagonal blocks [ne, nb, nb] with torch, from elem_ptr and the neighbours (as the tile path does)"""
    nb, ne = loc.nb, loc.n_own
    nbrs = dm.neighbors.reshape(loc.nf, -1)[:, :ne].to(torch.int64)
    e = torch.arange(ne, device="cuda")
    nint = (nbrs >= 0).sum(0)
    pos = ((nbrs >= 0) & (nbrs < e)).sum(0)
    rl = nb * (nint + 1)
    base = dp.elem_ptr[:ne] + pos * nb
    r = torch.arange(nb, device="cuda")
    idx = base[:, None, None] + r[None, :, None] * rl[:, None, None] + r[None, None, :]
    D = sum(t * v[idx] for t, v in zip(theta, vals))
    return torch.linalg.inv(D)


def build(name, n, part=(1, 1)):
    """the meshes and coefficients of scripts/bench_apply.py's configurations (part: subdomains in x and y); returns an
    assemble(sigma_scale)"""
    import torch
    import hdd_amd as H
    ctx = H.Context(0)
    if name == "c3":
        n = n or 1024
        grid = H.Grid.structured(H.SIMPLEX, n, n, (-1, -1), (1, 1), px=part[0], py=part[1])
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
        grid = H.Grid.structured(et, nx, ny, (0, 0), (5, 1), px=part[0], py=part[1])
        loc = grid.local()
        k = loc.checkerboard((0, 0), (5, 1), 100, 20, 10.0 ** np.random.default_rng(10).uniform(-3, 3, 2000))
        fns = [H.scalar_fn(H.FN_CONST, 1.0)]
        ten = H.tensor_fn(H.TENSOR_ISO_PER_ELEM, per_elem=torch.from_numpy(k).cuda())
        label = "%s_spe10_%s_%dx%d" % (name, "p1" if name == "c2" else "q1", nx, ny)
    dm = H.DeviceMesh(loc)
    dp = H.DevicePattern(loc, ctx=ctx, dmesh=dm, on_device=True)

    def assemble(scale, vals=None):
        prm = H.params(H.SIGMA_INNER_P1 * scale, H.SIGMA_BOUNDARY_P1 * scale)
        vals = H.assemble(ctx, dm, dp, fns, ten, prm, vals=vals)
        torch.cuda.synchronize()
        return vals
    return H, ctx, loc, dm, dp, assemble, label


def run_batched(args, torch, H, ctx, nb, dm, dp, vals, theta, label, reference, scale, gen):
    """--rhs N: one hdd_operator_solve_batched call on N right-hand sides against N hdd_operator_solve calls (the
    unchanged single-solve path) on the same columns, alternating over the rounds in this process.  --thetas N: one
    hdd_operator_solve_multi call against N single solves at the columns' own thetas, likewise."""
    multi = args.thetas > 0
    n, nnz, nc, N, iters = dp.t.n_rows, dp.nnz, len(vals), args.thetas or args.rhs, args.iters
    B = torch.randn((N, n), dtype=torch.float64, device="cuda", generator=gen)
    if multi and nc == 2:
        thetas = np.stack([np.ones(N), np.linspace(0.3, 1.0, N)], axis=1)
    elif multi:
        thetas = np.linspace(1.0, 2.0, N).reshape(N, 1)
    else:
        thetas = np.tile(np.asarray(theta, np.float64), (N, 1))

    def batched(k):
        if multi:
            return H.solve_multi(ctx, dp, vals, B, thetas, dmesh=dm, rtol=0.0, max_iter=k, check_every=max(k, 1))
        return H.solve_batched(ctx, dp, vals, B, theta=theta, dmesh=dm, rtol=0.0, max_iter=k, check_every=max(k, 1))

    def singles(k):
        return [H.solve(ctx, dp, vals, B[j], theta=thetas[j], dmesh=dm, rtol=0.0, max_iter=k, check_every=max(k, 1))
                for j in range(N)]

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    timed(batched, 3), timed(singles, 3)   # warm-up
    names = {}
    ms = dict(batched=[], batched_setup=[], singles=[], singles_setup=[])
    per = dict(batched=[], singles=[])
    for _ in range(args.rounds):
        t, (X, infos) = timed(batched, iters)
        names["batched"] = H.last_solve_kernels()
        ms["batched"].append(t)
        ms["batched_setup"].append(timed(batched, 0)[0])
        t, one = timed(singles, iters)
        names["singles"] = H.last_solve_kernels()
        ms["singles"].append(t)
        ms["singles_setup"].append(timed(singles, 0)[0])
        for k in per:
            per[k].append((ms[k][-1] - ms[k + "_setup"][-1]) / iters)
    identical = all(bool(torch.equal(X[j].view(torch.int64), one[j][0].view(torch.int64))) for j in range(N))
    med = {k: float(np.median(v)) for k, v in per.items()}
    groups = (N + 3) // 4
    if multi:   # every column has inverse blocks of its own
        model_b = groups * 8 * nnz * nc + N * (13 + (nb + 1) / 2) * 8 * n
    else:
        model_b = groups * (8 * nnz * nc + (nb + 1) / 2 * 8 * n) + N * 13 * 8 * n
    model_s = N * (8 * nnz * nc + (13 + (nb + 1) / 2) * 8 * n)
    res = dict(config=label, n_rows=n, nnz=nnz, n_comp=nc, block_size=nb, n_rhs=N, iters=iters, rounds=args.rounds,
               mode="thetas" if multi else "rhs", thetas=thetas.tolist(),
               reference_penalties=reference, sigma_scale=scale, kernels=names,
               status=[i.status for i in infos], iterations=[i.iterations for i in infos],
               columns_bit_identical_to_singles=identical,
               ms={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()},
               ms_per_iteration={k: dict(median=med[k], min=float(min(v)), max=float(max(v))) for k, v in per.items()},
               batched_over_singles=med["batched"] / med["singles"],
               model_bytes_per_iteration=dict(batched=model_b, singles=model_s), model_ratio=model_b / model_s,
               model_GBps=dict(batched=model_b / med["batched"] / 1e6, singles=model_s / med["singles"] / 1e6))
    print(json.dumps(res), flush=True)


def run_blocks(args, torch, H, ctx, loc, dm, dp, vals, theta, label, reference, scale, gen):
    """--blocks PX,PY: one hdd_operator_solve_blocks call over all subdomains against the loop of single solves with
    block=(ss, ss), alternating over the rounds in this process"""
    grid, nb = loc.grid, loc.nb
    n, nnz, nc, iters = dp.t.n_rows, dp.nnz, len(vals), args.iters
    S = args.blocks[0] * args.blocks[1]
    bounds = [grid.subdomain_range(s, s + 1)[0] * nb for s in range(S)] + [grid.subdomain_range(S - 1, S)[1] * nb]
    assert bounds[0] == 0 and bounds[-1] == n
    b = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)

    def blocks(k):
        return H.solve_blocks(ctx, dp, vals, b, theta=theta, dmesh=dm, bounds=bounds, rtol=0.0, max_iter=k, check_every=max(k, 1))

    def singles(k):
        return [H.solve(ctx, dp, vals, b[bounds[s]:bounds[s + 1]], theta=theta, dmesh=dm, block=(s, s), grid=grid, rtol=0.0,
                        max_iter=k, check_every=max(k, 1)) for s in range(S)]

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    timed(blocks, 3), timed(singles, 3)   # warm-up
    names = {}
    ms = dict(blocks=[], blocks_setup=[], singles=[], singles_setup=[])
    per = dict(blocks=[], singles=[])
    identical = True
    for _ in range(args.rounds):
        t, (x, infos) = timed(blocks, iters)
        names["blocks"] = H.last_solve_kernels()
        ms["blocks"].append(t)
        ms["blocks_setup"].append(timed(blocks, 0)[0])
        t, one = timed(singles, iters)
        names["singles"] = H.last_solve_kernels()
        ms["singles"].append(t)
        ms["singles_setup"].append(timed(singles, 0)[0])
        for k in per:
            per[k].append((ms[k][-1] - ms[k + "_setup"][-1]) / iters)
        for s in range(S):
            xs, i = one[s]
            identical = identical and bool(torch.equal(x[bounds[s]:bounds[s + 1]].view(torch.int64), xs.view(torch.int64))) and \
                (i.status, i.iterations, i.residual, i.rhs_norm) == (infos[s].status, infos[s].iterations, infos[s].residual, infos[s].rhs_norm)
    med = {k: float(np.median(v)) for k, v in per.items()}
    model = 8 * nnz * nc + (13 + (nb + 1) / 2) * 8 * n
    statuses = sorted(set(i.status for i in infos))
    res = dict(config=label, n_rows=n, nnz=nnz, n_comp=nc, block_size=nb, partition=list(args.blocks), n_blocks=S,
               rows_per_block=dict(min=min(e - a for a, e in zip(bounds[:-1], bounds[1:])), max=max(e - a for a, e in zip(bounds[:-1], bounds[1:]))),
               iters=iters, rounds=args.rounds, mode="blocks", reference_penalties=reference, sigma_scale=scale, kernels=names,
               statuses=statuses, iterations=dict(min=min(i.iterations for i in infos), max=max(i.iterations for i in infos)),
               segments_bit_identical_to_singles=identical,
               ms={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()},
               ms_per_iteration={k: dict(median=med[k], min=float(min(v)), max=float(max(v))) for k, v in per.items()},
               blocks_over_singles=med["blocks"] / med["singles"],
               model_bytes_per_whole_matrix_iteration=model,
               model_GBps=dict(blocks=model / med["blocks"] / 1e6, singles=model / med["singles"] / 1e6))
    print(json.dumps(res), flush=True)


def run_config(args):
    import torch
    torch.cuda.set_device(0)
    H, ctx, loc, dm, dp, assemble, label = build(args.config, args.n, args.blocks or (1, 1))
    vals = assemble(1.0)
    n, nnz, nb, nc = dp.t.n_rows, dp.nnz, loc.nb, len(vals)
    theta = [1.0, 0.3][:nc]
    gen = torch.Generator(device="cuda").manual_seed(5)
    b = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    iters = args.iters
    _, i0 = H.solve(ctx, dp, vals, b, theta=theta, dmesh=dm, rtol=0.0, max_iter=iters, check_every=iters)
    reference = dict(status=i0.status, iterations=i0.iterations, residual=i0.residual)
    scale = 1.0
    while i0.status == H.SOLVE_BREAKDOWN and scale < 1000:
        scale *= args.sigma_scale
        vals = assemble(scale, vals)
        _, i0 = H.solve(ctx, dp, vals, b, theta=theta, dmesh=dm, rtol=0.0, max_iter=iters, check_every=iters)
    if args.blocks:
        return run_blocks(args, torch, H, ctx, loc, dm, dp, vals, theta, label, reference, scale, gen)
    if args.rhs or args.thetas:
        return run_batched(args, torch, H, ctx, nb, dm, dp, vals, theta, label, reference, scale, gen)
    Dinv = inverse_blocks(torch, loc, dm, dp, vals, theta)

    def fused(k):
        return H.solve(ctx, dp, vals, b, theta=theta, dmesh=dm, rtol=0.0, max_iter=k, check_every=max(k, 1))

    q = torch.empty(n, dtype=torch.float64, device="cuda")

    def composed(k):
        x = torch.zeros_like(b)
        r = b.clone()
        z = torch.bmm(Dinv, r.view(-1, nb, 1)).view(-1)
        p = z.clone()
        rho = torch.dot(r, z).item()
        for _ in range(k):
            H.apply(ctx, dp, vals, p, theta=theta, dmesh=dm, out=q)
            alpha = rho / torch.dot(p, q).item()
            x.add_(p, alpha=alpha)
            r.add_(q, alpha=-alpha)
            z = torch.bmm(Dinv, r.view(-1, nb, 1)).view(-1)
            rho_new = torch.dot(r, z).item()
            p.mul_(rho_new / rho).add_(z)
            rho = rho_new
        return x, torch.linalg.vector_norm(r).item()

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    timed(fused, 3), timed(composed, 3)   # warm-up
    ms = dict(fused=[], fused_setup=[], composed=[], composed_setup=[])
    for _ in range(args.rounds):
        t, (xf, info) = timed(fused, iters)
        ms["fused"].append(t)
        ms["fused_setup"].append(timed(fused, 0)[0])
        t, (xc, rc) = timed(composed, iters)
        ms["composed"].append(t)
        ms["composed_setup"].append(timed(composed, 0)[0])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    per_f = (med["fused"] - med["fused_setup"]) / iters
    per_c = (med["composed"] - med["composed_setup"]) / iters
    model = 8 * nnz * nc + (13 + (nb + 1) / 2) * 8 * n
    res = dict(config=label, n_rows=n, nnz=nnz, n_comp=nc, block_size=nb, iters=iters, rounds=args.rounds,
               reference_penalties=reference, sigma_scale=scale,
               kernels=H.last_solve_kernels(), status=info.status, iterations=info.iterations,
               residual_fused=info.residual, residual_composed=rc, rhs_norm=info.rhs_norm,
               x_rel_diff=float(torch.linalg.vector_norm(xf - xc) / torch.linalg.vector_norm(xc)),
               ms={k: dict(median=med[k], min=float(min(v)), max=float(max(v))) for k, v in ms.items()},
               ms_per_iteration_fused=per_f, ms_per_iteration_composed=per_c, composed_over_fused=per_c / per_f,
               model_bytes_per_iteration=model, model_GBps_fused=model / per_f / 1e6,
               model_GBps_composed=model / per_c / 1e6)
    if args.converge:
        t, (x, ic) = timed(lambda k: H.solve(ctx, dp, vals, b, theta=theta, dmesh=dm, rtol=1e-8, max_iter=k, check_every=64),
                           args.converge)
        res["to_rtol_1e-8"] = dict(status=ic.status, iterations=ic.iterations, residual=ic.residual, ms=t)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["c2", "c3", "c4"])
    ap.add_argument("--config", default=None, help="(child) run this one configuration in this process")
    ap.add_argument("--n", type=int, default=0, help="nx of the mesh (default: the configuration's size)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sigma-scale", type=float, default=4.0, help="penalty factor per step when the solve breaks down")
    ap.add_argument("--converge", type=int, default=0, help="also solve to rtol 1e-8 with at most this many iterations")
    ap.add_argument("--rhs", type=int, default=0, help="N > 0: time one batched solve of N right-hand sides against N single "
                    "solves instead (bench_solve_batched.jsonl)")
    ap.add_argument("--thetas", type=int, default=0, help="N > 0: time one solve_multi of N columns at N thetas against N single "
                    "solves at those thetas instead (bench_solve_multi.jsonl)")
    ap.add_argument("--blocks", type=lambda v: tuple(int(t) for t in v.split(",")), default=None,
                    help="PX,PY: time one solve_blocks over all PX x PY subdomains against the loop of single local solves instead "
                    "(appended to bench_solve_blocks.jsonl)")
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per configuration (child process)")
    ap.add_argument("--out", default=None, help="directory for bench_solve.jsonl")
    args = ap.parse_args()
    if args.config:
        run_config(args)
        return 0
    lines = []
    for c in args.configs:
        cmd = [sys.executable, os.path.abspath(__file__), "--config", c, "--n", str(args.n), "--iters", str(args.iters),
               "--rounds", str(args.rounds), "--converge", str(args.converge), "--sigma-scale", str(args.sigma_scale), "--rhs", str(args.rhs),
               "--thetas", str(args.thetas)]
        if args.blocks:
            cmd += ["--blocks", "%d,%d" % args.blocks]
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
        name = "bench_solve_blocks.jsonl" if args.blocks else "bench_solve_multi.jsonl" if args.thetas else "bench_solve_batched.jsonl" if args.rhs else "bench_solve.jsonl"
        with open(os.path.join(args.out, name), "a" if args.blocks else "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
