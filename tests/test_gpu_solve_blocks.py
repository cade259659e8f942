"""Every segment of a partition per call (hdd_operator_solve_blocks / hdd_operator_apply_blocks: H.solve_blocks,
H.apply_blocks) against the single calls on the segments' ranges.

The oracle is hdd_operator_solve (H.solve) with the range (bounds[s], bounds[s + 1]) squared on (b_s, x0_s) with the
same options on the same path: the contract is bit equality, so every comparison is torch.equal on the bits of x and
the histories and equality of the tuples (status, iterations, residual, rhs_norm) -- the doubles by their bits, so that a
NaN residual compares, too.  Every case asserts the kernel names.  Case 1 also takes the host matrix through
test_gpu_solve.check_solution.  The meshes are ones DESIGN.md 4.7 lists as positive definite (principal blocks of a
definite matrix are definite); where a case needs converged solves it asserts the statuses of the single solves.
"""
import ctypes as C
import struct

import numpy as np
import pytest

from cases import SPE10_LOWER, SPE10_UPPER, os2014_components
from test_gpu_apply import Case
from test_gpu_apply_grid import grid_case, tile_grid
from test_gpu_solve import RTOL, check_solution, dev, numpy_pcg, problem

H = pytest.importorskip("hdd_amd")
pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def names(path, nb, bs, pre=True):
    """what hdd_last_solve_kernels() reports for a blocks solve"""
    apply = {"tile": "apply_tile_blocks_kernel<%d, %d, dot>" % (nb, nb), "csr": "apply_csr_blocks_kernel<8, dot>",
             "csr64": "apply_csr_blocks_kernel<64, dot>"}[path]
    return apply + " + cg_update_blocks<%d%s> + cg_direction_blocks" % (bs, "" if pre else ", none")


def bits(i):
    return (i.status, i.iterations, struct.pack("d", i.residual), struct.pack("d", i.rhs_norm))


def same(a, b):
    """bit equality of two float64 tensors (torch.equal, but NaNs compare by their bits, too)"""
    torch = _torch()
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def sub_bounds(c, s0, s1):
    """the rows at which subdomains s0 .. s1 - 1 begin and end"""
    nb = c.grid.nb
    return [nb * c.grid.subdomain_range(s, s + 1)[0] for s in range(s0, s1)] + [nb * c.grid.subdomain_range(s1 - 1, s1)[1]]


_EXTRA = {}


def extra_case(ctx, name):
    if name not in _EXTRA:
        if name == "q1_4x2":      # eight subdomains of 40 elements
            _EXTRA[name] = Case(ctx, H.Grid.structured(H.CUBE, 40, 8, SPE10_LOWER, SPE10_UPPER, px=4, py=2))
        elif name == "p1_4x3":    # twelve subdomains of 120 elements
            _EXTRA[name] = Case(ctx, H.Grid.structured(H.SIMPLEX, 60, 12, SPE10_LOWER, SPE10_UPPER, px=4, py=3))
        elif name == "os2014_2x2":
            fns = [H.scalar_fn(H.FN_SINUSOID, a, b, kx, ky, order=3) for (a, b, kx, ky) in os2014_components()]
            _EXTRA[name] = Case(ctx, H.Grid.structured(H.SIMPLEX, 16, 16, (-1, -1), (1, 1), px=2, py=2), kappas=fns,
                                tensor=H.tensor_fn())
    return _EXTRA[name]


def rhs_for(c, bd, seed):
    return dev(np.random.default_rng(seed).standard_normal(bd[-1] - bd[0]))


def singles(ctx, c, bd, b, dm, x0=None, vals=None, **kw):
    """the single solves on the segments' ranges: [(x_s, info_s)]"""
    out = []
    for lo, hi in zip(bd[:-1], bd[1:]):
        a, e = lo - bd[0], hi - bd[0]
        out.append(H.solve(ctx, c.dp, c.vals if vals is None else vals, b[a:e], dmesh=dm, block=(lo, hi, lo, hi),
                           x0=None if x0 is None else x0[a:e], history=True, **kw))
    return out


def against_singles(ctx, c, bd, b, dm, kernels, x0=None, vals=None, ref=None, **kw):
    """one blocks solve, bit for bit the single solves (ref: computed before); returns x, infos, the single solves"""
    torch = _torch()
    x, infos = H.solve_blocks(ctx, c.dp, c.vals if vals is None else vals, b, dmesh=dm, bounds=bd, x0=x0, history=True, **kw)
    assert H.last_solve_kernels() == kernels
    assert x.shape == (bd[-1] - bd[0],) and len(infos) == len(bd) - 1
    if ref is None:
        ref = singles(ctx, c, bd, b, dm, x0=x0, vals=vals, **kw)
    for s, (xs, i) in enumerate(ref):
        a, e = bd[s] - bd[0], bd[s + 1] - bd[0]
        print("segment %d: status %d, %d iterations, ||r|| %.3e" % (s, infos[s].status, infos[s].iterations, infos[s].residual))
        assert bits(infos[s]) == bits(i), (s, bits(infos[s]), bits(i))
        assert same(x[a:e], xs), s
        assert same(infos[s].history, i.history), s
    return x, infos, ref


# ---- 1, 2: all subdomains in one call -------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["tile", "csr"])
def test_all_four_subdomains(ctx, path):
    """Kuhn 40 x 8 in 2 x 2 subdomains: four segments of 160 elements = 2.5 tiles, the second and the fourth beginning
    inside a tile of the global numbering; against the single solves and against the sliced host matrix"""
    P = problem(ctx, "p1_block")
    c = P.c
    bd = sub_bounds(c, 0, 4)
    assert [(e - a) // 3 for a, e in zip(bd[:-1], bd[1:])] == [160] * 4 and [(a // 3) % 64 for a in bd[:-1]] == [0, 32, 0, 32]
    host = []
    for s in range(4):
        A = P.A[bd[s]:bd[s + 1], bd[s]:bd[s + 1]].tocsr()
        xs = np.random.default_rng(60 + s).standard_normal(A.shape[0])
        host.append((A, float(np.linalg.eigvalsh(A.toarray())[0]), xs, A @ xs))
    b = dev(np.concatenate([h[3] for h in host]))
    x, infos, _ = against_singles(ctx, c, bd, b, c.dm if path == "tile" else None, names(path, 3, 3), rtol=RTOL)
    for s, (A, lmin, xs, rhs) in enumerate(host):
        check_solution(A, lmin, rhs, xs, x[bd[s]:bd[s + 1]], infos[s], numpy_pcg(A, rhs, 3, RTOL)[1])
    # the front end's subdomains= gives the same bounds
    x2, infos2 = H.solve_blocks(ctx, c.dp, c.vals, b, dmesh=c.dm if path == "tile" else None, subdomains=(0, 4), rtol=RTOL)
    assert _torch().equal(x2, x) and [bits(i) for i in infos2] == [bits(i) for i in infos]


@pytest.mark.parametrize("path", ["tile", "csr"])
def test_segments_shorter_than_one_wave(ctx, path):
    """Q1 40 x 8 in 4 x 2 subdomains: eight segments of 40 elements"""
    c = extra_case(ctx, "q1_4x2")
    bd = sub_bounds(c, 0, 8)
    assert [(e - a) // 4 for a, e in zip(bd[:-1], bd[1:])] == [40] * 8
    _, _, ref = against_singles(ctx, c, bd, rhs_for(c, bd, 70), c.dm if path == "tile" else None, names(path, 4, 4), rtol=RTOL)
    assert all(i.status == H.SOLVE_CONVERGED and i.iterations > 0 for _, i in ref)


# ---- 3: unequal segments, check_every ---------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["tile", "csr"])
def test_unequal_segments_and_check_every(ctx, path):
    """Kuhn 60 x 12 in 4 x 3 subdomains of 120 elements, merged into segments of 1, 3, 1 and 7 subdomains: the segments
    end at different iterations (asserted), so finished ones are frozen while the others go on; the number of
    iterations between two looks changes no bit"""
    c = extra_case(ctx, "p1_4x3")
    sb = sub_bounds(c, 0, 12)
    assert [(e - a) // 3 for a, e in zip(sb[:-1], sb[1:])] == [120] * 12
    bd = [sb[0], sb[1], sb[4], sb[5], sb[12]]
    dm = c.dm if path == "tile" else None
    b = rhs_for(c, bd, 71)
    ref = singles(ctx, c, bd, b, dm, rtol=RTOL, check_every=1)
    its = [i.iterations for _, i in ref]
    assert all(i.status == H.SOLVE_CONVERGED for _, i in ref) and len(set(its)) > 1, its
    for ce in (1, 7, 0):
        against_singles(ctx, c, bd, b, dm, names(path, 3, 3), ref=ref, rtol=RTOL, check_every=ce)


# ---- 4: a sub-interval, padding and alignment -------------------------------------------------------------------------

def _raw_blocks(ctx, c, bd, b, dm, bs, shift, max_iter=10000):
    """hdd_operator_solve_blocks through ctypes: b, x, the workspace and the history inside NaN padding, x and the
    workspace `shift` doubles past a 16-byte boundary; nothing around them may be written"""
    torch = _torch()
    rows, n = bd[-1] - bd[0], len(bd) - 1
    n_work = int(H.lib().hdd_operator_solve_blocks_workspace(rows, bs, n))
    ldh = max_iter + 1
    nan = lambda m: torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
    bbuf, xbuf, wbuf, hbuf = nan(rows + 8), nan(rows + 8), nan(n_work + 8), nan(n * ldh + 8)
    o = 2 + shift
    bbuf[3:3 + rows] = b
    hbuf[4:4 + n * ldh] = 0.0
    x, w = xbuf[o:o + rows], wbuf[o:o + n_work]
    assert x.data_ptr() % 16 == 8 * shift and w.data_ptr() % 16 == 8 * shift
    ptrs = (C.c_void_p * 1)(c.vals[0].data_ptr())
    opt = H.SolveOptions(RTOL, 0.0, max_iter, 0, H.PRECOND_BLOCK_JACOBI, bs, 0, 0)
    infos = (H.SolveInfo * n)()
    bounds = np.asarray(bd, np.int64)
    rc = H.lib().hdd_operator_solve_blocks(ctx.h, None if dm is None else C.addressof(dm.t), C.addressof(c.dp.t), ptrs, 1, None,
                                           n, bounds.ctypes.data, bbuf[3:].data_ptr(), x.data_ptr(), C.addressof(opt),
                                           w.data_ptr(), n_work, hbuf[4:].data_ptr(), ldh, C.addressof(infos),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, H.lib().hdd_last_error(None)
    torch.cuda.synchronize()
    for buf, lead, m in ((xbuf, o, rows), (wbuf, o, n_work), (bbuf, 3, rows), (hbuf, 4, n * ldh)):
        assert bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + m:]).all())
    assert torch.equal(bbuf[3:3 + rows], b)
    hist = hbuf[4:4 + n * ldh].reshape(n, ldh)
    return x.clone(), [bits(i) for i in infos], [hist[s, :infos[s].iterations + 1].clone() for s in range(n)]


@pytest.mark.parametrize("path", ["tile", "csr"])
@pytest.mark.parametrize("bs", [2, 4])
def test_sub_interval_padding_and_alignment(ctx, path, bs):
    """subdomains 1 and 2 of the 2 x 2 partition only: the interval begins behind row 0 and ends before n_rows"""
    torch = _torch()
    P = problem(ctx, "p1_block")
    c = P.c
    bd = sub_bounds(c, 1, 3)
    assert bd[0] > 0 and bd[-1] < c.n_rows and all(v % bs == 0 for v in bd)
    dm = c.dm if path == "tile" else None
    b = rhs_for(c, bd, 72)
    xa, ia, ha = _raw_blocks(ctx, c, bd, b, dm, bs, 0)
    assert H.last_solve_kernels() == names(path, 3, bs)
    xu, iu, hu = _raw_blocks(ctx, c, bd, b, dm, bs, 1)
    assert iu == ia and torch.equal(xu, xa) and all(torch.equal(u, a) for u, a in zip(hu, ha))
    ref = singles(ctx, c, bd, b, dm, rtol=RTOL, block_size=bs)
    for s, (xs, i) in enumerate(ref):
        assert i.status == H.SOLVE_CONVERGED
        assert ia[s] == bits(i) and torch.equal(xa[bd[s] - bd[0]:bd[s + 1] - bd[0]], xs) and torch.equal(ha[s], i.history)


# ---- 5: mixed fates ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["tile", "csr"])
def test_mixed_fates(ctx, path):
    """a zero segment, a NaN, a segment that is not definite and a healthy one in one call: every fate stays with its
    segment, the call returns normally, and the healthy segment keeps the bits of its single solve"""
    torch = _torch()
    P = problem(ctx, "p1_block")
    c = P.c
    dm = c.dm if path == "tile" else None
    bd = sub_bounds(c, 0, 4)
    assert P.lmin > 0
    vals = [c.vals[0].clone()]
    rp = c.rp
    vals[0][int(rp[bd[2]]):int(rp[bd[3]])] *= -1.0          # the rows of segment 2: its diagonal blocks, A_22 = -A_22
    b = rhs_for(c, bd, 73)
    b[bd[0]:bd[1]] = 0.0
    b[bd[1] + 7] = float("nan")
    x0 = rhs_for(c, bd, 74)
    for guess in (None, x0):
        x, infos, _ = against_singles(ctx, c, bd, b, dm, names(path, 3, 3), x0=guess, vals=vals, rtol=RTOL)
        assert bits(infos[0]) == (H.SOLVE_CONVERGED, 0, struct.pack("d", 0.0), struct.pack("d", 0.0))
        assert not bool(x[bd[0]:bd[1]].any())
        assert (infos[1].status, infos[1].iterations) == (H.SOLVE_BREAKDOWN, 0)
        assert (infos[2].status, infos[2].iterations) == (H.SOLVE_BREAKDOWN, 0)
        assert infos[3].status == H.SOLVE_CONVERGED and infos[3].iterations > 0
        for s in (1, 2):      # broken down before the first iteration: x is the initial guess
            want = torch.zeros_like(x[bd[s]:bd[s + 1]]) if guess is None else guess[bd[s]:bd[s + 1]]
            assert torch.equal(x[bd[s]:bd[s + 1]], want), s
    # without the preconditioner the negated segment breaks down on p . Ap <= 0 in the first iteration: x untouched
    x, infos, _ = against_singles(ctx, c, bd, b, dm, names(path, 3, 3, pre=False), vals=vals, rtol=RTOL, precond="none")
    assert (infos[2].status, infos[2].iterations) == (H.SOLVE_BREAKDOWN, 0) and not bool(x[bd[2]:bd[3]].any())
    assert infos[3].status == H.SOLVE_CONVERGED and infos[0].iterations == 0
    # -A: every segment breaks down
    b2 = rhs_for(c, bd, 75)
    x, infos, _ = against_singles(ctx, c, bd, b2, dm, names(path, 3, 3), theta=[-1.0], rtol=RTOL)
    assert all((i.status, i.iterations) == (H.SOLVE_BREAKDOWN, 0) for i in infos) and bool(torch.isfinite(x).all())
    # max_iter
    x, infos, _ = against_singles(ctx, c, bd, b2, dm, names(path, 3, 3), rtol=RTOL, max_iter=3)
    assert all((i.status, i.iterations) == (H.SOLVE_MAX_ITER, 3) for i in infos)
    assert all(i.history.shape == (4,) and i.history[3].item() == i.residual for i in infos)
    x, infos, _ = against_singles(ctx, c, bd, b2, dm, names(path, 3, 3), rtol=RTOL, max_iter=0)
    assert all((i.status, i.iterations) == (H.SOLVE_MAX_ITER, 0) for i in infos) and not bool(x.any())


# ---- 6: warm start and atol ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["tile", "csr"])
def test_warm_start_and_atol(ctx, path):
    torch = _torch()
    P = problem(ctx, "p1_block")
    c = P.c
    dm = c.dm if path == "tile" else None
    bd = sub_bounds(c, 0, 4)
    b = rhs_for(c, bd, 76)
    for s in range(4):                                      # ||b_s|| a decade apart
        b[bd[s]:bd[s + 1]] *= 10.0 ** s
    x0 = rhs_for(c, bd, 77)
    _, infos, ref = against_singles(ctx, c, bd, b, dm, names(path, 3, 3), x0=x0, rtol=RTOL)
    assert all(i.status == H.SOLVE_CONVERGED and i.iterations > 0 for i in infos)
    # atol between the thresholds rtol ||b_s|| of segments 1 and 2: atol decides for 0 and 1, rtol for 2 and 3
    rt = [RTOL * i.rhs_norm for i in infos]
    atol = float(np.sqrt(rt[1] * rt[2]))
    assert rt[0] < rt[1] < atol < rt[2] < rt[3]
    _, infos, _ = against_singles(ctx, c, bd, b, dm, names(path, 3, 3), rtol=RTOL, atol=atol)
    for s, i in enumerate(infos):
        thresh = max(rt[s], atol)
        h = i.history.cpu().numpy()
        assert i.status == H.SOLVE_CONVERGED and i.iterations > 0
        assert i.residual <= thresh * (1 + 1e-12) and h[i.iterations - 1] > thresh, s


# ---- 7: other paths --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["tile", "csr"])
@pytest.mark.parametrize("bs", [1, 6])
def test_block_sizes(ctx, path, bs):
    """blocks from the CSR arrays (block_size != nb) under the tile and the CSR apply"""
    P = problem(ctx, "p1_block")
    c = P.c
    bd = sub_bounds(c, 0, 4)
    assert all(v % bs == 0 for v in bd)
    _, _, ref = against_singles(ctx, c, bd, rhs_for(c, bd, 78), c.dm if path == "tile" else None, names(path, 3, bs),
                                rtol=RTOL, block_size=bs)
    assert all(i.status == H.SOLVE_CONVERGED for _, i in ref)


def test_hexahedra(ctx):
    """Q1 hexahedra 4^3 in two x-slabs of 32, blocks of 8: a wave per row"""
    P = problem(ctx, "hex_block")
    c = P.c
    bd = sub_bounds(c, 0, 2)
    assert bd == [0, 256, 512]
    _, _, ref = against_singles(ctx, c, bd, rhs_for(c, bd, 79), c.dm, names("csr64", 8, 8), rtol=RTOL, block_size=8)
    assert all(i.status == H.SOLVE_CONVERGED for _, i in ref)


@pytest.mark.parametrize("path", ["tile", "csr"])
def test_two_components(ctx, path):
    """OS2014 16 x 16 in 2 x 2 subdomains, theta = (1, 0.5) fused; on the tile path and without a mesh"""
    c = extra_case(ctx, "os2014_2x2")
    assert len(c.vals) == 2
    bd = sub_bounds(c, 0, 4)
    _, _, ref = against_singles(ctx, c, bd, rhs_for(c, bd, 80), c.dm if path == "tile" else None, names(path, 3, 3),
                                theta=[1.0, 0.5], rtol=RTOL)
    assert all(i.status == H.SOLVE_CONVERGED for _, i in ref)


# ---- 8: multi-pass virtual grids -------------------------------------------------------------------------------------------

def multipass_bounds(c):
    """three segments of the large Kuhn mesh (in rows) and the facts the case rests on"""
    G = tile_grid(8)
    n_el = c.local.n_own
    n0, n1 = 64 * (G + 37) - 19, 64 * 10 + 17
    if c.ep[n0 + n1] % 2 == 0 and c.ep[n0] % 2 == 0:
        n1 += 1
    el = [0, n0, n0 + n1, n_el]
    tiles = [-(-(e - a) // 64) for a, e in zip(el[:-1], el[1:])]
    assert tiles[0] > G > 64                        # a second sweep; more than 64 partial sums of p . q
    assert -(-(el[1] - el[0]) // 256) > 64          # ... and of r . z, r . r (one per 256 blocks)
    assert 10 < tiles[1] < G and 0 < tiles[2] < G
    assert c.ep[el[1]] % 2 == 1 or c.ep[el[2]] % 2 == 1      # a later segment's image origin is misaligned
    return [3 * e for e in el]


@pytest.mark.parametrize("path", ["tile", "csr"])
def test_multi_pass_virtual_grids(ctx, path):
    c = grid_case(ctx, "p1")
    bd = multipass_bounds(c)
    _, infos, _ = against_singles(ctx, c, bd, rhs_for(c, bd, 81), c.dm if path == "tile" else None, names(path, 3, 3),
                                  rtol=0.0, max_iter=10)
    assert all((i.status, i.iterations) == (H.SOLVE_MAX_ITER, 10) for i in infos)


# ---- 9: apply_blocks ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,path", [("p1_block", "tile"), ("p1_block", "csr"), ("q1_4x2", "tile"), ("q1_4x2", "csr"),
                                       ("grid", "tile"), ("grid", "csr")])
def test_apply_blocks(ctx, name, path):
    """every segment has the bits of H.apply on its range; a NaN-filled segment of x stays in its own segment of y;
    nothing outside y is written"""
    torch = _torch()
    if name == "p1_block":
        c = problem(ctx, name).c
        bd = sub_bounds(c, 0, 4)
    elif name == "q1_4x2":
        c = extra_case(ctx, name)
        bd = sub_bounds(c, 0, 8)
    else:
        c = grid_case(ctx, "p1")
        bd = multipass_bounds(c)
    nb = c.grid.nb
    dm = c.dm if path == "tile" else None
    kernel = "apply_tile_blocks_kernel<%d, %d>" % (nb, nb) if path == "tile" else "apply_csr_blocks_kernel<8>"
    rows = bd[-1] - bd[0]
    x = rhs_for(c, bd, 82)
    ybuf = torch.full((rows + 8,), float("nan"), dtype=torch.float64, device="cuda")
    y = H.apply_blocks(ctx, c.dp, c.vals, x, dmesh=dm, bounds=bd, out=ybuf[3:3 + rows])
    assert H.last_apply_kernel() == kernel
    assert y.data_ptr() == ybuf[3:].data_ptr()
    assert bool(torch.isnan(ybuf[:3]).all()) and bool(torch.isnan(ybuf[3 + rows:]).all())
    for lo, hi in zip(bd[:-1], bd[1:]):
        want = H.apply(ctx, c.dp, c.vals, x[lo - bd[0]:hi - bd[0]], dmesh=dm, block=(lo, hi, lo, hi))
        assert torch.equal(y[lo - bd[0]:hi - bd[0]], want), (lo, hi)
    assert bool(torch.isfinite(y).all())
    if name != "grid":
        y_sub = H.apply_blocks(ctx, c.dp, c.vals, x, dmesh=dm, subdomains=(0, len(bd) - 1))
        assert torch.equal(y_sub, y)
    # a NaN-filled segment of x
    xn = x.clone()
    xn[bd[1] - bd[0]:bd[2] - bd[0]] = float("nan")
    yn = H.apply_blocks(ctx, c.dp, c.vals, xn, dmesh=dm, bounds=bd)
    assert torch.equal(yn[:bd[1] - bd[0]], y[:bd[1] - bd[0]]) and torch.equal(yn[bd[2] - bd[0]:], y[bd[2] - bd[0]:])
    assert bool(torch.isnan(yn[bd[1] - bd[0]:bd[2] - bd[0]]).all())
    # a sub-interval: the later segments alone
    y1 = H.apply_blocks(ctx, c.dp, c.vals, x[bd[1] - bd[0]:], dmesh=dm, bounds=bd[1:])
    assert torch.equal(y1, y[bd[1] - bd[0]:])
