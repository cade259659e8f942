"""hdd_operator_apply / hdd_operator_apply2 past one pass: meshes large enough that the tile kernel's workgroups walk
several tiles (tile_range's XCD sweep, the LDS image re-used behind lds_wave_sync, `if (!active) continue` in a tile
that is not the wave's last), that apply_csr_kernel takes more than one grid-stride pass and that apply2 runs its 512
workgroups over more than one row per thread and sums 512 partials.  test_gpu_apply.py stays below all of these.

The sizes are derived from the device's CU count with the grid formulas of apply_plan.hh / abi_apply.hip and every
condition is asserted as an input condition (grid_facts): a device with another CU count gets another mesh or fails
loudly.  On 256 CUs:
  p1    Kuhn 600 x 146 on the SPE10 box, synthetic checkerboard tensor: 175,200 elements = 2,738 tiles > G = 2,048
        (2,737 whole tiles + 32 elements; 342.25 tiles per XCD eighth, so 86 or 87 of an eighth's 256 waves take two
        tiles and the others one), 525,600 rows > 16384 * 32 (second pass of apply_csr_kernel<8, NV>) and > 512 * 1024 (apply2)
  q1    cube 260 x 253, same box and tensor, both penalties times 4 (SIGMA_SCALE): 65,780 elements = 1,028 tiles
        > G = 1,024 (128.5 per eighth: 4 waves take two tiles), 52 elements in the last tile, 263,120 rows
  hex   Q1 hexahedra 24 x 20 x 18: 69,120 rows > 16384 * 4 (second pass of apply_csr_kernel<64, NV>)
Reference and tolerance are test_gpu_apply.py's: the scipy matrix of the downloaded arrays and 2 gamma_K |A||x| per
row, exact zeros where the scale is zero.  The reference of a (case, x) pair is computed once and shared.
"""
import numpy as np
import pytest

import test_gpu_apply as TA
from cases import SPE10_LOWER, SPE10_UPPER
from test_gpu_apply import Case, apply2_reference, both_paths, reference, strided

H = pytest.importorskip("hdd_amd")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

CSR_GRID_CAP = 16384      # apply_grid: workgroups of a plain CSR launch
APPLY2_BLOCKS = 512       # apply_kernels.hh
HEX_N = (24, 20, 18)
# penalty factor per case (H.params(8 s, 14 s)); 1: the reference's penalties.  test_gpu_solve_grid.py needs positive
# definite matrices: on the q1 mesh, whose elements are 4.9 times as wide as high, 63,191 of the 65,780 diagonal
# blocks are not positive definite with the reference's penalties and all are with 4 times them.
SIGMA_SCALE = {"p1": 1.0, "q1": 4.0}


def _torch():
    import torch
    return torch


def n_cu():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def tile_grid(per_cu, n_tiles=None):
    """apply_grid: workgroups of the tile kernel (per_cu 8 for P1, 4 for Q1)"""
    G = max(8, (n_cu() * per_cu) & ~7)
    return G if n_tiles is None else min(G, n_tiles)


def tiles_per_wave(G, n_tiles):
    """tile_range (swipdg_persistent.hh): how many tiles each of the G workgroups walks"""
    if G >= n_tiles:
        return np.ones(n_tiles, np.int64)
    b = np.arange(G)
    x, w, gx = b & 7, b >> 3, G >> 3
    s0, s1 = n_tiles * x // 8, n_tiles * (x + 1) // 8
    return np.maximum(0, -(-(s1 - s0 - w) // gx))


def p1_conditions(n_el, G):
    n_tiles = -(-n_el // 64)
    return (G < n_tiles < 2 * G and n_el % 64 == 32 and n_tiles % 8 != 0 and 3 * n_el > CSR_GRID_CAP * 32
            and 3 * n_el > APPLY2_BLOCKS * 1024)


def p1_size():
    """the fewest Kuhn triangles with p1_conditions, nx a multiple of the checkerboard's 100 columns (ties: the
    flattest mesh, the SPE10 box being 5 x 1); px = 4, py = 2 must divide it"""
    G = tile_grid(8)
    best = None
    for nx in range(100, 1601, 100):
        for ny in range(2, 4000, 2):
            if p1_conditions(2 * nx * ny, G):
                if best is None or (nx * ny, -nx) < (best[0] * best[1], -best[0]):
                    best = (nx, ny)
                break
    assert best is not None, "no P1 mesh for %d CUs" % n_cu()
    return best


def q1_conditions(n_el, G):
    n_tiles = -(-n_el // 64)
    return G < n_tiles < 2 * G and n_el % 64 != 0 and n_tiles % 8 != 0


def q1_size():
    """nx the first multiple of 20 at or above sqrt(64 G), ny the smallest with q1_conditions"""
    G = tile_grid(4)
    nx = -(-int(np.ceil(np.sqrt(64.0 * G))) // 20) * 20
    for ny in range(1, 100000):
        if q1_conditions(nx * ny, G):
            return nx, ny
    raise AssertionError("no Q1 mesh for %d CUs" % n_cu())


_CASES = {}


def grid_case(ctx, name):
    """the large cases, assembled once per session (test_gpu_solve_grid.py shares them)"""
    if name in _CASES:
        return _CASES[name]
    if name in ("p1", "p1_block"):
        nx, ny = p1_size()
        s = SIGMA_SCALE["p1"]
        part = dict(px=4, py=2) if name == "p1_block" else {}
        c = Case(ctx, H.Grid.structured(H.SIMPLEX, nx, ny, SPE10_LOWER, SPE10_UPPER, **part),
                 prm=H.params(H.SIGMA_INNER_P1 * s, H.SIGMA_BOUNDARY_P1 * s))
    elif name == "q1":
        nx, ny = q1_size()
        s = SIGMA_SCALE["q1"]
        c = Case(ctx, H.Grid.structured(H.CUBE, nx, ny, SPE10_LOWER, SPE10_UPPER),
                 prm=H.params(H.SIGMA_INNER_P1 * s, H.SIGMA_BOUNDARY_P1 * s))
    elif name == "hex":
        c = Case(ctx, H.Grid.structured3d(HEX_N, degree=1), tensor=H.tensor_fn(dim=3), prm=H.params_for(1, 3))
    else:
        raise KeyError(name)
    _CASES[name] = c
    return c


def grid_facts(c, name):
    """asserts the input conditions of the module docstring; returns (rows, n_tiles, G)"""
    rows, n_el = c.n_rows, c.local.n_own
    if name == "hex":
        assert rows == 8 * n_el and rows > CSR_GRID_CAP * 4            # apply_csr_kernel<64, NV> loops
        assert c.dp.nnz // rows > 32                                   # ... and is the kernel taken (short_rows false)
        return rows, 0, 0
    per_cu, nb = (8, 3) if name.startswith("p1") else (4, 4)
    G = tile_grid(per_cu)
    n_tiles = -(-n_el // 64)
    assert rows == nb * n_el and c.n_cols == rows
    assert n_tiles > G, (n_tiles, G)                                   # tile_range's sweep, not {b, b + 1, 1}
    assert n_el % 64 != 0                                              # a partial last tile
    per_wave = tiles_per_wave(G, n_tiles)
    assert per_wave.sum() == n_tiles and per_wave.min() == 1 and per_wave.max() == 2    # one and two tiles per wave
    assert n_tiles % 8 != 0                                            # uneven XCD eighths
    if nb == 3:
        assert n_el % 64 == 32
        assert rows > CSR_GRID_CAP * 32                                # apply_csr_kernel<8, NV> loops
        assert rows > APPLY2_BLOCKS * 1024                             # apply2_partial_kernel at its cap
    assert c.dp.nnz // rows <= 32                                      # short rows: 8 lanes per row
    return rows, n_tiles, G


_REFERENCES = {}


@pytest.fixture(autouse=True)
def shared_references(monkeypatch):
    """both_paths computes its reference through test_gpu_apply.reference: the same function, remembered per
    (arrays, theta, range, x), so that the 19 M-entry host matrices are built once per case and vector set"""
    def remembered(rp, col, hvals, theta, shape, rng, X):
        key = (id(rp), id(hvals[0]), None if theta is None else tuple(theta), rng, X.shape, X.tobytes()[:64])
        if key not in _REFERENCES:
            _REFERENCES[key] = reference(rp, col, hvals, theta, shape, rng, X)
        return _REFERENCES[key]
    monkeypatch.setattr(TA, "reference", remembered)
    return remembered


def worst_fraction(y, y_ref, bound):
    err = np.abs(y.cpu().numpy().reshape(y_ref.shape) - y_ref)
    return float((err[bound > 0] / bound[bound > 0]).max())


@pytest.mark.parametrize("name", ["p1", "q1"])
@pytest.mark.parametrize("n_vec", [1, 5])
def test_persistent_tiles_and_csr_passes(ctx, shared_references, name, n_vec):
    """more tiles than workgroups on the tile path, and for p1 more rows than one pass of the generic path; 1 vector
    and 5 (one 4-vector launch, then one single-vector launch), ldx != n"""
    c = grid_case(ctx, name)
    rows, n_tiles, G = grid_facts(c, name)
    X = np.random.default_rng(300 + n_vec).standard_normal((n_vec, c.n_cols))
    yt, yg = both_paths(ctx, c, X)      # asserts apply_tile_kernel< / apply_csr_kernel< and the bound on both paths
    assert H.last_apply_kernel() == "apply_csr_kernel<8, 1>"      # the last launch is the single-vector one
    H.apply(ctx, c.dp, c.vals, strided(X, 5), dmesh=c.dm)
    assert H.last_apply_kernel() == ("apply_tile_kernel<3, 3, 1>" if name == "p1" else "apply_tile_kernel<4, 4, 1>")
    y_ref, bound, _ = shared_references(c.rp, c.col, c.hvals, None, (c.n_rows, c.n_cols), None, X)
    print("%s: rows %d, n_tiles %d > G %d, worst error / bound: tile %.3f, csr %.3f"
          % (name, rows, n_tiles, G, worst_fraction(yt, y_ref, bound), worst_fraction(yg, y_ref, bound)))


@pytest.mark.parametrize("n_vec", [1, 5])
def test_hexahedra_csr_passes(ctx, shared_references, n_vec):
    """a wave per row over more rows than 16384 workgroups of 4 waves hold: the generic path only"""
    c = grid_case(ctx, "hex")
    rows, _, _ = grid_facts(c, "hex")
    X = np.random.default_rng(310 + n_vec).standard_normal((n_vec, c.n_cols))
    yt, yg = both_paths(ctx, c, X, tile=False)
    assert H.last_apply_kernel() == "apply_csr_kernel<64, 1>"
    y_ref, bound, _ = shared_references(c.rp, c.col, c.hvals, None, (c.n_rows, c.n_cols), None, X)
    print("hex: rows %d, worst error / bound %.3f" % (rows, worst_fraction(yg, y_ref, bound)))


def test_block_range_off_the_tile_boundaries(ctx):
    """the p1 mesh in 4 x 2 subdomains: a coupling operator (ss, nn) whose rows start inside a tile of the global
    numbering (the range's tiles are counted from its own first element), on both paths; with NaN in every value
    outside the column range the result is the same bit for bit"""
    torch = _torch()
    c = grid_case(ctx, "p1_block")
    nb = c.grid.nb
    assert c.local.n_own == grid_case(ctx, "p1").local.n_own and c.grid.n_sub == 8
    pair = None
    for ss in range(c.grid.n_sub):
        a, b = c.grid.subdomain_range(ss, ss + 1)
        if a % 64 == 0:
            continue
        cols = c.col[c.rp[a * nb]:c.rp[b * nb]] // nb
        for nn in range(c.grid.n_sub):
            p, q = c.grid.subdomain_range(nn, nn + 1)
            if nn != ss and ((cols >= p) & (cols < q)).any():
                pair = (ss, nn)
                break
        if pair:
            break
    assert pair is not None, "no coupling operator off a tile boundary"
    ss, nn = pair
    a, b = c.grid.subdomain_range(ss, ss + 1)
    p, q = c.grid.subdomain_range(nn, nn + 1)
    assert a % 64 != 0 and b - a > 64
    rng = (a * nb, b * nb, p * nb, q * nb)
    X = np.random.default_rng(320).standard_normal((3, rng[3] - rng[2]))
    yt, yg = both_paths(ctx, c, X, block=(ss, nn), rng=rng)
    assert yt.shape == (3, rng[1] - rng[0]) and bool(yt.any())
    outside = torch.from_numpy((c.col < rng[2]) | (c.col >= rng[3])).cuda()
    assert bool(outside.any())
    poisoned = [torch.where(outside, torch.full_like(v, float("nan")), v) for v in c.vals]
    xd = strided(X, 5)
    for dm, clean in ((c.dm, yt), (None, yg)):
        y = H.apply(ctx, c.dp, poisoned, xd, dmesh=dm, block=(ss, nn))
        assert bool(torch.isfinite(y).all()) and torch.equal(y, clean)


def test_apply2_at_its_block_cap(ctx, shared_references):
    """apply2 on the p1 case, 2 x 3 vectors.  blocks == 512 (rows > 512 * 1024): every thread of
    apply2_partial_kernel takes more than one row -- four or five, the fifth in a second sweep of the 131,072
    threads that only part of them makes -- and apply2_final_kernel sums 512 partials per pair."""
    torch = _torch()
    c = grid_case(ctx, "p1")
    rows, _, _ = grid_facts(c, "p1")
    assert min(APPLY2_BLOCKS, (rows + 1023) // 1024) == APPLY2_BLOCKS and 4 * APPLY2_BLOCKS * 256 < rows
    r = np.random.default_rng(330)
    V, Uv = r.standard_normal((2, c.n_rows)), r.standard_normal((3, c.n_cols))
    ref, bound = apply2_reference(c.rp, c.col, c.hvals, (c.n_rows, c.n_cols), V, Uv)
    for dm in (c.dm, None):
        got = H.apply2(ctx, c.dp, c.vals, strided(V, 3), strided(Uv, 5), dmesh=dm)
        assert got.shape == (2, 3)
        assert H.last_apply_kernel().startswith("apply_tile_kernel<" if dm is not None else "apply_csr_kernel<")
        err = np.abs(got.cpu().numpy() - ref)
        print("apply2 %s: worst error / bound %.3e" % ("tile" if dm is not None else "csr", (err / bound).max()))
        assert (err <= bound).all(), (err, bound)
        again = H.apply2(ctx, c.dp, c.vals, strided(V, 3), strided(Uv, 5), dmesh=dm)
        assert torch.equal(got, again)


@pytest.mark.parametrize("name", ["p1", "q1", "hex"])
def test_determinism(ctx, name):
    torch = _torch()
    c = grid_case(ctx, name)
    grid_facts(c, name)
    X = strided(np.random.default_rng(340).standard_normal((5, c.n_cols)), 2)
    for dm in (c.dm, None):
        a = H.apply(ctx, c.dp, c.vals, X, dmesh=dm)
        b = H.apply(ctx, c.dp, c.vals, X, dmesh=dm)
        assert torch.equal(a, b)
