"""Operator application with a theta per vector (hdd_operator_apply_multi: H.apply_multi).

The contract: row j of the result is bit for bit what H.apply gives for (thetas[j], X[j]) on the same path (compared
through int64 views).  The tile kernel takes P1 with at most three and Q1 with one value array; what it does not take
runs the CSR kernel even when a mesh is given, and is then compared with H.apply without the mesh.  Against the host
scipy matrix A(theta_j) every row is held to test_gpu_apply's derived bound 2 gamma_K |theta||A||x|.

Shapes: OS2014's two components on a P1 Kuhn grid 12 x 11 (264 elements: 4 tiles + 8 elements), a third component
(kappa = 1) for three LDS images, the two arrays four times over for HDD_MAX_COMP on the CSR path, Q1 13 x 10 (130
elements: 2 tiles + 2), hexahedra Q1 4^3, and the coupling blocks of a 2 x 2 partition.  n_vec 1, 3, 4, 5, 8: a partial
group, a full one, a full and a partial one, two full ones.  mu_j is spread over [0.1, 1]."""
import numpy as np
import pytest

from cases import os2014_components
from test_gpu_apply import Case, check, reference, strided

H = pytest.importorskip("hdd_amd")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

N_VECS = (1, 3, 4, 5, 8)
_CASES = {}


def _torch():
    import torch
    return torch


def bits(t):
    return t.contiguous().view(_torch().int64)


def mus(n):
    return np.linspace(0.1, 1.0, n) if n > 1 else np.array([0.3])


def os2014_kappas(extra=False):
    fns = [H.scalar_fn(H.FN_SINUSOID, a, b, kx, ky, order=3) for (a, b, kx, ky) in os2014_components()]
    # kappa = 1 as a sinusoid of amplitude zero: one assembly takes components of one integration order
    return fns + ([H.scalar_fn(H.FN_SINUSOID, 1.0, 0.0, 0.0, 0.0, order=3)] if extra else [])


def case(ctx, name):
    """the assembled cases, built once per session: OS2014's two components and kappa = 1 as the third"""
    if name not in _CASES:
        if name == "p1":
            c = Case(ctx, H.Grid.structured(H.SIMPLEX, 12, 11, (-1, -1), (1, 1)), kappas=os2014_kappas(True), tensor=H.tensor_fn())
            assert c.n_rows == 3 * 264
        elif name == "q1":
            c = Case(ctx, H.Grid.structured(H.CUBE, 13, 10, (-1, -1), (1, 1)), kappas=os2014_kappas(), tensor=H.tensor_fn())
            assert c.n_rows == 4 * 130
        elif name == "hex":
            c = Case(ctx, H.Grid.structured3d((4, 4, 4), degree=1), tensor=H.tensor_fn(dim=3), prm=H.params_for(1, 3))
        elif name == "p1_block":
            c = Case(ctx, H.Grid.structured(H.SIMPLEX, 16, 16, (-1, -1), (1, 1), px=2, py=2), kappas=os2014_kappas(), tensor=H.tensor_fn())
        else:
            raise KeyError(name)
        _CASES[name] = c
    return _CASES[name]


def thetas_for(n_vec, n_comp):
    """theta_j = (1, mu_j, 1 + mu_j / 2, ...): the affine decomposition's (1, mu) first, distinct in every column"""
    mu = mus(n_vec)
    cols = [np.ones(n_vec), mu] + [1.0 + mu / (q + 1) for q in range(1, n_comp - 1)]
    return np.stack(cols[:n_comp], axis=1) if n_comp > 1 else mu.reshape(-1, 1)


def run(ctx, c, sel, n_vec, dm, tile, block=None, rng=None, seed=0):
    """apply_multi on the value arrays sel of c against H.apply per column (bitwise, same path) and the host"""
    torch = _torch()
    vals = [c.vals[q] for q in sel]
    hvals = [c.hvals[q] for q in sel]
    cols = c.n_cols if rng is None else rng[3] - rng[2]
    X = np.random.default_rng(50 + seed).standard_normal((n_vec, cols))
    th = thetas_for(n_vec, len(sel))
    xd = strided(X, 5)
    Y = H.apply_multi(ctx, c.dp, vals, xd, th, dmesh=dm, block=block)
    name = H.last_apply_kernel()
    assert name.startswith("apply_tile_multi_kernel<" if tile else "apply_csr_multi_kernel<"), name
    assert name.endswith(", 4>"), name                      # the instantiation's vector count, whatever n_vec is
    for j in range(n_vec):
        yj = H.apply(ctx, c.dp, vals, xd[j], theta=th[j], dmesh=dm if tile else None, block=block)
        assert H.last_apply_kernel().startswith("apply_tile_kernel<" if tile else "apply_csr_kernel<")
        assert torch.equal(bits(Y[j]), bits(yj)), (j, int((bits(Y[j]) != bits(yj)).sum()))
        y_ref, bound, _ = reference(c.rp, c.col, hvals, th[j], (c.n_rows, c.n_cols), rng, X[j:j + 1])
        check(Y[j], y_ref, bound, "column %d" % j)
    return Y, name


@pytest.mark.parametrize("n_vec", N_VECS)
@pytest.mark.parametrize("path", ["tile", "csr"])
def test_two_components_p1(ctx, path, n_vec):
    c = case(ctx, "p1")
    _, name = run(ctx, c, (0, 1), n_vec, c.dm if path == "tile" else None, path == "tile")
    assert name == ("apply_tile_multi_kernel<3, 3, 4>" if path == "tile" else "apply_csr_multi_kernel<8, 4>")


@pytest.mark.parametrize("n_vec", N_VECS)
@pytest.mark.parametrize("path", ["tile", "csr"])
def test_three_components_p1(ctx, path, n_vec):
    """three LDS images per wave on the tile path"""
    c = case(ctx, "p1")
    run(ctx, c, (0, 1, 2), n_vec, c.dm if path == "tile" else None, path == "tile", seed=1)


@pytest.mark.parametrize("n_vec", [1, 5])
def test_one_component_p1(ctx, n_vec):
    """one image, read once per entry; scalar theta_j"""
    c = case(ctx, "p1")
    run(ctx, c, (0,), n_vec, c.dm, True, seed=2)


@pytest.mark.parametrize("n_vec", [3, 8])
@pytest.mark.parametrize("n_comp", [4, 8])
def test_more_components_than_images_take_the_csr_kernel(ctx, n_comp, n_vec):
    """the two arrays repeated: with the mesh given, too, the CSR kernel (HDD_MAX_COMP value arrays)"""
    c = case(ctx, "p1")
    for dm in (c.dm, None):
        _, name = run(ctx, c, (0, 1) * (n_comp // 2), n_vec, dm, False, seed=3)
        assert name == "apply_csr_multi_kernel<8, 4>"


@pytest.mark.parametrize("n_vec", N_VECS)
def test_q1(ctx, n_vec):
    """one component: the tile kernel; two: 80 KB of images, the CSR kernel although the mesh is given"""
    c = case(ctx, "q1")
    _, name = run(ctx, c, (0,), n_vec, c.dm, True, seed=4)
    assert name == "apply_tile_multi_kernel<4, 4, 4>"
    _, name = run(ctx, c, (0, 1), n_vec, c.dm, False, seed=5)
    assert name == "apply_csr_multi_kernel<8, 4>"
    run(ctx, c, (0, 1), n_vec, None, False, seed=5)


@pytest.mark.parametrize("n_vec", [1, 5, 8])
def test_hexahedra(ctx, n_vec):
    c = case(ctx, "hex")
    _, name = run(ctx, c, (0,), n_vec, c.dm, False, seed=6)
    assert name == "apply_csr_multi_kernel<64, 4>"


@pytest.mark.parametrize("ss,nn", [(0, 1), (1, 0), (2, 3), (3, 3)])
@pytest.mark.parametrize("path", ["tile", "csr"])
def test_coupling_blocks(ctx, path, ss, nn):
    """the operator (ss, nn) of a 2 x 2 partition in place, x in nn's numbering"""
    c = case(ctx, "p1_block")
    g = c.grid
    (a, b), (d, e) = g.subdomain_range(ss, ss + 1), g.subdomain_range(nn, nn + 1)
    rng = (3 * a, 3 * b, 3 * d, 3 * e)
    Y, _ = run(ctx, c, (0, 1), 5, c.dm if path == "tile" else None, path == "tile", block=(ss, nn), rng=rng, seed=7)
    assert Y.shape == (5, 3 * (b - a))
    if ss != nn:
        assert bool((Y != 0).any())      # input condition: the subdomains are neighbours, the block is not empty


@pytest.mark.parametrize("name,sel", [("p1", (0, 1, 2)), ("q1", (0,)), ("q1", (0, 1)), ("hex", (0,))])
def test_no_thetas_is_the_multi_vector_apply(ctx, name, sel):
    torch = _torch()
    c = case(ctx, name)
    vals = [c.vals[q] for q in sel]
    for n_vec in (1, 5):
        xd = strided(np.random.default_rng(60).standard_normal((n_vec, c.n_cols)), 3)
        for dm in (c.dm, None):
            Y = H.apply_multi(ctx, c.dp, vals, xd, None, dmesh=dm)
            tile = H.last_apply_kernel().startswith("apply_tile_multi")
            Yr = H.apply(ctx, c.dp, vals, xd, dmesh=dm if tile else None)
            assert torch.equal(bits(Y), bits(Yr)), (n_vec, dm is None)


def test_out_argument_and_rejects(ctx):
    torch = _torch()
    c = case(ctx, "p1")
    X = torch.from_numpy(np.random.default_rng(61).standard_normal((3, c.n_cols))).cuda()
    th = thetas_for(3, 2)
    out = torch.full((3, c.n_rows + 4), float("nan"), dtype=torch.float64, device="cuda")
    Y = H.apply_multi(ctx, c.dp, c.vals[:2], X, th, dmesh=c.dm, out=out[:, :c.n_rows])
    assert Y.data_ptr() == out.data_ptr() and bool(torch.isnan(out[:, c.n_rows:]).all())
    assert torch.equal(bits(Y), bits(H.apply_multi(ctx, c.dp, c.vals[:2], X, th, dmesh=c.dm)))
    for bad in (th[:2], th[:, :1], np.ones((3, 3))):
        with pytest.raises(H.HddError):
            H.apply_multi(ctx, c.dp, c.vals[:2], X, bad, dmesh=c.dm)
    with pytest.raises(H.HddError):
        H.apply_multi(ctx, c.dp, c.vals[:2], X[0], th[:1], dmesh=c.dm)            # one dimension
