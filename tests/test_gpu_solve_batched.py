"""The batched device solve (hdd_operator_solve_batched: H.solve_batched) against the single solve, column by column.

The contract: column j of a batch ends with exactly the x, iterations, status, residual, rhs_norm and history that
H.solve gives for (b_j, x0_j) with the same options -- bit for bit (x is compared through an int64 view, the doubles
of the info for equality), whatever the other columns hold, however the columns fall into groups of four, and
whatever check_every is.  The single solve is the oracle; test_gpu_solve.py pins it against host matrices, and
check_solution's assertions are repeated here per column of the batch.

Columns: b_j = A xs_j on the host for xs_0 the case's own vector, xs_1 a smooth one (a product of two low-frequency
cosines of the row number) and xs_2.. further random ones.  Input condition, asserted from the single solves: the
iteration counts within a batch take at least two distinct values, so that a column is frozen while others go on.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_solve import RTOL, check_solution, dev, numpy_pcg, problem

H = pytest.importorskip("hdd_amd")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def kernels(apply, bs, pre=True):
    """the spelling hdd.h documents: the vector count is that of the instantiation (4), not n_rhs"""
    return "%s + cg_update<%d, %s4> + cg_direction<4>" % (apply, bs, "" if pre else "none, ")


TILE_P1, TILE_Q1 = "apply_tile_kernel<3, 3, 4, dot>", "apply_tile_kernel<4, 4, 4, dot>"
CSR8, CSR64 = "apply_csr_kernel<8, 4, dot>", "apply_csr_kernel<64, 4, dot>"

_COLUMNS = {}


def smooth(n):
    i = (np.arange(n) + 0.5) / n
    return np.cos(np.pi * i) * np.cos(3.0 * np.pi * i)


def columns(P, name, n):
    """(XS, B) [n, rows]: the first n of the case's eight columns (computed once)"""
    if name not in _COLUMNS:
        rows = P.A.shape[0]
        xs = [P.xs, smooth(rows)] + [np.random.default_rng(100 + j).standard_normal(rows) for j in range(6)]
        XS = np.stack(xs)
        B = np.stack([P.A @ x for x in xs])
        assert np.array_equal(B[0], P.b)
        _COLUMNS[name] = (XS, B, {})
    XS, B, _ = _COLUMNS[name]
    return XS[:n], B[:n]


def ref_iterations(P, name, j, bs):
    XS, B, ref = _COLUMNS[name]
    if (j, bs) not in ref:
        ref[j, bs] = P.ref_iterations(bs) if j == 0 else numpy_pcg(P.A, B[j], bs, RTOL)[1]
    return ref[j, bs]


def bits(t):
    return t.contiguous().view(_torch().int64)


def same_info(a, b):
    """iterations, status, residual, rhs_norm and the history for equality (NaN residuals by their bits)"""
    fa = np.array([a.residual, a.rhs_norm]).view(np.int64)
    fb = np.array([b.residual, b.rhs_norm]).view(np.int64)
    ok = (a.status, a.iterations) == (b.status, b.iterations) and np.array_equal(fa, fb)
    if a.history is not None or b.history is not None:
        ok = ok and a.history.shape == b.history.shape and bool(_torch().equal(bits(a.history), bits(b.history)))
    return ok


def assert_columns_equal_singles(X, infos, singles, what=""):
    torch = _torch()
    assert X.shape[0] == len(infos) == len(singles)
    for j, (x1, i1) in enumerate(singles):
        print("%s column %d: batched %d iterations status %d residual %.3e | single %d iterations status %d residual %.3e"
              % (what, j, infos[j].iterations, infos[j].status, infos[j].residual, i1.iterations, i1.status, i1.residual))
    for j, (x1, i1) in enumerate(singles):
        assert torch.equal(bits(X[j]), bits(x1)), (what, j, int((bits(X[j]) != bits(x1)).sum()))
        assert same_info(infos[j], i1), (what, j, (infos[j].status, infos[j].iterations, infos[j].residual, infos[j].rhs_norm),
                                         (i1.status, i1.iterations, i1.residual, i1.rhs_norm))


def run_both(ctx, c, B, dm, X0=None, **kw):
    """the batch and, after it, its single solves: X, infos, [(x_j, info_j)], the batch's kernel names"""
    Bd = dev(B)
    X, infos = H.solve_batched(ctx, c.dp, c.vals, Bd, dmesh=dm, X0=None if X0 is None else dev(X0), history=True, **kw)
    names = H.last_solve_kernels()
    singles = [H.solve(ctx, c.dp, c.vals, Bd[j], dmesh=dm, x0=None if X0 is None else dev(X0[j]), history=True, **kw)
               for j in range(B.shape[0])]
    return X, infos, singles, names


CASES = [("p1", "tile", 0, kernels(TILE_P1, 3)), ("p1", "csr", 0, kernels(CSR8, 3)),
         ("q1", "tile", 0, kernels(TILE_Q1, 4)), ("q1", "csr", 0, kernels(CSR8, 4)),
         ("os2014", "tile", 0, kernels(TILE_P1, 3)), ("hex_q1", "csr", 8, kernels(CSR64, 8)),
         ("hex_q2", "csr", 1, kernels(CSR64, 1))]
SHAPES = [(c, n) for c in CASES for n in ((1, 2, 3, 4, 5, 8) if c[:2] == ("p1", "tile") else (3, 8))]


@pytest.mark.parametrize("case,n_rhs", SHAPES, ids=["%s-%s-%d" % (c[0], c[1], n) for c, n in SHAPES])
def test_columns_are_the_single_solves(ctx, case, n_rhs):
    """every path of the single solve's dispatch; a partial group (1, 2, 3), a full one (4), a full and a partial one
    (5), two full ones (8)"""
    name, path, bs, expected = case
    P = problem(ctx, name)
    c = P.c
    XS, B = columns(P, name, n_rhs)
    X, infos, singles, names = run_both(ctx, c, B, c.dm if path == "tile" else None, theta=P.theta, block_size=bs, rtol=RTOL)
    assert names == expected
    assert X.shape == (n_rhs, c.n_rows)
    assert_columns_equal_singles(X, infos, singles, "%s %s" % (name, path))
    if n_rhs > 1:   # input condition: some column is frozen while others iterate
        assert len({i.iterations for _, i in singles}) >= 2, [i.iterations for _, i in singles]
    for j in range(n_rhs):
        check_solution(P.A, P.lmin, B[j], XS[j], X[j], infos[j], ref_iterations(P, name, j, P.bs))


@pytest.mark.parametrize("path", ["tile", "csr"])
def test_zero_column_in_the_middle(ctx, path):
    torch = _torch()
    P = problem(ctx, "p1")
    c = P.c
    _, B = columns(P, "p1", 5)
    B = B.copy()
    B[2] = 0.0
    X0 = np.stack([np.full(c.n_rows, 0.25)] * 5)     # b = 0 gives x = 0 whatever the initial guess was
    for x0 in (None, X0):
        X, infos, singles, _ = run_both(ctx, c, B, c.dm if path == "tile" else None, X0=x0, rtol=RTOL)
        assert not bool(bits(X[2]).any())            # exactly +0.0
        assert (infos[2].status, infos[2].iterations, infos[2].residual, infos[2].rhs_norm) == (H.SOLVE_CONVERGED, 0, 0.0, 0.0)
        assert_columns_equal_singles(X, infos, singles, "zero column")
        for j in (0, 1, 3, 4):
            assert infos[j].status == H.SOLVE_CONVERGED and infos[j].iterations > 0


@pytest.mark.parametrize("name,path,col", [("p1", "tile", 1), ("p1", "csr", 3), ("q1", "tile", 4)])
def test_nan_stays_in_its_column(ctx, name, path, col):
    torch = _torch()
    P = problem(ctx, name)
    c = P.c
    _, B = columns(P, name, 5)
    B = B.copy()
    B[col, 7] = float("nan")
    X, infos, singles, _ = run_both(ctx, c, B, c.dm if path == "tile" else None, rtol=RTOL)
    assert_columns_equal_singles(X, infos, singles, "NaN column")
    assert (singles[col][1].status, singles[col][1].iterations) == (H.SOLVE_BREAKDOWN, 0)
    assert (infos[col].status, infos[col].iterations) == (H.SOLVE_BREAKDOWN, 0)
    for j in range(5):
        if j != col:
            assert bool(torch.isfinite(X[j]).all()) and infos[j].status == H.SOLVE_CONVERGED


def test_nan_during_the_iteration_stays_in_its_column(ctx):
    """a NaN that enters through x0 (r0 = b - A x0): the same isolation with the warm-start apply in the way"""
    torch = _torch()
    P = problem(ctx, "p1")
    c = P.c
    XS, B = columns(P, "p1", 3)
    X0 = 0.5 * XS
    X0[1, 100] = float("nan")
    X, infos, singles, _ = run_both(ctx, c, B, c.dm, X0=X0, rtol=RTOL)
    assert infos[1].status == H.SOLVE_BREAKDOWN
    assert_columns_equal_singles(X, infos, singles, "NaN in x0")
    for j in (0, 2):
        assert bool(torch.isfinite(X[j]).all()) and infos[j].status == H.SOLVE_CONVERGED


def test_indefinite_block_breaks_every_column_down(ctx):
    torch = _torch()
    E = problem(ctx, "esv8")
    c = E.c
    assert E.lmin > 0
    _, B = columns(E, "esv8", 3)
    for dm in (c.dm, None):
        X, infos, singles, _ = run_both(ctx, c, B, dm, theta=[-1.0], rtol=RTOL)
        assert [(i.status, i.iterations) for i in infos] == [(H.SOLVE_BREAKDOWN, 0)] * 3
        assert_columns_equal_singles(X, infos, singles, "-A")
        assert bool(torch.isfinite(X).all())
    # without the preconditioner the breakdown is p . Ap <= 0 in the first iteration, per column
    X, infos, singles, _ = run_both(ctx, c, B, c.dm, theta=[-1.0], precond="none", rtol=RTOL)
    assert [(i.status, i.iterations) for i in infos] == [(H.SOLVE_BREAKDOWN, 0)] * 3 and not bool(X.any())
    assert_columns_equal_singles(X, infos, singles, "-A, none")


@pytest.mark.parametrize("path", ["tile", "csr"])
def test_max_iter(ctx, path):
    P = problem(ctx, "p1")
    c = P.c
    _, B = columns(P, "p1", 5)
    for max_iter in (5, 0):
        X, infos, singles, _ = run_both(ctx, c, B, c.dm if path == "tile" else None, rtol=RTOL, max_iter=max_iter)
        assert [(i.status, i.iterations) for i in infos] == [(H.SOLVE_MAX_ITER, max_iter)] * 5
        assert_columns_equal_singles(X, infos, singles, "max_iter %d" % max_iter)


def _raw_batched(ctx, c, B, dm, bs, ldb=None, ldx=None, shift=0, X0=None, rtol=RTOL, max_iter=10000, check_every=0,
                 history=False):
    """hdd_operator_solve_batched through ctypes: b with row stride ldb inside NaN; x with row stride ldx and the
    workspace `shift` doubles past a 16-byte boundary, inside NaN.  Returns X [n_rhs, rows], the info tuples and the
    whole history [n_rhs, max_iter + 1] after checking that nothing around x (its padding beyond `rows` included)
    and the workspace was written."""
    torch = _torch()
    n_rhs, rows = B.shape
    ldb, ldx = ldb or rows, ldx or rows
    n_work = int(H.lib().hdd_operator_solve_batched_workspace(rows, bs, n_rhs))
    nan = float("nan")
    bbuf = torch.full((n_rhs, ldb), nan, dtype=torch.float64, device="cuda")
    bbuf[:, :rows] = dev(B)
    xbuf = torch.full((n_rhs * ldx + 8,), nan, dtype=torch.float64, device="cuda")
    wbuf = torch.full((n_work + 8,), nan, dtype=torch.float64, device="cuda")
    x, w = xbuf[2 + shift:2 + shift + n_rhs * ldx], wbuf[2 + shift:2 + shift + n_work]
    assert x.data_ptr() % 16 == 8 * shift and w.data_ptr() % 16 == 8 * shift
    X = x.view(n_rhs, ldx)
    flags = 0
    if X0 is not None:
        X[:, :rows] = dev(X0)
        flags = H.SOLVE_X0
    ldh = max_iter + 1
    hist = torch.zeros((n_rhs, ldh), dtype=torch.float64, device="cuda") if history else None
    ptrs = (C.c_void_p * len(c.vals))(*[v.data_ptr() for v in c.vals])
    opt = H.SolveOptions(rtol, 0.0, max_iter, check_every, H.PRECOND_BLOCK_JACOBI, bs, flags, 0)
    infos = (H.SolveInfo * n_rhs)()
    rc = H.lib().hdd_operator_solve_batched(ctx.h, None if dm is None else C.addressof(dm.t), C.addressof(c.dp.t), ptrs,
                                            len(c.vals), None, None, bbuf.data_ptr(), ldb, x.data_ptr(), ldx, n_rhs,
                                            C.addressof(opt), w.data_ptr(), n_work,
                                            None if hist is None else hist.data_ptr(), ldh, C.addressof(infos),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, H.lib().hdd_last_error(None)
    torch.cuda.synchronize()
    for buf, n in ((xbuf, n_rhs * ldx), (wbuf, n_work)):
        assert bool(torch.isnan(buf[:2 + shift]).all()) and bool(torch.isnan(buf[2 + shift + n:]).all())
    if ldx > rows:
        assert bool(torch.isnan(X[:, rows:]).all())            # the sentinel in the padding of every column
    assert bool(torch.isnan(bbuf[:, rows:]).all()) and torch.equal(bbuf[:, :rows], dev(B))
    return X[:, :rows].clone(), [(i.status, i.iterations, i.residual, i.rhs_norm) for i in infos], hist


def test_frozen_columns_and_their_history(ctx):
    """rtol = 1e-2; column 0 starts at 0.98 xs_0 (its residual is 0.02 ||b||, a factor of two from the threshold),
    the others at zero: it ends several times sooner, and nothing of it is touched afterwards"""
    torch = _torch()
    P = problem(ctx, "p1")
    c = P.c
    XS, B = columns(P, "p1", 4)
    X0 = np.zeros_like(XS)
    X0[0] = 0.98 * XS[0]
    singles = [H.solve(ctx, c.dp, c.vals, dev(B[j]), dmesh=c.dm, x0=dev(X0[j]), rtol=1e-2, history=True) for j in range(4)]
    its = [i.iterations for _, i in singles]
    print("iterations of the single solves:", its)
    assert all(i.status == H.SOLVE_CONVERGED for _, i in singles)
    assert 0 < 2 * its[0] < min(its[1:]), its                # input condition: more than a factor of two apart
    X, infos, hist = _raw_batched(ctx, c, B, c.dm, 3, X0=X0, rtol=1e-2, history=True)
    for j, (x1, i1) in enumerate(singles):
        assert torch.equal(bits(X[j]), bits(x1)), j
        assert infos[j] == (i1.status, i1.iterations, i1.residual, i1.rhs_norm), j
        assert torch.equal(bits(hist[j, :its[j] + 1]), bits(i1.history)), j
        assert not bool(bits(hist[j, its[j] + 1:]).any()), j       # beyond its own count: untouched zeros
    # the front end gives the same
    Xf, infos_f = H.solve_batched(ctx, c.dp, c.vals, dev(B), dmesh=c.dm, X0=dev(X0), rtol=1e-2, history=True)
    assert_columns_equal_singles(Xf, infos_f, singles, "rtol 1e-2")


@pytest.mark.parametrize("name,path", [("p1", "tile"), ("q1", "csr")])
def test_check_every(ctx, name, path):
    """1, 7 or 32 (the default) iterations enqueued between two looks: the same bits in every column"""
    torch = _torch()
    P = problem(ctx, name)
    c = P.c
    _, B = columns(P, name, 5)
    dm = c.dm if path == "tile" else None
    runs = [H.solve_batched(ctx, c.dp, c.vals, dev(B), dmesh=dm, rtol=RTOL, check_every=ce, history=True) for ce in (1, 7, 0)]
    X1, I1 = runs[0]
    assert all(i.status == H.SOLVE_CONVERGED and i.iterations > 32 for i in I1)
    for X, I in runs[1:]:
        assert torch.equal(bits(X), bits(X1))
        assert all(same_info(a, b) for a, b in zip(I, I1))
    singles = [H.solve(ctx, c.dp, c.vals, dev(B[j]), dmesh=dm, rtol=RTOL, check_every=50, history=True) for j in range(5)]
    assert_columns_equal_singles(X1, I1, singles, "check_every")


@pytest.mark.parametrize("name,path,bs", [("p1", "tile", 2), ("p1", "csr", 3), ("q1", "tile", 4), ("p1", "tile", 8)])
@pytest.mark.parametrize("n_rhs", [3, 5])
def test_leading_dimensions_and_alignment(ctx, name, path, bs, n_rhs):
    """ldb, ldx = rows + 1 (odd: every other column of x is 8 bytes off) and rows + 6; x and the workspace 8 bytes
    off a 16-byte boundary (the scalar-load instantiations of the even block sizes): the bits of the aligned,
    densely packed call, and the padding of x keeps its sentinel (checked in _raw_batched)"""
    torch = _torch()
    P = problem(ctx, name)
    c = P.c
    rows = c.n_rows
    assert rows % bs == 0
    _, B = columns(P, name, n_rhs)
    dm = c.dm if path == "tile" else None
    Xa, ia, _ = _raw_batched(ctx, c, B, dm, bs)
    assert H.last_solve_kernels().endswith("cg_update<%d, 4> + cg_direction<4>" % bs)
    assert all(i[0] == H.SOLVE_CONVERGED for i in ia) and bool(torch.isfinite(Xa).all())
    for ldb, ldx, shift in [(rows + 1, rows + 1, 0), (rows + 6, rows + 6, 0), (rows, rows, 1), (rows + 1, rows + 6, 1),
                            (rows + 6, rows + 1, 1)]:
        X, i, _ = _raw_batched(ctx, c, B, dm, bs, ldb=ldb, ldx=ldx, shift=shift)
        assert torch.equal(bits(X), bits(Xa)), (ldb, ldx, shift)
        assert i == ia, (ldb, ldx, shift)
    singles = [H.solve(ctx, c.dp, c.vals, dev(B[j]), dmesh=dm, block_size=bs, rtol=RTOL) for j in range(n_rhs)]
    for j, (x1, i1) in enumerate(singles):
        assert torch.equal(bits(Xa[j]), bits(x1)) and ia[j] == (i1.status, i1.iterations, i1.residual, i1.rhs_norm), j


def test_strided_right_hand_sides_through_the_front_end(ctx):
    """B as a view with a row stride: the stride is ldb"""
    torch = _torch()
    P = problem(ctx, "q1")
    c = P.c
    _, B = columns(P, "q1", 3)
    buf = torch.full((3, c.n_rows + 5), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :c.n_rows] = dev(B)
    X, infos = H.solve_batched(ctx, c.dp, c.vals, buf[:, :c.n_rows], dmesh=c.dm, rtol=RTOL)
    Xd, infos_d = H.solve_batched(ctx, c.dp, c.vals, dev(B), dmesh=c.dm, rtol=RTOL)
    assert torch.equal(bits(X), bits(Xd)) and all(same_info(a, b) for a, b in zip(infos, infos_d))
    assert all(i.status == H.SOLVE_CONVERGED for i in infos)
    assert bool(torch.isnan(buf[:, c.n_rows:]).all())


def _local_problem(P, ss, nb, n_rhs, seed):
    a, b = P.c.grid.subdomain_range(ss, ss + 1)
    A = P.A[nb * a:nb * b, nb * a:nb * b].tocsr()
    lmin = float(np.linalg.eigvalsh(A.toarray())[0])
    XS = np.stack([smooth(A.shape[0])] + [np.random.default_rng(seed + j).standard_normal(A.shape[0]) for j in range(n_rhs - 1)])
    return A, lmin, XS, np.stack([A @ x for x in XS])


@pytest.mark.parametrize("path", ["tile", "csr"])
@pytest.mark.parametrize("ss", [0, 1, 2, 3])
def test_local_solves(ctx, ss, path):
    """SPE10 Kuhn 40 x 8 in 2 x 2 subdomains: three right-hand sides on get_local_operator(ss) through the block range"""
    P = problem(ctx, "p1_block")
    c = P.c
    A, lmin, XS, B = _local_problem(P, ss, 3, 3, 200 + 10 * ss)
    X, infos, singles, names = run_both(ctx, c, B, c.dm if path == "tile" else None, block=(ss, ss), rtol=RTOL)
    assert names == kernels(TILE_P1 if path == "tile" else CSR8, 3)
    assert X.shape == B.shape
    assert_columns_equal_singles(X, infos, singles, "local %d" % ss)
    for j in range(3):
        check_solution(A, lmin, B[j], XS[j], X[j], infos[j], numpy_pcg(A, B[j], 3, RTOL)[1])


@pytest.mark.parametrize("ss", [0, 1])
def test_local_solves_hexahedra(ctx, ss):
    P = problem(ctx, "hex_block")
    c = P.c
    assert c.grid.n_sub == 2 and c.grid.nb == 8
    A, lmin, XS, B = _local_problem(P, ss, 8, 2, 300 + 10 * ss)
    X, infos, singles, names = run_both(ctx, c, B, c.dm, block=(ss, ss), block_size=8, rtol=RTOL)
    assert names == kernels(CSR64, 8)
    assert_columns_equal_singles(X, infos, singles, "hex local %d" % ss)
    for j in range(2):
        check_solution(A, lmin, B[j], XS[j], X[j], infos[j], numpy_pcg(A, B[j], 8, RTOL)[1])


@pytest.mark.parametrize("name,path", [("p1", "tile"), ("q1", "csr")])
def test_initial_guesses_per_column(ctx, name, path):
    """every column of X0 is that column's initial guess: a good one, zero, a random one, the solution itself"""
    P = problem(ctx, name)
    c = P.c
    XS, B = columns(P, name, 5)
    X0 = np.zeros_like(XS)
    X0[0] = XS[0] * (1.0 + 1e-5)
    X0[2] = np.random.default_rng(9).standard_normal(c.n_rows)
    X0[3] = XS[3]
    X0[4] = 0.5 * XS[4]
    X, infos, singles, _ = run_both(ctx, c, B, c.dm if path == "tile" else None, X0=X0, rtol=RTOL)
    assert_columns_equal_singles(X, infos, singles, "X0")
    assert infos[3].iterations == 0 and all(i.status == H.SOLVE_CONVERGED for i in infos)
    assert len({i.iterations for i in infos}) >= 3
    for j in range(5):
        assert np.linalg.norm(B[j] - P.A @ X[j].cpu().numpy()) <= 2 * RTOL * np.linalg.norm(B[j])


def test_no_preconditioner(ctx):
    P = problem(ctx, "p1")
    c = P.c
    XS, B = columns(P, "p1", 4)
    X, infos, singles, names = run_both(ctx, c, B, c.dm, precond="none", block_size=1, rtol=RTOL)
    assert names == kernels(TILE_P1, 1, pre=False)
    assert_columns_equal_singles(X, infos, singles, "none")
    assert len({i.iterations for i in infos}) >= 2
    pre = H.solve(ctx, c.dp, c.vals, dev(B[0]), dmesh=c.dm, rtol=RTOL)[1]
    assert infos[0].iterations > pre.iterations          # it is the iteration without the preconditioner
    for j in range(4):
        if infos[j].status == H.SOLVE_CONVERGED:
            assert np.linalg.norm(B[j] - P.A @ X[j].cpu().numpy()) <= 2 * RTOL * np.linalg.norm(B[j])


def test_front_end_rejects(ctx):
    torch = _torch()
    P = problem(ctx, "p1")
    c = P.c
    _, B = columns(P, "p1", 2)
    with pytest.raises(H.HddError):
        H.solve_batched(ctx, c.dp, c.vals, dev(B[0]), dmesh=c.dm)                    # one dimension
    with pytest.raises(H.HddError):
        H.solve_batched(ctx, c.dp, c.vals, dev(B)[:, :-3], dmesh=c.dm)               # the wrong number of rows
    with pytest.raises(H.HddError):
        H.solve_batched(ctx, c.dp, c.vals, torch.zeros((9, c.n_rows), dtype=torch.float64, device="cuda"), dmesh=c.dm)
    with pytest.raises(H.HddError):
        H.solve_batched(ctx, c.dp, c.vals, dev(B), dmesh=c.dm, X0=dev(B[:1]))
