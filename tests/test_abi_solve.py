"""The solver entry points of the C ABI (hdd_operator_solve, hdd_operator_solve_workspace, hdd_last_solve_kernels):
declared, exported, bound by the Python front-end, and every argument check comes before the first device call -- so
they answer HDD_ERR_INVALID (1) here, without a GPU.  The pointers that stand for the context and the device arrays
are never dereferenced by a rejected call."""
import ctypes as C

import numpy as np

import hdd_amd as H

NAMES = ("hdd_operator_solve", "hdd_operator_solve_workspace", "hdd_last_solve_kernels")


def test_symbols_exported_and_bound():
    L = H.lib()
    declared = H.declared_symbols()
    for n in NAMES:
        assert n in declared, n
        assert getattr(L, n).argtypes is not None, n
    assert L.hdd_last_solve_kernels.restype is C.c_char_p
    assert L.hdd_operator_solve_workspace.restype is C.c_int64
    assert isinstance(H.last_solve_kernels(), str)
    assert callable(H.solve)
    assert (H.PRECOND_NONE, H.PRECOND_BLOCK_JACOBI) == (0, 1)
    assert (H.SOLVE_CONVERGED, H.SOLVE_MAX_ITER, H.SOLVE_BREAKDOWN) == (0, 1, 2)
    assert C.sizeof(H.SolveOptions) == 40 and C.sizeof(H.SolveInfo) == 24
    assert L.hdd_abi_version() == 8        # additive: the ABI version stays


def test_workspace_size():
    ws = H.lib().hdd_operator_solve_workspace
    for bs in range(0, 9):
        sizes = [ws(24 * k, bs) for k in (0, 1, 2, 10, 1000)]
        assert all(s > 0 for s in sizes), bs
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[-1], bs
    # p, q, r, z and the packed inverse blocks at least
    assert ws(2400, 3) >= 4 * 2400 + 2400 // 3 * 6
    assert ws(2400, 0) >= max(ws(2400, bs) for bs in range(1, 9))   # the mesh's nb is unknown to this function
    assert ws(-1, 3) == 0 and ws(24, 9) == 0 and ws(24, -1) == 0


class _Operands:
    """valid-looking host descriptors; `fake` stands for a context / device array"""

    def __init__(self, n_rows=12, n_cols=12):
        self.keep = np.zeros(64)
        self.fake = self.keep.ctypes.data
        self.pat = H.CsrT(n_rows, n_cols, 48, self.fake, self.fake, self.fake)
        self.vals = (C.c_void_p * 1)(self.fake)
        self.opt = H.SolveOptions(1e-8, 0.0, 100, 0, H.PRECOND_BLOCK_JACOBI, 3, 0, 0)
        self.info = H.SolveInfo()
        # a P1 mesh of 4 elements (12 rows); nothing in it is dereferenced by a rejected call
        self.mesh = H.MeshT(H.SIMPLEX, 1, 4, 0, 4, self.fake, self.fake, self.fake, None, None)

    def solve(self, ctx="fake", pattern="pat", vals="vals", b="fake", x="fake", opt="opt", work="fake", info="info",
              n_comp=1, n_work=None, rng=None, mesh=None, history=None):
        def g(k):
            if k is None:
                return None
            if k in ("pat", "opt", "info"):
                return C.addressof(getattr(self, k))
            return getattr(self, k)
        if n_work is None:
            n_work = H.lib().hdd_operator_solve_workspace(12, 8)
        return H.lib().hdd_operator_solve(g(ctx), None if mesh is None else C.addressof(mesh), g(pattern), g(vals), n_comp,
                                          None, None if rng is None else C.addressof(rng), g(b), g(x), g(opt), g(work),
                                          n_work, history, g(info), None)


def _msg():
    return H.lib().hdd_last_error(None)


def test_rejects_null_arguments():
    o = _Operands()
    for k in ("ctx", "pattern", "vals", "b", "x", "opt", "work", "info"):
        assert o.solve(**{k: None}) == 1, k
        assert _msg().startswith(b"hdd_operator_solve:"), k
    o.vals[0] = None                      # a null value array inside d_vals
    assert o.solve() == 1
    assert H.lib().hdd_operator_solve(None, None, None, None, 1, None, None, None, None, None, None, 0, None, None,
                                      None) == 1


def test_operator_checks_are_those_of_apply():
    o = _Operands()
    for n in (0, H.MAX_COMP + 1):
        assert o.solve(n_comp=n) == 1 and b"n_comp" in _msg()
    assert o.solve(rng=H.BlockRange(0, 13, 0, 13)) == 1 and b"range" in _msg()


def test_range_must_be_square_and_diagonal():
    o = _Operands()
    for r in [(0, 6, 6, 12), (0, 6, 0, 12), (0, 12, 0, 6), (3, 9, 0, 6)]:
        assert o.solve(rng=H.BlockRange(*r)) == 1, r
        assert b"square" in _msg()
    wide = _Operands(n_rows=12, n_cols=15)        # the whole matrix must be square
    assert wide.solve() == 1 and b"square" in _msg()


def test_options():
    for field, bad, word in [("max_iter", -1, b"max_iter"), ("rtol", -1e-3, b"rtol"), ("rtol", float("nan"), b"rtol"),
                             ("atol", -1.0, b"atol"), ("atol", float("nan"), b"atol"), ("precond", 2, b"precond"),
                             ("precond", -1, b"precond"), ("block_size", 9, b"block_size"),
                             ("block_size", -1, b"block_size"), ("check_every", -1, b"check_every")]:
        o = _Operands()
        setattr(o.opt, field, bad)
        assert o.solve() == 1, (field, bad)
        assert word in _msg() and _msg().startswith(b"hdd_operator_solve:"), (field, bad, _msg())


def test_block_size():
    o = _Operands()
    o.opt.block_size = 0                         # no mesh to take nb from
    assert o.solve() == 1 and b"block_size" in _msg()
    hexq2 = H.MeshT(H.HEX, 2, 4, 0, 4, o.fake, o.fake, o.fake, None, None)   # nb = 27 > 8
    assert o.solve(mesh=hexq2) == 1
    for bs in (5, 7, 8):                         # 12 rows are no multiple
        o.opt.block_size = bs
        assert o.solve() == 1 and b"multiples" in _msg(), bs
    o.opt.block_size = 4                         # the bounds of a range, not only its length
    assert o.solve(rng=H.BlockRange(2, 10, 2, 10)) == 1 and b"multiples" in _msg()


def test_workspace_too_small_explicit_and_implied_block_size():
    """n_work is checked against the block size the call resolves: block_size 0 on a P1 mesh needs what block_size 3
    needs"""
    need = H.lib().hdd_operator_solve_workspace(12, 3)
    o = _Operands()
    assert o.solve(n_work=need - 1) == 1 and b"n_work" in _msg()
    assert o.solve(n_work=0) == 1 and b"n_work" in _msg()
    o.opt.block_size = 0
    assert o.solve(mesh=o.mesh, n_work=need - 1) == 1 and b"n_work" in _msg()
