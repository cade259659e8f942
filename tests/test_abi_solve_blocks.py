"""The entry points for every segment of a partition per call (hdd_operator_solve_blocks, its workspace function,
hdd_operator_apply_blocks): declared, exported, bound by the Python front-end, additive to ABI 8, and every argument
check comes before the first device call -- so they answer HDD_ERR_INVALID (1) here, without a GPU.  The pointers that
stand for the context and the device arrays are never dereferenced by a rejected call."""
import ctypes as C

import numpy as np

import hdd_amd as H

NAMES = ("hdd_operator_solve_blocks", "hdd_operator_solve_blocks_workspace", "hdd_operator_apply_blocks")
WHO = b"hdd_operator_solve_blocks:"
WHO_APPLY = b"hdd_operator_apply_blocks:"


def test_symbols_exported_and_bound():
    L = H.lib()
    declared = H.declared_symbols()
    for n in NAMES:
        assert n in declared, n
        assert getattr(L, n).argtypes is not None, n
    assert L.hdd_operator_solve_blocks_workspace.restype is C.c_int64
    assert len(L.hdd_operator_solve_blocks.argtypes) == 17
    assert len(L.hdd_operator_apply_blocks.argtypes) == 11
    assert callable(H.solve_blocks) and callable(H.apply_blocks)
    assert H.MAX_SOLVE_BLOCKS == 4096
    assert "#define HDD_MAX_SOLVE_BLOCKS 4096" in open(H.HEADER).read()
    assert L.hdd_abi_version() == 8        # additive: the ABI version stays


def test_workspace_size():
    ws = H.lib().hdd_operator_solve_blocks_workspace
    for bs in range(0, 9):
        for n in (1, 4, 64, H.MAX_SOLVE_BLOCKS):
            sizes = [ws(24 * k, bs, n) for k in (0, 1, 2, 10, 1000, 100000)]
            assert all(s > 0 for s in sizes), (bs, n)
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[-1], (bs, n)
        by_n = [ws(2400, bs, n) for n in (1, 2, 3, 16, 17, 1000, H.MAX_SOLVE_BLOCKS)]
        assert all(a < b for a, b in zip(by_n, by_n[1:])), bs
    for n in (1, 7, H.MAX_SOLVE_BLOCKS):
        # p, q, r, z of the interval and the packed inverse blocks
        assert ws(2400, 3, n) >= 4 * 2400 + 2400 // 3 * 6
        assert ws(2400, 8, n) >= 4 * 2400 + 2400 // 8 * 36
        # ... and a state, a table entry and the bounds of the partial sums per segment: rows / 4 + n of the apply,
        # four kinds of rows / (256 bs) + n of the update
        assert ws(2400, 3, n) >= 4 * 2400 + 2400 // 3 * 6 + 16 * n + (2400 // 4 + n) + 4 * (2400 // (256 * 3) + n)
        assert ws(2400, 0, n) >= max(ws(2400, bs, n) for bs in range(1, 9))   # covers every block size
    # a function of (rows, block_size, n_blocks) alone
    assert ws(2400, 3, 5) == ws(2400, 3, 5)
    for n in (0, -1, H.MAX_SOLVE_BLOCKS + 1):
        assert ws(24, 3, n) == 0, n
    assert ws(-1, 3, 2) == 0 and ws(24, 9, 2) == 0 and ws(24, -1, 2) == 0


class _Operands:
    """valid-looking host descriptors; `fake` stands for a context / device array"""

    def __init__(self, n_rows=12, n_cols=12):
        self.keep = np.zeros(64)
        self.fake = self.keep.ctypes.data
        self.pat = H.CsrT(n_rows, n_cols, 48, self.fake, self.fake, self.fake)
        self.vals = (C.c_void_p * 1)(self.fake)
        self.opt = H.SolveOptions(1e-8, 0.0, 100, 0, H.PRECOND_BLOCK_JACOBI, 3, 0, 0)
        self.info = (H.SolveInfo * 8)()
        self.mesh = H.MeshT(H.SIMPLEX, 1, 4, 0, 4, self.fake, self.fake, self.fake, None, None)

    def _g(self, k):
        if k is None:
            return None
        if k in ("pat", "opt", "info"):
            return C.addressof(getattr(self, k))
        return getattr(self, k)

    def solve(self, ctx="fake", pattern="pat", vals="vals", b="fake", x="fake", opt="opt", work="fake", info="info",
              n_comp=1, n_work=None, mesh=None, history=None, ldh=101, bounds=(0, 6, 12), n_blocks=None):
        g = self._g
        bd = None if bounds is None else np.asarray(bounds, np.int64)
        if n_blocks is None:
            n_blocks = len(bounds) - 1
        if n_work is None:
            n_work = H.lib().hdd_operator_solve_blocks_workspace(12, 0, 8)
        return H.lib().hdd_operator_solve_blocks(g(ctx), None if mesh is None else C.addressof(mesh), g(pattern), g(vals), n_comp,
                                                 None, n_blocks, None if bd is None else bd.ctypes.data, g(b), g(x), g(opt),
                                                 g(work), n_work, history, ldh, g(info), None)

    def apply(self, ctx="fake", pattern="pat", vals="vals", x="fake", y="fake", n_comp=1, bounds=(0, 6, 12), n_blocks=None):
        g = self._g
        bd = None if bounds is None else np.asarray(bounds, np.int64)
        if n_blocks is None:
            n_blocks = len(bounds) - 1
        return H.lib().hdd_operator_apply_blocks(g(ctx), None, g(pattern), g(vals), n_comp, None, n_blocks,
                                                 None if bd is None else bd.ctypes.data, g(x), g(y), None)


def _msg():
    return H.lib().hdd_last_error(None)


def test_rejects_null_arguments():
    o = _Operands()
    for k in ("ctx", "pattern", "vals", "b", "x", "opt", "work", "info"):
        assert o.solve(**{k: None}) == 1, k
        assert _msg().startswith(WHO), k
    assert o.solve(bounds=None, n_blocks=2) == 1 and _msg().startswith(WHO) and b"bounds" in _msg()
    o.vals[0] = None                      # a null value array inside d_vals
    assert o.solve() == 1 and _msg().startswith(WHO)
    assert H.lib().hdd_operator_solve_blocks(None, None, None, None, 1, None, 1, None, None, None, None, None, 0, None, 0,
                                             None, None) == 1
    o = _Operands()
    for k in ("ctx", "pattern", "vals", "x", "y"):
        assert o.apply(**{k: None}) == 1, k
        assert _msg().startswith(WHO_APPLY), k
    assert o.apply(bounds=None, n_blocks=2) == 1 and _msg().startswith(WHO_APPLY) and b"bounds" in _msg()


def test_n_blocks():
    o = _Operands()
    for n in (0, -1, H.MAX_SOLVE_BLOCKS + 1, 100000):
        assert o.solve(n_blocks=n) == 1, n
        assert _msg().startswith(WHO) and b"n_blocks" in _msg(), (n, _msg())
        assert o.apply(n_blocks=n) == 1, n
        assert _msg().startswith(WHO_APPLY) and b"n_blocks" in _msg(), (n, _msg())


def test_bounds():
    o = _Operands()
    for bd in [(0, 6, 6), (0, 9, 6, 12), (6, 0), (3, 3)]:
        assert o.solve(bounds=bd) == 1, bd
        assert _msg().startswith(WHO) and b"ascending" in _msg(), (bd, _msg())
        assert o.apply(bounds=bd) == 1 and _msg().startswith(WHO_APPLY) and b"ascending" in _msg(), bd
    for bd in [(-3, 6, 12), (0, 6, 15), (0, 13)]:
        assert o.solve(bounds=bd) == 1, bd
        assert _msg().startswith(WHO) and b"outside" in _msg(), (bd, _msg())
        assert o.apply(bounds=bd) == 1 and _msg().startswith(WHO_APPLY) and b"outside" in _msg(), bd
    # the square part of a rectangular matrix
    r = _Operands(n_rows=12, n_cols=9)
    assert r.solve(bounds=(0, 6, 12)) == 1 and b"outside" in _msg()
    r = _Operands(n_rows=9, n_cols=12)
    assert r.solve(bounds=(0, 6, 12)) == 1 and b"outside" in _msg()
    # no multiple of the block size: the first, an inner and the last bound (block_size 3, and 0 = nb of the mesh)
    for bd in [(1, 6, 12), (0, 5, 12), (0, 6, 11), (0, 3, 7, 12)]:
        assert o.solve(bounds=bd) == 1, bd
        assert _msg().startswith(WHO) and b"multiples" in _msg(), (bd, _msg())
    o.opt.block_size = 0
    assert o.solve(bounds=(0, 4, 12), mesh=o.mesh) == 1 and b"multiples" in _msg()
    o.opt.block_size = 5
    assert o.solve(bounds=(0, 6, 12)) == 1 and b"multiples" in _msg()


def test_history_leading_dimension():
    o = _Operands()                         # max_iter = 100
    for ldh in (100, 0, -5):
        assert o.solve(history=o.fake, ldh=ldh) == 1, ldh
        assert _msg().startswith(WHO) and b"ldh" in _msg(), (ldh, _msg())


def test_workspace_too_small_explicit_and_implied_block_size():
    o = _Operands()
    need = H.lib().hdd_operator_solve_blocks_workspace(12, 3, 2)
    assert o.solve(n_work=need - 1) == 1 and b"n_work" in _msg() and _msg().startswith(WHO)
    assert o.solve(n_work=0) == 1 and b"n_work" in _msg()
    # what one segment needs is not enough for two; the rows of the interval decide, not the pattern's
    assert o.solve(n_work=H.lib().hdd_operator_solve_blocks_workspace(12, 3, 1)) == 1 and b"n_work" in _msg()
    assert o.solve(bounds=(3, 6, 9), n_work=H.lib().hdd_operator_solve_blocks_workspace(6, 3, 2) - 1) == 1 and b"n_work" in _msg()
    o.opt.block_size = 0
    assert o.solve(mesh=o.mesh, n_work=need - 1) == 1 and b"n_work" in _msg()


def test_checks_shared_with_the_single_solve():
    o = _Operands()
    for n in (0, H.MAX_COMP + 1):
        assert o.solve(n_comp=n) == 1 and b"n_comp" in _msg() and _msg().startswith(WHO)
        assert o.apply(n_comp=n) == 1 and b"n_comp" in _msg() and _msg().startswith(WHO_APPLY)
    for field, bad, word in [("max_iter", -1, b"max_iter"), ("rtol", float("nan"), b"rtol"), ("atol", -1.0, b"atol"),
                             ("precond", 2, b"precond"), ("block_size", 9, b"block_size"), ("check_every", -1, b"check_every")]:
        o = _Operands()
        setattr(o.opt, field, bad)
        assert o.solve() == 1, (field, bad)
        assert word in _msg() and _msg().startswith(WHO), (field, bad, _msg())
    o = _Operands()
    o.opt.block_size = 0                         # no mesh to take nb from
    assert o.solve() == 1 and b"block_size" in _msg()
