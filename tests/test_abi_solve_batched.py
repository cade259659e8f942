"""The batched solver entry points of the C ABI (hdd_operator_solve_batched, hdd_operator_solve_batched_workspace):
declared, exported, bound by the Python front-end, additive to ABI 8, and every argument check comes before the first
device call -- so they answer HDD_ERR_INVALID (1) here, without a GPU.  The pointers that stand for the context and
the device arrays are never dereferenced by a rejected call."""
import ctypes as C

import numpy as np

import hdd_amd as H

NAMES = ("hdd_operator_solve_batched", "hdd_operator_solve_batched_workspace")
WHO = b"hdd_operator_solve_batched:"


def test_symbols_exported_and_bound():
    L = H.lib()
    declared = H.declared_symbols()
    for n in NAMES:
        assert n in declared, n
        assert getattr(L, n).argtypes is not None, n
    assert L.hdd_operator_solve_batched_workspace.restype is C.c_int64
    assert len(L.hdd_operator_solve_batched.argtypes) == 19
    assert callable(H.solve_batched)
    assert L.hdd_abi_version() == 8        # additive: the ABI version stays


def test_workspace_size():
    ws = H.lib().hdd_operator_solve_batched_workspace
    for bs in range(0, 9):
        for n_rhs in (1, 4, 8):
            sizes = [ws(24 * k, bs, n_rhs) for k in (0, 1, 2, 10, 1000)]
            assert all(s > 0 for s in sizes), (bs, n_rhs)
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[-1], (bs, n_rhs)
        by_rhs = [ws(2400, bs, n) for n in range(1, H.MAX_VEC + 1)]
        assert all(a < b for a, b in zip(by_rhs, by_rhs[1:])), bs
    for n_rhs in range(1, H.MAX_VEC + 1):
        # p, q, r, z per right-hand side, the packed inverse blocks once
        assert ws(2400, 3, n_rhs) >= n_rhs * 4 * 2400 + 2400 // 3 * 6
        assert ws(2400, 8, n_rhs) >= n_rhs * 4 * 2400 + 2400 // 8 * 36
        # ... once: a further right-hand side costs its vectors and partial sums, not another set of blocks
        if n_rhs > 1:
            assert ws(2400, 8, n_rhs) - ws(2400, 8, n_rhs - 1) == ws(2400, 1, n_rhs) - ws(2400, 1, n_rhs - 1)
        assert ws(2400, 0, n_rhs) >= max(ws(2400, bs, n_rhs) for bs in range(1, 9))   # covers every block size
        # a single solve's workspace is never more than the batch's of one column
        assert ws(2400, 3, n_rhs) >= H.lib().hdd_operator_solve_workspace(2400, 3)
    for n_rhs in (0, -1, H.MAX_VEC + 1):
        assert ws(24, 3, n_rhs) == 0, n_rhs
    assert ws(-1, 3, 2) == 0 and ws(24, 9, 2) == 0 and ws(24, -1, 2) == 0


class _Operands:
    """valid-looking host descriptors; `fake` stands for a context / device array"""

    def __init__(self, n_rows=12, n_cols=12, n_rhs=3):
        self.keep = np.zeros(64)
        self.fake = self.keep.ctypes.data
        self.pat = H.CsrT(n_rows, n_cols, 48, self.fake, self.fake, self.fake)
        self.vals = (C.c_void_p * 1)(self.fake)
        self.opt = H.SolveOptions(1e-8, 0.0, 100, 0, H.PRECOND_BLOCK_JACOBI, 3, 0, 0)
        self.info = (H.SolveInfo * H.MAX_VEC)()
        self.n_rhs = n_rhs
        self.mesh = H.MeshT(H.SIMPLEX, 1, 4, 0, 4, self.fake, self.fake, self.fake, None, None)

    def solve(self, ctx="fake", pattern="pat", vals="vals", b="fake", x="fake", opt="opt", work="fake", info="info",
              n_comp=1, n_work=None, rng=None, mesh=None, history=None, ldb=12, ldx=12, ldh=101, n_rhs=None):
        def g(k):
            if k is None:
                return None
            if k in ("pat", "opt", "info"):
                return C.addressof(getattr(self, k))
            return getattr(self, k)
        n_rhs = self.n_rhs if n_rhs is None else n_rhs
        if n_work is None:
            n_work = H.lib().hdd_operator_solve_batched_workspace(12, 8, H.MAX_VEC)
        return H.lib().hdd_operator_solve_batched(g(ctx), None if mesh is None else C.addressof(mesh), g(pattern), g(vals),
                                                  n_comp, None, None if rng is None else C.addressof(rng), g(b), ldb, g(x),
                                                  ldx, n_rhs, g(opt), g(work), n_work, history, ldh, g(info), None)


def _msg():
    return H.lib().hdd_last_error(None)


def test_rejects_null_arguments():
    o = _Operands()
    for k in ("ctx", "pattern", "vals", "b", "x", "opt", "work", "info"):
        assert o.solve(**{k: None}) == 1, k
        assert _msg().startswith(WHO), k
    o.vals[0] = None                      # a null value array inside d_vals
    assert o.solve() == 1 and _msg().startswith(WHO)
    assert H.lib().hdd_operator_solve_batched(None, None, None, None, 1, None, None, None, 0, None, 0, 1, None, None, 0,
                                              None, 0, None, None) == 1


def test_n_rhs():
    o = _Operands()
    for n in (0, -1, H.MAX_VEC + 1, 100):
        assert o.solve(n_rhs=n) == 1, n
        assert _msg().startswith(WHO) and b"n_rhs" in _msg(), (n, _msg())


def test_leading_dimensions():
    o = _Operands()
    for kw in (dict(ldb=11), dict(ldx=11), dict(ldb=0), dict(ldx=-1)):
        assert o.solve(**kw) == 1, kw
        assert _msg().startswith(WHO) and b"ldb / ldx" in _msg(), (kw, _msg())
    # the range's rows decide, not the pattern's
    assert o.solve(rng=H.BlockRange(3, 9, 3, 9), ldb=5) == 1 and b"ldb / ldx" in _msg()
    # also with a single right-hand side
    assert o.solve(n_rhs=1, ldx=11) == 1 and b"ldb / ldx" in _msg()


def test_history_leading_dimension():
    o = _Operands()                         # max_iter = 100
    for ldh in (100, 0, -5):
        assert o.solve(history=o.fake, ldh=ldh) == 1, ldh
        assert _msg().startswith(WHO) and b"ldh" in _msg(), (ldh, _msg())


def test_workspace_too_small_explicit_and_implied_block_size():
    o = _Operands()
    need = H.lib().hdd_operator_solve_batched_workspace(12, 3, o.n_rhs)
    assert o.solve(n_work=need - 1) == 1 and b"n_work" in _msg() and _msg().startswith(WHO)
    assert o.solve(n_work=0) == 1 and b"n_work" in _msg()
    # what one right-hand side needs is not enough for three
    assert o.solve(n_work=H.lib().hdd_operator_solve_batched_workspace(12, 3, 1)) == 1 and b"n_work" in _msg()
    assert o.solve(n_work=H.lib().hdd_operator_solve_workspace(12, 3)) == 1 and b"n_work" in _msg()
    o.opt.block_size = 0
    assert o.solve(mesh=o.mesh, n_work=need - 1) == 1 and b"n_work" in _msg()


def test_checks_shared_with_the_single_solve():
    o = _Operands()
    for n in (0, H.MAX_COMP + 1):
        assert o.solve(n_comp=n) == 1 and b"n_comp" in _msg() and _msg().startswith(WHO)
    assert o.solve(rng=H.BlockRange(0, 13, 0, 13)) == 1 and b"range" in _msg()
    for r in [(0, 6, 6, 12), (0, 6, 0, 12), (3, 9, 0, 6)]:
        assert o.solve(rng=H.BlockRange(*r)) == 1 and b"square" in _msg(), r
    for field, bad, word in [("max_iter", -1, b"max_iter"), ("rtol", float("nan"), b"rtol"), ("atol", -1.0, b"atol"),
                             ("precond", 2, b"precond"), ("block_size", 9, b"block_size"), ("check_every", -1, b"check_every")]:
        o = _Operands()
        setattr(o.opt, field, bad)
        assert o.solve() == 1, (field, bad)
        assert word in _msg() and _msg().startswith(WHO), (field, bad, _msg())
    o = _Operands()
    o.opt.block_size = 0                         # no mesh to take nb from
    assert o.solve() == 1 and b"block_size" in _msg()
    o.opt.block_size = 5                         # 12 rows are no multiple
    assert o.solve() == 1 and b"multiples" in _msg()
