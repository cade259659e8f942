"""The per-column-theta entry points of the C ABI (hdd_operator_apply_multi, hdd_operator_solve_multi,
hdd_operator_solve_multi_workspace): declared, exported, bound by the Python front-end, additive to ABI 8, and every
argument check comes before the first device call -- so they answer HDD_ERR_INVALID (1) here, without a GPU, with
the entry's own name in front of the message.  The pointers that stand for the context and the device arrays are
never dereferenced by a rejected call."""
import ctypes as C

import numpy as np

import hdd_amd as H

NAMES = ("hdd_operator_apply_multi", "hdd_operator_solve_multi", "hdd_operator_solve_multi_workspace")
SOLVE = b"hdd_operator_solve_multi:"
APPLY = b"hdd_operator_apply_multi:"


def test_symbols_exported_and_bound():
    L = H.lib()
    declared = H.declared_symbols()
    for n in NAMES:
        assert n in declared, n
        assert getattr(L, n).argtypes is not None, n
    assert L.hdd_operator_solve_multi_workspace.restype is C.c_int64
    assert len(L.hdd_operator_apply_multi.argtypes) == 14
    assert len(L.hdd_operator_solve_multi.argtypes) == 20
    assert callable(H.apply_multi) and callable(H.solve_multi)
    assert L.hdd_abi_version() == 8        # additive: the ABI version stays


def packed_blocks(rows, bs):
    """doubles of one set of packed inverse blocks, every set starting 16-byte aligned"""
    n = rows // bs * (bs * (bs + 1) // 2)
    return n + (n & 1)


def test_workspace_size():
    ws = H.lib().hdd_operator_solve_multi_workspace
    wb = H.lib().hdd_operator_solve_batched_workspace
    for bs in range(0, 9):
        for n_rhs in (1, 4, 8):
            sizes = [ws(24 * k, bs, n_rhs) for k in (0, 1, 2, 10, 1000)]
            assert all(s > 0 for s in sizes), (bs, n_rhs)
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[-1], (bs, n_rhs)
        by_rhs = [ws(2400, bs, n) for n in range(1, H.MAX_VEC + 1)]
        assert all(a < b for a, b in zip(by_rhs, by_rhs[1:])), bs
        for n_rhs in range(1, H.MAX_VEC + 1):
            assert ws(2400, bs, n_rhs) >= wb(2400, bs, n_rhs), (bs, n_rhs)
    for rows in (2400, 840):
        for bs in range(1, 9):
            if rows % bs:
                continue
            assert ws(rows, bs, 1) == wb(rows, bs, 1)                 # one column: one set of blocks
            for n_rhs in range(2, H.MAX_VEC + 1):
                # a further column costs what it costs the batch, and one more set of packed blocks
                assert ws(rows, bs, n_rhs) - ws(rows, bs, n_rhs - 1) == \
                    wb(rows, bs, n_rhs) - wb(rows, bs, n_rhs - 1) + packed_blocks(rows, bs), (rows, bs, n_rhs)
                assert ws(rows, bs, n_rhs) == wb(rows, bs, n_rhs) + (n_rhs - 1) * packed_blocks(rows, bs)
    for n_rhs in range(1, H.MAX_VEC + 1):
        assert ws(2400, 0, n_rhs) >= max(ws(2400, bs, n_rhs) for bs in range(1, 9))   # covers every block size
    for n_rhs in (0, -1, H.MAX_VEC + 1):
        assert ws(24, 3, n_rhs) == 0, n_rhs
    assert ws(-1, 3, 2) == 0 and ws(24, 9, 2) == 0 and ws(24, -1, 2) == 0


def test_batched_workspace_is_what_it_was():
    """the batched function's values (head of 72 doubles: eight 64-byte states and 64 bytes of group words; per column
    four kinds of 4096 partial sums and p, q, r, z; one set of packed blocks), as before this entry existed"""
    wb = H.lib().hdd_operator_solve_batched_workspace
    for rows, bs, n_rhs in [(2400, 3, 1), (2400, 3, 4), (2400, 8, 8), (12, 3, 3), (13 * 4, 4, 5), (0, 3, 2), (7, 1, 2)]:
        even = rows + (rows & 1)
        assert wb(rows, bs, n_rhs) == 72 + n_rhs * (4 * 4096 + 4 * even) + packed_blocks(rows, bs), (rows, bs, n_rhs)
    assert wb(2400, 0, 3) == max(wb(2400, bs, 3) for bs in range(1, 9))


class _Operands:
    """valid-looking host descriptors; `fake` stands for a context / device array"""

    def __init__(self, n_rows=12, n_cols=12, n_rhs=3):
        self.keep = np.zeros(64)
        self.fake = self.keep.ctypes.data
        self.pat = H.CsrT(n_rows, n_cols, 48, self.fake, self.fake, self.fake)
        self.vals = (C.c_void_p * 2)(self.fake, self.fake)
        self.opt = H.SolveOptions(1e-8, 0.0, 100, 0, H.PRECOND_BLOCK_JACOBI, 3, 0, 0)
        self.info = (H.SolveInfo * H.MAX_VEC)()
        self.n_rhs = n_rhs
        self.mesh = H.MeshT(H.SIMPLEX, 1, 4, 0, 4, self.fake, self.fake, self.fake, None, None)
        self.theta = np.ones((H.MAX_VEC, H.MAX_COMP))

    def _g(self, k):
        if k is None:
            return None
        if k in ("pat", "opt", "info"):
            return C.addressof(getattr(self, k))
        if k == "theta":
            return self.theta.ctypes.data
        return getattr(self, k)

    def solve(self, ctx="fake", pattern="pat", vals="vals", b="fake", x="fake", opt="opt", work="fake", info="info",
              n_comp=1, theta="theta", ldt=H.MAX_COMP, n_work=None, rng=None, mesh=None, history=None, ldb=12, ldx=12,
              ldh=101, n_rhs=None):
        g = self._g
        n_rhs = self.n_rhs if n_rhs is None else n_rhs
        if n_work is None:
            n_work = H.lib().hdd_operator_solve_multi_workspace(12, 8, H.MAX_VEC)
        return H.lib().hdd_operator_solve_multi(g(ctx), None if mesh is None else C.addressof(mesh), g(pattern), g(vals),
                                                n_comp, g(theta), ldt, None if rng is None else C.addressof(rng), g(b), ldb,
                                                g(x), ldx, n_rhs, g(opt), g(work), n_work, history, ldh, g(info), None)

    def apply(self, ctx="fake", pattern="pat", vals="vals", x="fake", y="fake", n_comp=1, theta="theta", ldt=H.MAX_COMP,
              rng=None, ldx=12, ldy=12, n_vec=3):
        g = self._g
        return H.lib().hdd_operator_apply_multi(g(ctx), None, g(pattern), g(vals), n_comp, g(theta), ldt,
                                                None if rng is None else C.addressof(rng), g(x), ldx, g(y), ldy, n_vec, None)


def _msg():
    return H.lib().hdd_last_error(None)


def test_solve_rejects_null_arguments():
    o = _Operands()
    for k in ("ctx", "pattern", "vals", "b", "x", "opt", "work", "info"):
        assert o.solve(**{k: None}) == 1, k
        assert _msg().startswith(SOLVE), k
    o.vals[0] = None                      # a null value array inside d_vals
    assert o.solve() == 1 and _msg().startswith(SOLVE)
    assert H.lib().hdd_operator_solve_multi(None, None, None, None, 1, None, 0, None, None, 0, None, 0, 1, None, None, 0,
                                            None, 0, None, None) == 1


def test_apply_rejections():
    o = _Operands()
    for k in ("ctx", "pattern", "vals", "x", "y"):
        assert o.apply(**{k: None}) == 1, k
        assert _msg().startswith(APPLY), k
    for n in (0, -1, H.MAX_VEC + 1):
        assert o.apply(n_vec=n) == 1 and _msg().startswith(APPLY) and b"n_vec" in _msg(), n
    for n in (0, H.MAX_COMP + 1):
        assert o.apply(n_comp=n) == 1 and _msg().startswith(APPLY) and b"n_comp" in _msg(), n
    assert o.apply(n_comp=2, ldt=1) == 1 and _msg().startswith(APPLY) and b"ldt" in _msg()
    assert o.apply(n_comp=1, ldt=0) == 1 and b"ldt" in _msg()
    for kw in (dict(ldx=11), dict(ldy=11), dict(ldx=0)):
        assert o.apply(**kw) == 1 and _msg().startswith(APPLY) and b"ldx / ldy" in _msg(), kw
    assert o.apply(rng=H.BlockRange(0, 13, 0, 12)) == 1 and b"range" in _msg()
    o.vals[1] = None
    assert o.apply(n_comp=2) == 1 and _msg().startswith(APPLY)


def test_n_rhs():
    o = _Operands()
    for n in (0, -1, H.MAX_VEC + 1, 100):
        assert o.solve(n_rhs=n) == 1, n
        assert _msg().startswith(SOLVE) and b"n_rhs" in _msg(), (n, _msg())


def test_theta_leading_dimension():
    o = _Operands()
    for n_comp, ldt in [(2, 1), (2, 0), (1, 0), (2, -3)]:
        assert o.solve(n_comp=n_comp, ldt=ldt) == 1, (n_comp, ldt)
        assert _msg().startswith(SOLVE) and b"ldt" in _msg(), (n_comp, ldt, _msg())
    # without thetas ldt means nothing: the call goes on to the next check (a workspace of nothing)
    assert o.solve(n_comp=2, theta=None, ldt=0, n_work=0) == 1 and b"n_work" in _msg()
    assert o.solve(n_comp=2, ldt=2, n_work=0) == 1 and b"n_work" in _msg()


def test_leading_dimensions():
    o = _Operands()
    for kw in (dict(ldb=11), dict(ldx=11), dict(ldb=0), dict(ldx=-1)):
        assert o.solve(**kw) == 1, kw
        assert _msg().startswith(SOLVE) and b"ldb / ldx" in _msg(), (kw, _msg())
    assert o.solve(rng=H.BlockRange(3, 9, 3, 9), ldb=5) == 1 and b"ldb / ldx" in _msg()
    assert o.solve(n_rhs=1, ldx=11) == 1 and b"ldb / ldx" in _msg()


def test_history_leading_dimension():
    o = _Operands()                         # max_iter = 100
    for ldh in (100, 0, -5):
        assert o.solve(history=o.fake, ldh=ldh) == 1, ldh
        assert _msg().startswith(SOLVE) and b"ldh" in _msg(), (ldh, _msg())


def test_workspace_too_small():
    o = _Operands()
    need = H.lib().hdd_operator_solve_multi_workspace(12, 3, o.n_rhs)
    assert o.solve(n_work=need - 1) == 1 and b"n_work" in _msg() and _msg().startswith(SOLVE)
    assert b"hdd_operator_solve_multi_workspace" in _msg()
    assert o.solve(n_work=0) == 1 and b"n_work" in _msg()
    # what the same-theta batch needs holds one set of inverse blocks: not enough for two or more columns
    for n_rhs in range(2, H.MAX_VEC + 1):
        batched = H.lib().hdd_operator_solve_batched_workspace(12, 3, n_rhs)
        assert batched < H.lib().hdd_operator_solve_multi_workspace(12, 3, n_rhs)
        assert o.solve(n_rhs=n_rhs, n_work=batched) == 1 and b"n_work" in _msg() and _msg().startswith(SOLVE), n_rhs
    assert o.solve(n_work=H.lib().hdd_operator_solve_multi_workspace(12, 3, 1)) == 1 and b"n_work" in _msg()
    o.opt.block_size = 0
    assert o.solve(mesh=o.mesh, n_work=need - 1) == 1 and b"n_work" in _msg()


def test_checks_shared_with_the_single_solve():
    o = _Operands()
    for n in (0, H.MAX_COMP + 1):
        assert o.solve(n_comp=n) == 1 and b"n_comp" in _msg() and _msg().startswith(SOLVE)
    assert o.solve(rng=H.BlockRange(0, 13, 0, 13)) == 1 and b"range" in _msg()
    for r in [(0, 6, 6, 12), (0, 6, 0, 12), (3, 9, 0, 6)]:
        assert o.solve(rng=H.BlockRange(*r)) == 1 and b"square" in _msg(), r
    for field, bad, word in [("max_iter", -1, b"max_iter"), ("rtol", float("nan"), b"rtol"), ("atol", -1.0, b"atol"),
                             ("precond", 2, b"precond"), ("block_size", 9, b"block_size"), ("check_every", -1, b"check_every")]:
        o = _Operands()
        setattr(o.opt, field, bad)
        assert o.solve() == 1, (field, bad)
        assert word in _msg() and _msg().startswith(SOLVE), (field, bad, _msg())
    o = _Operands()
    o.opt.block_size = 0                         # no mesh to take nb from
    assert o.solve() == 1 and b"block_size" in _msg()
    o.opt.block_size = 5                         # 12 rows are no multiple
    assert o.solve() == 1 and b"multiples" in _msg()
