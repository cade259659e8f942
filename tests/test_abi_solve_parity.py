"""The two solver entry points answer what they answered before their host code was merged into one driver:
tests/golden/solve_abi_parent.json, recorded by tests/golden/make_solve_abi.py at the commit before the merge, holds
the workspace sizes of both workspace functions and the full hdd_last_error text of every call that test_abi_solve.py
and test_abi_solve_batched.py make to be rejected (same fake operands; no device).  Equality, no tolerance: the first
failing check of a call and its wording are part of the ABI's behaviour."""
import json
import os

import hdd_amd as H
import test_abi_solve as S1
import test_abi_solve_batched as SB

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_abi_parent.json")
ROWS = (0, 24, 2400, 24000)
N_RHS = (1, 3, 4, 5, H.MAX_VEC)
KEYS = ("ctx", "pattern", "vals", "b", "x", "opt", "work", "info")
OPTIONS = [("max_iter", -1), ("rtol", -1e-3), ("rtol", float("nan")), ("atol", -1.0), ("atol", float("nan")),
           ("precond", 2), ("precond", -1), ("block_size", 9), ("block_size", -1), ("check_every", -1)]
OPTIONS_BATCHED = [("max_iter", -1), ("rtol", float("nan")), ("atol", -1.0), ("precond", 2), ("block_size", 9),
                   ("check_every", -1)]


def _with(M, field, value, **kw):
    o = M._Operands(**kw)
    setattr(o.opt, field, value)
    return o


def _null_vals(M):
    o = M._Operands()
    o.vals[0] = None
    return o


def _single_calls():
    """(label, call) of every rejected call of test_abi_solve.py, in its order"""
    L, O = H.lib(), S1._Operands
    for k in KEYS:
        yield "null %s" % k, lambda k=k: O().solve(**{k: None})
    yield "null vals[0]", lambda: _null_vals(S1).solve()
    yield "all null", lambda: L.hdd_operator_solve(None, None, None, None, 1, None, None, None, None, None, None, 0, None,
                                                   None, None)
    for n in (0, H.MAX_COMP + 1):
        yield "n_comp %d" % n, lambda n=n: O().solve(n_comp=n)
    for r in [(0, 13, 0, 13), (0, 6, 6, 12), (0, 6, 0, 12), (0, 12, 0, 6), (3, 9, 0, 6)]:
        yield "range %s" % (r,), lambda r=r: O().solve(rng=H.BlockRange(*r))
    yield "12 x 15", lambda: O(n_rows=12, n_cols=15).solve()
    for field, bad in OPTIONS:
        yield "%s %r" % (field, bad), lambda f=field, b=bad: _with(S1, f, b).solve()
    yield "block_size 0, no mesh", lambda: _with(S1, "block_size", 0).solve()

    def hexq2():
        o = _with(S1, "block_size", 0)
        return o.solve(mesh=H.MeshT(H.HEX, 2, 4, 0, 4, o.fake, o.fake, o.fake, None, None))
    yield "block_size 0, hex Q2", hexq2
    for bs in (5, 7, 8):
        yield "block_size %d of 12 rows" % bs, lambda bs=bs: _with(S1, "block_size", bs).solve()
    yield "block_size 4, range 2..10", lambda: _with(S1, "block_size", 4).solve(rng=H.BlockRange(2, 10, 2, 10))
    need = L.hdd_operator_solve_workspace(12, 3)
    yield "n_work need - 1", lambda: O().solve(n_work=need - 1)
    yield "n_work 0", lambda: O().solve(n_work=0)

    def implied():
        o = _with(S1, "block_size", 0)
        return o.solve(mesh=o.mesh, n_work=need - 1)
    yield "n_work need - 1, block_size of the mesh", implied


def _batched_calls():
    """the same of test_abi_solve_batched.py"""
    L, O = H.lib(), SB._Operands
    for k in KEYS:
        yield "null %s" % k, lambda k=k: O().solve(**{k: None})
    yield "null vals[0]", lambda: _null_vals(SB).solve()
    yield "all null", lambda: L.hdd_operator_solve_batched(None, None, None, None, 1, None, None, None, 0, None, 0, 1, None,
                                                           None, 0, None, 0, None, None)
    for n in (0, -1, H.MAX_VEC + 1, 100):
        yield "n_rhs %d" % n, lambda n=n: O().solve(n_rhs=n)
    for kw in (dict(ldb=11), dict(ldx=11), dict(ldb=0), dict(ldx=-1)):
        yield "ld %s" % sorted(kw.items()), lambda kw=kw: O().solve(**kw)
    yield "range 3..9, ldb 5", lambda: O().solve(rng=H.BlockRange(3, 9, 3, 9), ldb=5)
    yield "n_rhs 1, ldx 11", lambda: O().solve(n_rhs=1, ldx=11)

    def history(ldh):
        o = O()
        return o.solve(history=o.fake, ldh=ldh)
    for ldh in (100, 0, -5):
        yield "ldh %d" % ldh, lambda ldh=ldh: history(ldh)
    need = L.hdd_operator_solve_batched_workspace(12, 3, 3)
    yield "n_work need - 1", lambda: O().solve(n_work=need - 1)
    yield "n_work 0", lambda: O().solve(n_work=0)
    yield "n_work of one column", lambda: O().solve(n_work=L.hdd_operator_solve_batched_workspace(12, 3, 1))
    yield "n_work of the single solve", lambda: O().solve(n_work=L.hdd_operator_solve_workspace(12, 3))

    def implied():
        o = _with(SB, "block_size", 0)
        return o.solve(mesh=o.mesh, n_work=need - 1)
    yield "n_work need - 1, block_size of the mesh", implied
    for n in (0, H.MAX_COMP + 1):
        yield "n_comp %d" % n, lambda n=n: O().solve(n_comp=n)
    for r in [(0, 13, 0, 13), (0, 6, 6, 12), (0, 6, 0, 12), (3, 9, 0, 6)]:
        yield "range %s" % (r,), lambda r=r: O().solve(rng=H.BlockRange(*r))
    for field, bad in OPTIONS_BATCHED:
        yield "%s %r" % (field, bad), lambda f=field, b=bad: _with(SB, f, b).solve()
    yield "block_size 0, no mesh", lambda: _with(SB, "block_size", 0).solve()
    yield "block_size 5 of 12 rows", lambda: _with(SB, "block_size", 5).solve()


def _rejected(calls):
    out = {}
    for label, call in calls:
        rc = call()
        assert label not in out, label
        out[label] = [rc, H.lib().hdd_last_error(None).decode()]
    return out


def record():
    """what the fixture holds, from the library that is loaded"""
    L = H.lib()
    return {
        "workspace": {"%d,%d" % (r, bs): L.hdd_operator_solve_workspace(r, bs) for r in ROWS for bs in range(9)},
        "workspace_batched": {"%d,%d,%d" % (r, bs, n): L.hdd_operator_solve_batched_workspace(r, bs, n)
                              for r in ROWS for bs in range(9) for n in N_RHS},
        "rejected": _rejected(_single_calls()),
        "rejected_batched": _rejected(_batched_calls()),
    }


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_workspace_sizes_are_the_parents():
    want, got = _fixture(), record()
    assert len(want["workspace"]) == 4 * 9 and len(want["workspace_batched"]) == 4 * 9 * 5
    assert got["workspace"] == want["workspace"]
    assert got["workspace_batched"] == want["workspace_batched"]


def test_rejected_calls_answer_the_parents_messages():
    want, got = _fixture(), record()
    for part, who in (("rejected", "hdd_operator_solve: "), ("rejected_batched", "hdd_operator_solve_batched: ")):
        assert list(got[part]) == list(want[part])
        for label, (rc, msg) in want[part].items():
            assert rc == 1 and msg.startswith(who), (part, label, msg)
            assert got[part][label] == [rc, msg], (part, label)
