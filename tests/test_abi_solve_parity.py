"""The two solver entry points answer what they answered before their host code was merged into one driver:
tests/golden/solve_abi_parent.json, recorded by tests/golden/make_solve_abi.py at the commit before the merge, holds
the workspace sizes of both workspace functions and the full hdd_last_error text of every call that test_abi_solve.py
and test_abi_solve_batched.py make to be rejected (same fake operands; no device).  Equality, no tolerance: the first
failing check of a call and its wording are part of the ABI's behaviour."""
import json
import os

import hdd_amd as H
import test_abi_estimate as TE
import test_abi_estimate_blocks as TEB
import test_abi_solve as S1
import test_abi_solve_batched as SB
import test_abi_solve_blocks as SK
import test_abi_solve_multi as SM

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_abi_parent.json")
ROWS = (0, 24, 2400, 24000)
N_RHS = (1, 3, 4, 5, H.MAX_VEC)
N_BLOCKS = (1, 2, 17, H.MAX_SOLVE_BLOCKS)
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


# ---- the entries that came after the merge: hdd_operator_solve_multi, hdd_operator_solve_blocks and the two estimate
# calls, recorded by the same script at the commit before their host code went through one call path per layer
def _multi_calls():
    """(label, call) of every rejected hdd_operator_solve_multi call of test_abi_solve_multi.py, in its order"""
    L, O = H.lib(), SM._Operands
    for k in KEYS:
        yield "null %s" % k, lambda k=k: O().solve(**{k: None})
    yield "null vals[0]", lambda: _null_vals(SM).solve()
    yield "all null", lambda: L.hdd_operator_solve_multi(None, None, None, None, 1, None, 0, None, None, 0, None, 0, 1, None,
                                                         None, 0, None, 0, None, None)
    for n in (0, -1, H.MAX_VEC + 1, 100):
        yield "n_rhs %d" % n, lambda n=n: O().solve(n_rhs=n)
    for n_comp, ldt in [(2, 1), (2, 0), (1, 0), (2, -3)]:
        yield "n_comp %d, ldt %d" % (n_comp, ldt), lambda n=n_comp, l=ldt: O().solve(n_comp=n, ldt=l)
    yield "no theta, ldt 0, n_work 0", lambda: O().solve(n_comp=2, theta=None, ldt=0, n_work=0)
    yield "ldt 2, n_work 0", lambda: O().solve(n_comp=2, ldt=2, n_work=0)
    for kw in (dict(ldb=11), dict(ldx=11), dict(ldb=0), dict(ldx=-1)):
        yield "ld %s" % sorted(kw.items()), lambda kw=kw: O().solve(**kw)
    yield "range 3..9, ldb 5", lambda: O().solve(rng=H.BlockRange(3, 9, 3, 9), ldb=5)
    yield "n_rhs 1, ldx 11", lambda: O().solve(n_rhs=1, ldx=11)

    def history(ldh):
        o = O()
        return o.solve(history=o.fake, ldh=ldh)
    for ldh in (100, 0, -5):
        yield "ldh %d" % ldh, lambda ldh=ldh: history(ldh)
    need = L.hdd_operator_solve_multi_workspace(12, 3, 3)
    yield "n_work need - 1", lambda: O().solve(n_work=need - 1)
    yield "n_work 0", lambda: O().solve(n_work=0)
    for n in range(2, H.MAX_VEC + 1):
        yield "n_rhs %d, n_work of the batch" % n, lambda n=n: O().solve(
            n_rhs=n, n_work=L.hdd_operator_solve_batched_workspace(12, 3, n))
    yield "n_work of one column", lambda: O().solve(n_work=L.hdd_operator_solve_multi_workspace(12, 3, 1))

    def implied():
        o = _with(SM, "block_size", 0)
        return o.solve(mesh=o.mesh, n_work=need - 1)
    yield "n_work need - 1, block_size of the mesh", implied
    for n in (0, H.MAX_COMP + 1):
        yield "n_comp %d" % n, lambda n=n: O().solve(n_comp=n)
    for r in [(0, 13, 0, 13), (0, 6, 6, 12), (0, 6, 0, 12), (3, 9, 0, 6)]:
        yield "range %s" % (r,), lambda r=r: O().solve(rng=H.BlockRange(*r))
    for field, bad in OPTIONS_BATCHED:
        yield "%s %r" % (field, bad), lambda f=field, b=bad: _with(SM, f, b).solve()
    yield "block_size 0, no mesh", lambda: _with(SM, "block_size", 0).solve()
    yield "block_size 5 of 12 rows", lambda: _with(SM, "block_size", 5).solve()


def _blocks_calls():
    """the same of the hdd_operator_solve_blocks calls of test_abi_solve_blocks.py"""
    L, O = H.lib(), SK._Operands
    ws = L.hdd_operator_solve_blocks_workspace
    for k in KEYS:
        yield "null %s" % k, lambda k=k: O().solve(**{k: None})
    yield "null bounds", lambda: O().solve(bounds=None, n_blocks=2)
    yield "null vals[0]", lambda: _null_vals(SK).solve()
    yield "all null", lambda: L.hdd_operator_solve_blocks(None, None, None, None, 1, None, 1, None, None, None, None, None, 0,
                                                          None, 0, None, None)
    for n in (0, -1, H.MAX_SOLVE_BLOCKS + 1, 100000):
        yield "n_blocks %d" % n, lambda n=n: O().solve(n_blocks=n)
    for bd in [(0, 6, 6), (0, 9, 6, 12), (6, 0), (3, 3), (-3, 6, 12), (0, 6, 15), (0, 13)]:
        yield "bounds %s" % (bd,), lambda bd=bd: O().solve(bounds=bd)
    yield "12 x 9", lambda: O(n_rows=12, n_cols=9).solve(bounds=(0, 6, 12))
    yield "9 x 12", lambda: O(n_rows=9, n_cols=12).solve(bounds=(0, 6, 12))
    for bd in [(1, 6, 12), (0, 5, 12), (0, 6, 11), (0, 3, 7, 12)]:
        yield "bounds %s" % (bd,), lambda bd=bd: O().solve(bounds=bd)

    def of_the_mesh(**kw):
        o = _with(SK, "block_size", 0)
        return o.solve(mesh=o.mesh, **kw)
    yield "bounds (0, 4, 12), block_size of the mesh", lambda: of_the_mesh(bounds=(0, 4, 12))
    yield "block_size 5 of 12 rows", lambda: _with(SK, "block_size", 5).solve(bounds=(0, 6, 12))

    def history(ldh):
        o = O()
        return o.solve(history=o.fake, ldh=ldh)
    for ldh in (100, 0, -5):
        yield "ldh %d" % ldh, lambda ldh=ldh: history(ldh)
    need = ws(12, 3, 2)
    yield "n_work need - 1", lambda: O().solve(n_work=need - 1)
    yield "n_work 0", lambda: O().solve(n_work=0)
    yield "n_work of one segment", lambda: O().solve(n_work=ws(12, 3, 1))
    yield "bounds (3, 6, 9), n_work need - 1", lambda: O().solve(bounds=(3, 6, 9), n_work=ws(6, 3, 2) - 1)
    yield "n_work need - 1, block_size of the mesh", lambda: of_the_mesh(n_work=need - 1)
    for n in (0, H.MAX_COMP + 1):
        yield "n_comp %d" % n, lambda n=n: O().solve(n_comp=n)
    for field, bad in OPTIONS_BATCHED:
        yield "%s %r" % (field, bad), lambda f=field, b=bad: _with(SK, f, b).solve()
    yield "block_size 0, no mesh", lambda: _with(SK, "block_size", 0).solve()


def _changed(make, change):
    o = make()
    change(o)
    return o.call()


def _estimate_calls():
    """the same of the hdd_swipdg_estimate calls of test_abi_estimate.py"""
    O = TE._Operands
    for k in ("ctx", "est", "mesh", "kappa", "tensor", "prm", "u", "work", "sums"):
        yield "null %s" % k, lambda k=k: O().call(**{k: None})
    for n in (0, -1, H.MAX_COMP + 1):
        yield "n_comp %d" % n, lambda n=n: O().call(n_comp=n)
    for d in (-1, None, "-1"):
        label = "n_work %s" % ("need - 1" if d == -1 else "0" if d is None else "-1")

        def small(d=d):
            o = O()
            return o.call(n_work=o.est.n_work - 1 if d == -1 else 0 if d is None else -1)
        yield label, small
    yield "host-only", lambda: O().call()

    def no_vertices(o):
        o.mesh.elem_vertices = None
        o.mesh.vertex_coords = None

    def two_more(o):
        o.mesh.n_local += 2
        o.mesh.own_end += 2

    def no_faces(o):
        o.mesh.face_info = None

    def no_per_elem(o):
        o.kappa[1].per_elem = None
    for label, change in (("no elem_vertices", no_vertices), ("n_local + 2", two_more), ("no face_info", no_faces),
                          ("kappa without per_elem", no_per_elem)):
        yield label, lambda c=change: _changed(O, c)
    for field, bad in [("elem_type", H.CUBE), ("elem_type", H.HEX), ("degree", 2), ("own_begin", 1), ("own_end", 3)]:
        yield "mesh %s %d" % (field, bad), lambda f=field, b=bad: _changed(O, lambda o: setattr(o.mesh, f, b))
    yield "kappa sinusoid", lambda: _changed(O, lambda o: setattr(o.kappa[0], "kind", H.FN_SINUSOID))
    yield "tensor kind 7", lambda: _changed(O, lambda o: setattr(o.tensor, "kind", 7))
    yield "force order 7", lambda: _changed(O, lambda o: setattr(o.force, "order", 7))


def _estimate_blocks_calls():
    """the same of the hdd_block_swipdg_estimate calls of test_abi_estimate_blocks.py"""
    O = TEB._BlockOperands
    yield "no segments", lambda: O(segments=False).call()
    for k in ("ctx", "est", "sums"):
        yield "null %s" % k, lambda k=k: O().call(**{k: None})
    for role in ("mu", "bar", "hat", "min", "max"):
        for bad in ((1.0, 0.0), (-1.0, 1.0), (1.0, float("nan"))):
            yield "theta %s %r" % (role, bad), lambda r=role, b=bad: _changed(O, lambda o: o.theta.update({r: b}))
    for label, n_work in (("need - 1", lambda e: e.n_work_blocks - 1), ("of the ESV2007 call", lambda e: e.n_work),
                          ("0", lambda e: 0), ("-1", lambda e: -1)):
        def small(n_work=n_work):
            o = O()
            return o.call(n_work=n_work(o.est))
        yield "n_work %s" % label, small
    yield "mesh degree 2", lambda: _changed(O, lambda o: setattr(o.mesh, "degree", 2))
    yield "host-only", lambda: _changed(O, lambda o: o.theta.update(mu=(1.0, 0.5), bar=(0.7, 1.3), hat=(1.2, 0.4),
                                                                    min=(0.1, 0.2), max=(3.0, 4.0)))


def _estimator_workspaces():
    """hdd_estimator_blocks_workspace (and hdd_estimator_workspace beside it) for the segment layouts of
    test_abi_estimate_blocks.py::test_workspaces, without segments and without an estimator"""
    L = H.lib()
    est = H.Estimator(None, H.Grid.structured(H.SIMPLEX, 16, 17).local())
    n = 544
    out = {"null": [L.hdd_estimator_workspace(None), L.hdd_estimator_blocks_workspace(None)],
           "no segments": [L.hdd_estimator_workspace(est.h), L.hdd_estimator_blocks_workspace(est.h)]}
    for bounds in ([0, n], [0, 1, 3, 258, 514, n], [0, 257, n]):
        est.set_segments(bounds)
        out["%s" % (bounds,)] = [L.hdd_estimator_workspace(est.h), L.hdd_estimator_blocks_workspace(est.h)]
    est.set_segments()
    out["segments cleared"] = [L.hdd_estimator_workspace(est.h), L.hdd_estimator_blocks_workspace(est.h)]
    return out


LATER = (("rejected_multi", "hdd_operator_solve_multi: ", 54), ("rejected_blocks", "hdd_operator_solve_blocks: ", 47),
         ("rejected_estimate", "hdd_swipdg_estimate: ", 28), ("rejected_estimate_blocks", "hdd_block_swipdg_estimate: ", 25))


def record_later():
    """the sections of the fixture for the later entries, from the library that is loaded"""
    L = H.lib()
    return {
        "workspace_multi": {"%d,%d,%d" % (r, bs, n): L.hdd_operator_solve_multi_workspace(r, bs, n)
                            for r in ROWS for bs in range(9) for n in N_RHS},
        "workspace_blocks": {"%d,%d,%d" % (r, bs, n): L.hdd_operator_solve_blocks_workspace(r, bs, n)
                             for r in ROWS for bs in range(9) for n in N_BLOCKS},
        "workspace_estimator": _estimator_workspaces(),
        "rejected_multi": _rejected(_multi_calls()),
        "rejected_blocks": _rejected(_blocks_calls()),
        "rejected_estimate": _rejected(_estimate_calls()),
        "rejected_estimate_blocks": _rejected(_estimate_blocks_calls()),
    }


def test_workspace_sizes_of_the_later_entries_are_the_parents():
    want, got = _fixture(), record_later()
    assert len(want["workspace_multi"]) == 4 * 9 * 5 and len(want["workspace_blocks"]) == 4 * 9 * 4
    assert len(want["workspace_estimator"]) == 6
    for part in ("workspace_multi", "workspace_blocks", "workspace_estimator"):
        assert got[part] == want[part], part


def test_rejected_calls_of_the_later_entries_answer_the_parents_messages():
    want, got = _fixture(), record_later()
    for part, who, calls in LATER:
        assert list(got[part]) == list(want[part]), part
        assert len(want[part]) == calls, part
        for label, (rc, msg) in want[part].items():
            assert rc in (1, 3) and msg.startswith(who), (part, label, msg)
            assert got[part][label] == [rc, msg], (part, label)
