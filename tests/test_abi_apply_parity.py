"""The operator-application entry points answer what they answered before hdd_operator_apply and
hdd_operator_apply_multi were given shared argument checks: tests/golden/apply_abi_parent.json, recorded by
tests/golden/make_apply_abi.py at the commit before that change, holds the return code and the full hdd_last_error
text of rejected calls of hdd_operator_apply, hdd_operator_apply2 and hdd_operator_apply_multi (fake operands; no
device) -- among them calls that are wrong in two ways, which pin the order of the checks.  Equality, no tolerance:
the first failing check of a call and its wording are part of the ABI's behaviour."""
import ctypes as C
import json
import os

import numpy as np

import hdd_amd as H

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "apply_abi_parent.json")
ENTRIES = ("hdd_operator_apply", "hdd_operator_apply2", "hdd_operator_apply_multi")


class _Operands:
    """valid-looking host descriptors; `fake` (16-byte aligned) stands for a context / device array.  The mesh is four
    P1 elements whose face pattern `pat` is: with it the plan takes the tile path."""

    def __init__(self):
        self.keep = np.zeros(64)
        self.fake = (self.keep.ctypes.data + 15) & ~15
        self.pat = H.CsrT(12, 12, 48, self.fake, self.fake, self.fake)
        self.vals = (C.c_void_p * H.MAX_COMP)(*([self.fake] * H.MAX_COMP))
        self.mesh = H.MeshT(H.SIMPLEX, 1, 4, 0, 4, self.fake, self.fake, self.fake, None, None)
        self.theta = np.ones((H.MAX_VEC, H.MAX_COMP))

    def call(self, entry, ctx="fake", mesh=None, pattern="pat", vals="vals", x="fake", y="fake", work="fake", out="fake",
             n_comp=1, n_vec=1, n_v=1, ldt=H.MAX_COMP, ldx=12, ldy=12, rng=None):
        g = lambda k: None if k is None else (C.addressof(getattr(self, k)) if k in ("pat", "mesh") else getattr(self, k))
        L, r = H.lib(), None if rng is None else C.addressof(rng)
        if entry == "hdd_operator_apply":
            return L.hdd_operator_apply(g(ctx), g(mesh), g(pattern), g(vals), n_comp, None, r, g(x), ldx, g(y), ldy, n_vec, None)
        if entry == "hdd_operator_apply_multi":
            return L.hdd_operator_apply_multi(g(ctx), g(mesh), g(pattern), g(vals), n_comp, self.theta.ctypes.data, ldt, r,
                                              g(x), ldx, g(y), ldy, n_vec, None)
        return L.hdd_operator_apply2(g(ctx), g(mesh), g(pattern), g(vals), n_comp, None, r, g(y), ldy, n_v, g(x), ldx, n_vec,
                                     g(work), ldy, g(out), None)


def _edited(field, value, on="pat"):
    o = _Operands()
    setattr(getattr(o, on), field, value)
    return o


def _calls(entry):
    """(label, call) of the rejected calls of one entry"""
    O = _Operands
    for k in ("ctx", "pattern", "vals", "x", "y") + (("work", "out") if entry == "hdd_operator_apply2" else ()):
        yield "null %s" % k, lambda k=k: O().call(entry, **{k: None})
    yield "null x, n_vec 0, null ctx", lambda: O().call(entry, x=None, n_vec=0, ctx=None)
    for n in (0, -1, H.MAX_VEC + 1):
        yield "n_vec %d" % n, lambda n=n: O().call(entry, n_vec=n)
        yield "n_vec %d, null ctx" % n, lambda n=n: O().call(entry, n_vec=n, ctx=None)
    if entry == "hdd_operator_apply2":
        yield "n_v 9", lambda: O().call(entry, n_v=9)
    for n in (0, H.MAX_COMP + 1):
        yield "n_comp %d" % n, lambda n=n: O().call(entry, n_comp=n)
        yield "n_comp %d, ldx 0" % n, lambda n=n: O().call(entry, n_comp=n, ldx=0)

    def null_second():
        o = O()
        o.vals[1] = None
        return o.call(entry, n_comp=2, ldt=1)
    yield "null vals[1], ldt 1", null_second
    yield "negative nnz", lambda: _edited("nnz", -1).call(entry)
    for r in [(-1, 12, 0, 12), (0, 13, 0, 12), (5, 4, 0, 12), (0, 12, 0, 13), (0, 12, 7, 6)]:
        yield "range %s, ldx 0" % (r,), lambda r=r: O().call(entry, rng=H.BlockRange(*r), ldx=0)
    yield "unknown element type", lambda: _edited("elem_type", 77, "mesh").call(entry, mesh="mesh")
    yield "own_end beyond n_local", lambda: _edited("own_end", 5, "mesh").call(entry, mesh="mesh")
    yield "mesh without neighbors", lambda: _edited("neighbors", None, "mesh").call(entry, mesh="mesh")
    yield "15 rows on four P1 elements", lambda: _edited("n_rows", 15).call(entry, mesh="mesh")
    yield "no row_ptr, no mesh", lambda: _edited("row_ptr", None).call(entry, ldx=0)
    yield "no col, range off the blocks", lambda: _edited("col", None).call(entry, mesh="mesh", rng=H.BlockRange(1, 12, 0, 12))
    yield "no row_ptr, four components on the mesh, ldt 1", lambda: _edited("row_ptr", None).call(entry, mesh="mesh", n_comp=4, ldt=1, ldx=0)
    yield "ldt 1 of two components, ldx 0", lambda: O().call(entry, n_comp=2, ldt=1, ldx=0)
    yield "ldt 0, ldy 0", lambda: O().call(entry, ldt=0, ldy=0)
    for kw in (dict(ldx=11), dict(ldy=11), dict(ldx=0), dict(ldx=8, ldy=6, rng=H.BlockRange(0, 6, 0, 9))):
        yield "ld %s" % sorted((k, v) for k, v in kw.items() if k != "rng"), lambda kw=kw: O().call(entry, **kw)


def record():
    """what the fixture holds, from the library that is loaded"""
    out = {}
    for entry in ENTRIES:
        out[entry] = {}
        for label, call in _calls(entry):
            assert label not in out[entry], label
            rc = call()
            out[entry][label] = [rc, H.lib().hdd_last_error(None).decode()]
    return out


def test_rejected_calls_answer_the_parents_messages():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = record()
    assert list(want) == list(ENTRIES)
    for entry in ENTRIES:
        assert list(got[entry]) == list(want[entry]) and len(want[entry]) >= 35
        for label, (rc, msg) in want[entry].items():
            assert rc == 1 and msg.startswith(entry + ": "), (entry, label, msg)
            assert got[entry][label] == [rc, msg], (entry, label)
