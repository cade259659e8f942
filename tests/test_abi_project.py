"""The reduced-basis projection entry points (hdd_operator_project, its workspace function, hdd_vectors_inner):
declared, exported, bound by the Python front-end, additive to ABI 8, and every argument check comes before the first
device call -- so they answer HDD_ERR_INVALID (1) here, without a GPU.  The pointers that stand for the context and
the device arrays are never dereferenced by a rejected call."""
import ctypes as C

import numpy as np

import hdd_amd as H

NAMES = ("hdd_operator_project", "hdd_operator_project_workspace", "hdd_vectors_inner")
WHO = b"hdd_operator_project:"
WHO_INNER = b"hdd_vectors_inner:"


def test_symbols_exported_and_bound():
    L = H.lib()
    declared = H.declared_symbols()
    for n in NAMES:
        assert n in declared, n
        assert getattr(L, n).argtypes is not None, n
    assert L.hdd_operator_project_workspace.restype is C.c_int64
    assert len(L.hdd_operator_project_workspace.argtypes) == 3
    assert len(L.hdd_operator_project.argtypes) == 16
    assert len(L.hdd_vectors_inner.argtypes) == 12
    assert callable(H.project) and callable(H.inner) and callable(H.project_workspace)
    assert H.MAX_BASIS == 64
    assert "#define HDD_MAX_BASIS 64" in open(H.HEADER).read()
    assert L.hdd_abi_version() == 8        # additive: the ABI version stays


def test_workspace_size():
    ws = H.lib().hdd_operator_project_workspace
    sizes = (1, 2, 15, 16, 17, 33, 63, H.MAX_BASIS)
    for q in (1, 2, H.MAX_COMP):
        for n in (1, 17, H.MAX_BASIS):
            by_v = [ws(q, k, n) for k in sizes]
            by_u = [ws(q, n, k) for k in sizes]
            assert all(s > 0 for s in by_v + by_u)
            assert all(a < b for a, b in zip(by_v, by_v[1:])) and all(a < b for a, b in zip(by_u, by_u[1:])), (q, n)
    by_q = [ws(q, 5, 7) for q in range(1, H.MAX_COMP + 1)]
    assert all(a < b for a, b in zip(by_q, by_q[1:]))
    assert ws(2, 5, 7) >= 2 * 5 * 7                       # at least one share
    assert ws(2, 5, 7) == ws(2, 5, 7) == H.project_workspace(2, 5, 7)
    # modest at the largest call: 512 shares of 8 x 64 x 64
    assert ws(H.MAX_COMP, H.MAX_BASIS, H.MAX_BASIS) * 8 <= 128 << 20
    for bad in (0, -1, H.MAX_BASIS + 1):
        assert ws(1, bad, 4) == 0 and ws(1, 4, bad) == 0, bad
    for bad in (0, -1, H.MAX_COMP + 1):
        assert ws(bad, 4, 4) == 0, bad


class _Operands:
    """valid-looking host descriptors; `fake` stands for a context / device array"""

    def __init__(self, n_rows=12, n_cols=12):
        self.keep = np.zeros(64)
        self.fake = self.keep.ctypes.data
        self.pat = H.CsrT(n_rows, n_cols, 48, self.fake, self.fake, self.fake)
        self.vals = (C.c_void_p * 1)(self.fake)
        self.mesh = H.MeshT(H.SIMPLEX, 1, 4, 0, 4, self.fake, self.fake, self.fake, None, None)

    def _g(self, k):
        if k is None:
            return None
        if k == "pat":
            return C.addressof(self.pat)
        return getattr(self, k)

    def project(self, ctx="fake", pattern="pat", vals="vals", v="fake", u="fake", work="fake", out="fake", n_comp=1,
                n_v=3, n_u=5, ldv=12, ldu=12, n_work=None, rng=None, mesh=None):
        g = self._g
        if n_work is None:
            n_work = H.lib().hdd_operator_project_workspace(H.MAX_COMP, H.MAX_BASIS, H.MAX_BASIS)
        r = None if rng is None else H.BlockRange(*rng)
        return H.lib().hdd_operator_project(g(ctx), None if mesh is None else C.addressof(mesh), g(pattern), g(vals), n_comp,
                                            None if r is None else C.addressof(r), g(v), ldv, n_v, g(u), ldu, n_u, g(work),
                                            n_work, g(out), None)

    def inner(self, ctx="fake", v="fake", w="fake", work="fake", out="fake", n_v=3, n_w=5, ldv=12, ldw=12, n=12, n_work=None):
        g = self._g
        if n_work is None:
            n_work = H.lib().hdd_operator_project_workspace(1, H.MAX_BASIS, H.MAX_BASIS)
        return H.lib().hdd_vectors_inner(g(ctx), g(v), ldv, n_v, g(w), ldw, n_w, n, g(work), n_work, g(out), None)


def _msg():
    return H.lib().hdd_last_error(None)


def test_rejects_null_arguments():
    o = _Operands()
    for k in ("ctx", "pattern", "vals", "v", "u", "work", "out"):
        assert o.project(**{k: None}) == 1, k
        assert _msg().startswith(WHO), k
    for k in ("ctx", "v", "w", "work", "out"):
        assert o.inner(**{k: None}) == 1, k
        assert _msg().startswith(WHO_INNER), k
    o.vals[0] = None                      # a null value array inside d_vals
    assert o.project() == 1 and _msg().startswith(WHO)
    assert H.lib().hdd_operator_project(None, None, None, None, 1, None, None, 0, 1, None, 0, 1, None, 0, None, None) == 1
    assert H.lib().hdd_vectors_inner(None, None, 0, 1, None, 0, 1, 0, None, 0, None, None) == 1


def test_n_comp():
    o = _Operands()
    for n in (0, -1, H.MAX_COMP + 1):
        assert o.project(n_comp=n) == 1, n
        assert _msg().startswith(WHO) and b"n_comp" in _msg(), (n, _msg())


def test_basis_sizes():
    o = _Operands()
    for n in (0, -1, H.MAX_BASIS + 1, 1000):
        for k in ("n_v", "n_u"):
            assert o.project(**{k: n}) == 1, (k, n)
            assert _msg().startswith(WHO) and b"HDD_MAX_BASIS" in _msg(), (k, n, _msg())
        for k in ("n_v", "n_w"):
            assert o.inner(**{k: n}) == 1, (k, n)
            assert _msg().startswith(WHO_INNER) and b"HDD_MAX_BASIS" in _msg(), (k, n, _msg())


def test_leading_dimensions():
    o = _Operands(n_rows=12, n_cols=9)
    assert o.project(ldv=11, ldu=9) == 1 and _msg().startswith(WHO) and b"ldv" in _msg()
    assert o.project(ldv=12, ldu=8) == 1 and _msg().startswith(WHO) and b"ldu" in _msg()
    # the range decides, not the pattern
    assert o.project(rng=(3, 9, 0, 6), ldv=5, ldu=6) == 1 and b"ldv" in _msg()
    assert o.project(rng=(3, 9, 0, 6), ldv=6, ldu=5) == 1 and b"ldu" in _msg()
    assert o.inner(ldv=11) == 1 and _msg().startswith(WHO_INNER) and b"ldv" in _msg()
    assert o.inner(ldw=11) == 1 and _msg().startswith(WHO_INNER) and b"ldw" in _msg()
    assert o.inner(n=-1) == 1 and _msg().startswith(WHO_INNER)


def test_workspace_too_small():
    o = _Operands()
    ws = H.lib().hdd_operator_project_workspace
    assert o.project(n_work=ws(1, 3, 5) - 1) == 1 and _msg().startswith(WHO) and b"n_work" in _msg()
    assert o.project(n_work=0) == 1 and b"n_work" in _msg()
    assert o.project(n_v=4, n_work=ws(1, 3, 5)) == 1 and b"n_work" in _msg()    # what 3 x 5 needs is not enough for 4 x 5
    assert o.inner(n_work=ws(1, 3, 5) - 1) == 1 and _msg().startswith(WHO_INNER) and b"n_work" in _msg()
    assert o.inner(n_work=-1) == 1 and b"n_work" in _msg()


def test_range_outside_the_matrix():
    o = _Operands()
    for rng in [(0, 13, 0, 12), (-1, 12, 0, 12), (0, 12, 0, 13), (6, 3, 0, 12), (0, 12, 9, 3)]:
        assert o.project(rng=rng) == 1, rng
        assert _msg().startswith(WHO) and b"range" in _msg(), (rng, _msg())


def test_mesh_that_does_not_match_the_pattern():
    o = _Operands(n_rows=15, n_cols=15)     # the mesh owns 4 elements: 12 rows
    assert o.project(mesh=o.mesh, ldv=15, ldu=15) == 1 and _msg().startswith(WHO) and b"pattern rows" in _msg()
