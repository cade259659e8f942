"""The entry points of the a-posteriori estimator (hdd_estimator_create / _destroy / _workspace, hdd_swipdg_estimate,
hdd_last_estimate_kernels): declared, exported, bound by the Python front-end, additive to ABI 8, and every argument
check comes before the first device call -- so they answer HDD_ERR_INVALID (1) / HDD_ERR_UNSUPPORTED (3) here, without
a GPU.  The estimator is a host-only one (created without a context); the pointers that stand for the context and the
device arrays are never dereferenced by a rejected call."""
import ctypes as C

import numpy as np
import pytest

import hdd_amd as H

NAMES = ("hdd_estimator_create", "hdd_estimator_destroy", "hdd_estimator_workspace", "hdd_estimator_set_residual_star",
         "hdd_swipdg_estimate", "hdd_last_estimate_kernels")
WHO = b"hdd_swipdg_estimate:"
INVALID, UNSUPPORTED = 1, 3


def _msg():
    return H.lib().hdd_last_error(None)


def test_symbols_exported_and_bound():
    L = H.lib()
    declared = H.declared_symbols()
    for n in NAMES:
        assert n in declared, n
        assert getattr(L, n).argtypes is not None, n
    assert L.hdd_estimator_workspace.restype is C.c_int64
    assert len(L.hdd_swipdg_estimate.argtypes) == 19
    assert len(L.hdd_estimator_create.argtypes) == 3
    assert callable(H.estimate) and callable(H.Estimator) and callable(H.last_estimate_kernels)
    assert L.hdd_abi_version() == 8        # additive: the ABI version stays
    assert isinstance(H.last_estimate_kernels(), str)


def test_create_rejects_what_is_out_of_scope():
    L = H.lib()
    h = C.c_void_p()
    quad = H.Grid.structured(H.CUBE, 4, 4).local()
    assert L.hdd_estimator_create(None, quad.h, C.byref(h)) == UNSUPPORTED and b"simplex" in _msg()
    hexa = H.Grid.structured3d((2, 2, 2)).local()
    assert L.hdd_estimator_create(None, hexa.h, C.byref(h)) == UNSUPPORTED and b"simplex" in _msg()
    ghosts = H.Grid.structured(H.SIMPLEX, 4, 4, px=2, py=1).local(0, 1)
    assert ghosts.n_ghost > 0
    assert L.hdd_estimator_create(None, ghosts.h, C.byref(h)) == UNSUPPORTED and b"ghosts" in _msg()
    neumann = H.Grid.structured(H.SIMPLEX, 4, 4, boundary=H.BOUNDARY_ALL_NEUMANN).local()
    assert L.hdd_estimator_create(None, neumann.h, C.byref(h)) == UNSUPPORTED and b"Neumann" in _msg()
    assert not h.value
    with pytest.raises(H.HddError):
        H.Estimator(None, quad)
    ok = H.Grid.structured(H.SIMPLEX, 4, 4).local()
    assert L.hdd_estimator_create(None, None, C.byref(h)) == INVALID
    assert L.hdd_estimator_create(None, ok.h, None) == INVALID


def test_workspace_size():
    L = H.lib()
    assert L.hdd_estimator_workspace(None) == 0
    assert L.hdd_estimator_set_residual_star(None, 1) == INVALID
    sizes = []
    for nx in (1, 4, 16, 64):
        loc = H.Grid.structured(H.SIMPLEX, nx, nx).local()
        est = H.Estimator(None, loc)
        n, nv = 2 * nx * nx, (nx + 1) ** 2
        # the Oswald value of every vertex, four partial sums per 256 elements, the four totals
        assert est.n_work >= nv + 4 * -(-n // 256) + 4
        assert est.n_work <= nv + 1 + 4 * -(-n // 256) + 4
        assert est.n_work == L.hdd_estimator_workspace(est.h)
        sizes.append(est.n_work)
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]


class _Operands:
    """valid-looking descriptors around a host-only estimator; `fake` stands for a context / device array"""

    def __init__(self, nx=4):
        self.keep = np.zeros(64)
        self.fake = self.keep.ctypes.data
        self.local = H.Grid.structured(H.SIMPLEX, nx, nx).local()
        self.est = H.Estimator(None, self.local)
        n = self.local.n_local
        self.mesh = H.MeshT(H.SIMPLEX, 1, n, 0, n, self.fake, self.fake, self.fake, self.fake, self.fake)
        self.kappa = (H.ScalarFn * 2)(H.ScalarFn(H.FN_CONST, 0, 1.0, 0, 0, 0, None, None, 0, 0),
                                      H.ScalarFn(H.FN_PER_ELEM, 0, 0.0, 0, 0, 0, self.fake, None, 0, 0))
        self.tensor = H.TensorFn(H.TENSOR_CONST, 0, (C.c_double * 6)(1, 0, 1, 0, 0, 0), None)
        self.force = H.ScalarFn(H.FN_COS_PRODUCT, 3, 1.0, 0, 1.0, 1.0, None, None, 0, 0)
        self.prm = H.params()
        self.sums = np.zeros(4)

    def call(self, ctx="fake", est="est", mesh="mesh", kappa="kappa", tensor="tensor", force="force", prm="prm", u="fake",
             work="fake", sums="sums", n_comp=2, n_work=None):
        def g(k):
            if k is None:
                return None
            if k == "fake":
                return self.fake
            if k == "est":
                return self.est.h
            if k == "sums":
                return self.sums.ctypes.data
            return C.addressof(getattr(self, k))
        if n_work is None:
            n_work = self.est.n_work
        return H.lib().hdd_swipdg_estimate(g(ctx), g(est), g(mesh), g(kappa), n_comp, None, None, None, g(tensor), g(force),
                                           g(prm), g(u), g(work), n_work, None, None, None, g(sums), None)


def test_rejects_null_arguments():
    o = _Operands()
    for k in ("ctx", "est", "mesh", "kappa", "tensor", "prm", "u", "work", "sums"):
        assert o.call(**{k: None}) == INVALID, k
        assert _msg().startswith(WHO) and b"null" in _msg(), k
    for n in (0, -1, H.MAX_COMP + 1):
        assert o.call(n_comp=n) == INVALID and b"n_comp" in _msg()


def test_workspace_too_small():
    o = _Operands()
    for n_work in (o.est.n_work - 1, 0, -1):
        assert o.call(n_work=n_work) == INVALID, n_work
        assert _msg().startswith(WHO) and b"n_work" in _msg()
    # every check passed: what is left is the host-only estimator, still without a device call
    assert o.call() == INVALID and b"host-only" in _msg()


def test_mesh_checks():
    o = _Operands()
    o.mesh.elem_vertices = None
    o.mesh.vertex_coords = None
    assert o.call() == INVALID and b"elem_vertices" in _msg()
    o = _Operands()
    o.mesh.n_local += 2
    o.mesh.own_end += 2
    assert o.call() == INVALID and b"n_local" in _msg()
    o = _Operands()
    o.mesh.face_info = None
    assert o.call() == INVALID and b"mesh arrays" in _msg()
    o = _Operands()
    o.kappa[1].per_elem = None
    assert o.call() == INVALID and b"per_elem" in _msg()


def test_unsupported_without_a_device():
    for field, bad, word in [("elem_type", H.CUBE, b"simplex"), ("elem_type", H.HEX, b"simplex"), ("degree", 2, b"degree"),
                             ("own_begin", 1, b"whole-grid"), ("own_end", 3, b"whole-grid")]:
        o = _Operands()
        setattr(o.mesh, field, bad)
        assert o.call() == UNSUPPORTED, (field, bad)
        assert _msg().startswith(WHO) and word in _msg(), (field, _msg())
    o = _Operands()
    o.kappa[0].kind = H.FN_SINUSOID        # a smooth diffusion factor
    assert o.call() == UNSUPPORTED and b"CONST or PER_ELEM" in _msg()
    o = _Operands()
    o.tensor.kind = 7
    assert o.call() == UNSUPPORTED and b"tensor" in _msg()
    o = _Operands()
    o.force.order = 7                      # rules of order 9 and 16: more points than the kernel's table holds
    assert o.call() == UNSUPPORTED and b"order" in _msg()
