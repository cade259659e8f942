"""The operator-application entry points of the C ABI (hdd_operator_apply, hdd_operator_apply2,
hdd_last_apply_kernel): exported, bound by the Python front-end, and every argument check comes before the first
device call -- so they answer HDD_ERR_INVALID (1) here, without a GPU.  The pointers that stand for the context and
the device arrays are never dereferenced by a rejected call."""
import ctypes as C

import numpy as np

import hdd_amd as H

NAMES = ("hdd_operator_apply", "hdd_operator_apply2", "hdd_last_apply_kernel")


def test_symbols_exported_and_bound():
    L = H.lib()
    declared = H.declared_symbols()
    for n in NAMES:
        assert n in declared, n
        fn = getattr(L, n)
        assert fn.argtypes is not None, n
    assert L.hdd_last_apply_kernel.restype is C.c_char_p
    assert isinstance(H.last_apply_kernel(), str)
    assert H.MAX_VEC == 8
    assert L.hdd_abi_version() == 8        # additive: the ABI version stays


class _Operands:
    """valid-looking host descriptors; `fake` stands for a context / device array"""

    def __init__(self):
        self.keep = np.zeros(64)
        self.fake = self.keep.ctypes.data
        self.pat = H.CsrT(12, 12, 48, self.fake, self.fake, self.fake)
        self.vals = (C.c_void_p * 1)(self.fake)

    def apply(self, ctx="fake", pattern="pat", vals="vals", x="fake", y="fake", n_comp=1, n_vec=1, ldx=12, ldy=12,
              rng=None):
        g = lambda k: None if k is None else (C.addressof(self.pat) if k == "pat" else getattr(self, k))
        return H.lib().hdd_operator_apply(g(ctx), None, g(pattern), g(vals), n_comp, None,
                                          None if rng is None else C.addressof(rng), g(x), ldx, g(y), ldy, n_vec, None)

    def apply2(self, ctx="fake", pattern="pat", vals="vals", v="fake", u="fake", work="fake", out="fake", n_comp=1,
               n_v=1, n_u=1, ld=12, rng=None):
        g = lambda k: None if k is None else (C.addressof(self.pat) if k == "pat" else getattr(self, k))
        return H.lib().hdd_operator_apply2(g(ctx), None, g(pattern), g(vals), n_comp, None,
                                           None if rng is None else C.addressof(rng), g(v), ld, n_v, g(u), ld, n_u,
                                           g(work), ld, g(out), None)


def test_apply_rejects_null_arguments():
    o = _Operands()
    for k in ("ctx", "pattern", "vals", "x", "y"):
        assert o.apply(**{k: None}) == 1, k
        assert H.lib().hdd_last_error(None).startswith(b"hdd_operator_apply:")
    o.vals[0] = None                      # a null value array inside d_vals
    assert o.apply() == 1
    assert H.lib().hdd_operator_apply(None, None, None, None, 1, None, None, None, 0, None, 0, 1, None) == 1


def test_apply2_rejects_null_arguments():
    o = _Operands()
    for k in ("ctx", "pattern", "vals", "v", "u", "work", "out"):
        assert o.apply2(**{k: None}) == 1, k
        assert H.lib().hdd_last_error(None).startswith(b"hdd_operator_apply2:")


def test_vector_and_component_counts():
    o = _Operands()
    for n in (0, 9, -1):
        assert o.apply(n_vec=n) == 1, n
        assert b"n_vec" in H.lib().hdd_last_error(None)
        assert o.apply2(n_v=n) == 1 and o.apply2(n_u=n) == 1, n
    for n in (0, H.MAX_COMP + 1):
        assert o.apply(n_comp=n) == 1 and o.apply2(n_comp=n) == 1, n
        assert b"n_comp" in H.lib().hdd_last_error(None)


def test_leading_dimensions_and_ranges():
    o = _Operands()
    assert o.apply(ldx=11) == 1 and o.apply(ldy=11) == 1
    assert o.apply2(ld=11) == 1
    for r in [(-1, 12, 0, 12), (0, 13, 0, 12), (5, 4, 0, 12), (0, 12, 0, 13), (0, 12, 7, 6)]:
        rng = H.BlockRange(*r)
        assert o.apply(rng=rng) == 1, r
        assert b"range" in H.lib().hdd_last_error(None)
        assert o.apply2(rng=rng) == 1, r
    # a sub-range needs only its own leading dimensions -- but these would reach the device, so only the failing side:
    assert o.apply(rng=H.BlockRange(0, 6, 0, 9), ldx=8, ldy=6) == 1
