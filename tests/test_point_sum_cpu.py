"""eccx_point_sum without a GPU: the symbols are exported and bound, the argument checks that come before any device is
touched, and the models the GPU tests compare with agree with each other on a sum.  CPU only."""
import ctypes

import numpy as np

from oracle import ecc_ref as R1
from tests import g2_ref as G2
from tests import msm_ref as M


def test_symbols_are_exported_and_bound():
    from eccoxide_amd import _lib

    lib = _lib.load()
    for name in ("eccx_point_sum", "eccx_point_sum_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).restype is ctypes.c_int
    assert len(_lib.SYMBOLS["eccx_point_sum"][1]) == 10 and len(_lib.SYMBOLS["eccx_point_sum_dev"][1]) == 11


def test_null_context_is_refused_before_anything_else():
    from eccoxide_amd import _lib

    lib = _lib.load()
    offs = np.array([0, 1, 2], dtype=np.uint64)
    out, fl = ctypes.create_string_buffer(b"\x5a" * 192, 192), ctypes.create_string_buffer(b"\x5a\x5a", 2)
    for curve in (3, 7, 0, 99):
        assert lib.eccx_point_sum(None, curve, 2, offs.ctypes.data, 2, bytes(192), None, out, fl, 0) == -2
        assert lib.eccx_point_sum_dev(None, curve, 2, None, 2, None, None, None, None, 0, None) == -2
        assert lib.eccx_point_sum(None, curve, 0, None, 0, None, None, None, None, 0) == -2
    assert (out.raw, fl.raw) == (b"\x5a" * 192, b"\x5a\x5a")


def test_the_engine_layer_and_the_wrappers_name_the_entry_point():
    import os

    import eccoxide_amd as E
    from tests.oracle_lib import ROOT

    for name in ("point_sum", "point_sum_t", "bls_aggregate"):
        assert callable(getattr(E.Engine, name)), name
    assert "eccx_point_sum(" in open(os.path.join(ROOT, "include", "eccx.hpp")).read()
    assert "ffi::eccx_point_sum(" in open(os.path.join(ROOT, "rust", "eccoxide-gpu", "src", "bls.rs")).read()


def test_models_sum_of_multiples():
    """sum r_j G = (sum r_j mod r) G in both models, the identity of the GPU tests' expected values; a point and its negative
    cancel, and an outsider of order 13 cancels after 13 additions."""
    rs = [5, M.ORDER - 3, 1 << 200, 77]
    k = sum(rs) % M.ORDER
    acc1, acc2 = None, None
    for r in rs:
        acc1 = R1.affine_add(M.C, acc1, R1.affine_mul(M.C, r, M.G))
        acc2 = G2.add(acc2, G2.mul(r, G2.G))
    assert acc1 == R1.affine_mul(M.C, k, M.G) and acc2 == G2.mul(k, G2.G)
    assert R1.affine_add(M.C, acc1, M.neg(acc1)) is None and G2.add(acc2, G2.neg(acc2)) is None
    t, acc = G2.torsion_point(13), None
    for _ in range(13):
        acc = G2.add(acc, t)
    assert acc is None and not G2.in_subgroup_psi(t)
