"""GPU stress test of secp256k1's unsaturated field (P256K1U: 9 x 29-bit limbs, general Montgomery reduction) at the
operand bounds its types admit, through tests/hip_p256k1/libfieldcheck_k1.so: products and squares at the column
budget, the merged product of the mixed addition's Y3, the doubling's Y3 tail, subtraction chains, reductions from the
widest limbs, canonical output and the division-step inversion -- each against Python integers (residue, value bound,
limb bound), as tests/test_field_layer.py does for the other five fields."""
import ctypes
import os
import random

import numpy as np
import pytest

from tests.test_field_layer import check_out, gen, value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "hip_p256k1", "libfieldcheck_k1.so")
P = 2**256 - 2**32 - 977
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
(OP_MUL_TIGHT, OP_MUL_LAZY, OP_SQR_LAZY, OP_SUB_CHAIN, OP_REDUCE_MAX, OP_CANONICAL, OP_MUL_AUTO, OP_ADD_AUTO, OP_INVERT,
 OP_MUL_ADD, OP_MUL_BETA, OP_DBL_Y) = range(12)


class FieldCheckK1:
    def __init__(self):
        import torch  # noqa: F401  (one HIP runtime in the process, as eccoxide_amd._lib does)

        self.lib = ctypes.CDLL(LIB)
        self.lib.fieldcheck_k1_info.argtypes = [ctypes.POINTER(ctypes.c_int)]
        self.lib.fieldcheck_k1_run4.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_size_t]
        arr = (ctypes.c_int * 8)()
        assert self.lib.fieldcheck_k1_info(arr) == 0
        self.inf = dict(zip(["N", "B", "KMAX", "KKMAX", "KA", "KB", "KS", "L"], list(arr)))

    def run(self, op, a, b=None, c=None, d=None):
        a = np.ascontiguousarray(a, dtype=np.uint32)
        arrs = [a] + [np.ascontiguousarray(x if x is not None else a, dtype=np.uint32) for x in (b, c, d)]
        out = np.zeros_like(a)
        rc = self.lib.fieldcheck_k1_run4(op, *[x.ctypes.data for x in arrs], out.ctypes.data, a.shape[0])
        assert rc == 0, f"fieldcheck_k1_run4 failed: hip error {rc}"
        return out


@pytest.fixture(scope="module")
def fc():
    if not os.path.exists(LIB):
        pytest.fail("tests/hip_p256k1/libfieldcheck_k1.so missing: run __graft_entry__.build()")
    return FieldCheckK1()


def test_layout_without_gpu():
    """The layout the harness is built for (no GPU needed to read it)."""
    lib = ctypes.CDLL(LIB)
    arr = (ctypes.c_int * 8)()
    assert lib.fieldcheck_k1_info(arr) == 0
    assert list(arr)[:4] == [9, 29, 7, 6] and list(arr)[7] == 8


@pytest.mark.gpu
def test_products_at_the_operand_bounds(fc):
    rng = random.Random(256)
    inf = fc.inf
    rinv = pow(1 << (inf["B"] * inf["N"]), -1, P)
    n = 512
    cases = [(OP_MUL_TIGHT, (1, 3), (1, 3)),
             (OP_MUL_LAZY, (inf["KA"], 7), (inf["KB"], 4)),
             (OP_SQR_LAZY, (inf["KS"], 5), None),
             (OP_MUL_AUTO, (inf["KMAX"], 64), (inf["KMAX"], 64))]
    for op, (ka, va), bb in cases:
        a = gen(rng, inf, P, ka, va, n)
        b = gen(rng, inf, P, bb[0], bb[1], n) if bb else a
        out = fc.run(op, a, b)
        for i in range(n):
            want = value(a[i], inf["B"]) * value(b[i], inf["B"]) * rinv
            check_out(out[i], inf, P, want)
    # a * beta from the widest limbs (the endomorphism's x coordinate)
    a = gen(rng, inf, P, inf["KMAX"], 64, n)
    out = fc.run(OP_MUL_BETA, a)
    for i in range(n):
        check_out(out[i], inf, P, value(a[i], inf["B"]) * BETA)  # BETA is stored in Montgomery form: R cancels


@pytest.mark.gpu
def test_merged_products_and_doubling_tail(fc):
    rng = random.Random(257)
    inf = fc.inf
    B = inf["B"]
    rinv = pow(1 << (B * inf["N"]), -1, P)
    n = 768
    a, b, c, d = (gen(rng, inf, P, 1, 3, n) for _ in range(4))
    out = fc.run(OP_MUL_ADD, a, b, c, d)
    for i in range(n):
        va, vb, vc, vd = (value(x[i], B) for x in (a, b, c, d))
        check_out(out[i], inf, P, (va * (vb - vc) - vc * vd) * rinv)
    out = fc.run(OP_DBL_Y, a, b, c, d)
    for i in range(n):
        va, vb, vc, vd = (value(x[i], B) for x in (a, b, c, d))
        check_out(out[i], inf, P, va * (vb - vc) * rinv - 8 * vd * vd * rinv)


@pytest.mark.gpu
def test_sub_chain_and_reductions(fc):
    rng = random.Random(258)
    inf = fc.inf
    B, n = inf["B"], 512
    a, b = gen(rng, inf, P, 1, 3, n), gen(rng, inf, P, 1, 3, n)
    out = fc.run(OP_SUB_CHAIN, a, b)
    for i in range(n):
        check_out(out[i], inf, P, value(a[i], B) - 3 * value(b[i], B))
    a = gen(rng, inf, P, inf["KMAX"], 64, n)
    out = fc.run(OP_REDUCE_MAX, a)
    for i in range(n):
        check_out(out[i], inf, P, value(a[i], B))
    b = gen(rng, inf, P, inf["KMAX"], 64, n)
    out = fc.run(OP_ADD_AUTO, a, b)
    for i in range(n):
        check_out(out[i], inf, P, 2 * (value(a[i], B) + value(b[i], B)))


@pytest.mark.gpu
def test_canonical_output(fc):
    rng = random.Random(259)
    inf = fc.inf
    B, n = inf["B"], 512
    a = gen(rng, inf, P, inf["KMAX"], 64, n)
    rinv = pow(1 << (B * inf["N"]), -1, P)
    out = fc.run(OP_CANONICAL, a)
    for i in range(n):  # out of the Montgomery domain: the plain integer, fully reduced
        got = sum(int(x) << (32 * k) for k, x in enumerate(out[i][:8]))
        assert got == value(a[i], B) * rinv % P
        assert all(int(x) == 0 for x in out[i][8:])


@pytest.mark.gpu
def test_division_step_inversion(fc):
    rng = random.Random(260)
    vals = [0, 1, 2, P - 1, P - 2, 2**255, 2**256 - 2**32 - 978, 0x3D1, 2**32 + 977, (P + 1) // 2]
    vals += [rng.randrange(P) for _ in range(500)]
    a = np.zeros((len(vals), 9), dtype=np.uint32)
    for i, v in enumerate(vals):
        for k in range(8):
            a[i, k] = (v >> (32 * k)) & 0xFFFFFFFF
    out = fc.run(OP_INVERT, a)
    for i, v in enumerate(vals):
        got = sum(int(x) << (32 * k) for k, x in enumerate(out[i][:8]))
        assert got == (pow(v, -1, P) if v else 0), hex(v)
