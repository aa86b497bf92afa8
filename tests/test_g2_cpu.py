"""BLS12-381 G2 without a GPU: the Python model (tests/g2_ref.py) against the fixture extracted from the reference
(tests/golden/bls_g2.json), and what the C ABI, the Python layer and the C++ / Rust mirrors say about curve id 7."""
import ctypes
import hashlib
import json
import os
import random
import re

import pytest

from tests import g2_ref as G2
from tests import oracle_lib

FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bls_g2.json")))


def _f2(hexstr):
    v = G2.f2_from_bytes(bytes.fromhex(hexstr))
    assert v is not None
    return v


# ---- the model against the fixture -------------------------------------------------------------------------------
def test_parameters():
    p = FIX["params"]
    assert _f2(p["b"]) == G2.B and _f2(p["b3"]) == G2.B3
    assert (_f2(p["gx"]), _f2(p["gy"])) == G2.G
    assert _f2(p["psi_x_coeff"]) == G2.PSI_X and _f2(p["psi_y_coeff"]) == G2.PSI_Y


def test_generator_is_on_the_twist_and_has_order_r():
    assert G2.on_curve(G2.G)
    assert G2.mul(G2.R, G2.G) is None and G2.mul(G2.R - 1, G2.G) == G2.neg(G2.G)
    assert G2.in_subgroup(G2.G) and G2.in_subgroup_psi(G2.G)
    # the order of the twist: r h2 kills a point outside G2, r alone does not
    q = G2.point_of_x((1, 2))
    assert q is not None and G2.mul(G2.R * G2.H2, q) is None and G2.mul(G2.R, q) is not None


def test_group_law_cases():
    g, g2, g3 = G2.G, G2.mul(2, G2.G), G2.mul(3, G2.G)
    assert G2.add(g, g) == g2 and G2.add(g2, g) == g3 and G2.add(g, g2) == g3
    assert G2.add(g, G2.neg(g)) is None and G2.add(None, g) == g and G2.add(g, None) == g and G2.add(None, None) is None
    assert G2.on_curve(g2) and G2.on_curve(g3)
    rng = random.Random(1)
    for _ in range(4):
        a, b = rng.randrange(G2.R), rng.randrange(G2.R)
        assert G2.add(G2.mul(a, g), G2.mul(b, g)) == G2.mul((a + b) % G2.R, g)


def test_fp2_arithmetic():
    rng = random.Random(2)
    for _ in range(20):
        a, b = (rng.randrange(G2.P), rng.randrange(G2.P)), (rng.randrange(G2.P), rng.randrange(G2.P))
        assert G2.f2_mul(a, G2.f2_inv(a)) == G2.ONE
        assert G2.f2_sqr(a) == G2.f2_mul(a, a)
        assert G2.f2_mul(a, b) == G2.f2_mul(b, a)
        s = G2.f2_sqrt(G2.f2_sqr(a))
        assert s in (a, G2.f2_neg(a))
        assert G2.f2_is_largest(a) != G2.f2_is_largest(G2.f2_neg(a))
    assert not G2.f2_is_largest(G2.ZERO)
    half = (G2.P - 1) // 2
    assert not G2.f2_is_largest((half, 0)) and G2.f2_is_largest((half + 1, 0))
    assert G2.f2_is_largest((0, half + 1)) and not G2.f2_is_largest((G2.P - 1, half))
    nonsquares = [a for a in ((i, i + 1) for i in range(40)) if G2.f2_sqrt(a) is None]
    assert nonsquares  # the model rejects something


def test_serialization_kats():
    for e in FIX["serialization_kat"]:
        pt = G2.mul(e["k"], G2.G)
        c = bytes.fromhex(e["compressed"])
        assert G2.compress(pt) == c and G2.decompress(c, check_subgroup=True) == pt
        if "uncompressed" in e:
            u = bytes.fromhex(e["uncompressed"])
            assert G2.uncompressed(pt) == u and G2.from_uncompressed(u, check_subgroup=True) == pt
    assert G2.decompress(G2.compress(None)) is None and G2.from_uncompressed(G2.uncompressed(None)) is None


def test_rejection_rules():
    g = G2.compress(G2.G)
    assert G2.decompress(bytes([g[0] & 0x7F]) + g[1:]) == G2.REJECT                 # not the compressed flavour
    assert G2.decompress(bytes([0xE0]) + bytes(95)) == G2.REJECT                      # infinity with the sort bit
    assert G2.decompress(bytes([0xC0]) + bytes(94) + b"\x01") == G2.REJECT            # infinity with a payload
    pbytes = G2.P.to_bytes(48, "big")
    assert G2.decompress(bytes([pbytes[0] | 0x80]) + pbytes[1:] + bytes(48)) == G2.REJECT   # c1 = p
    assert G2.decompress(bytes([0x80]) + bytes(47) + pbytes) == G2.REJECT             # c0 = p
    x_off = next(x for x in ((i, i + 1) for i in range(40)) if G2.point_of_x(x) is None)
    assert G2.decompress(bytes([0x80 | G2.f2_to_bytes(x_off)[0]]) + G2.f2_to_bytes(x_off)[1:]) == G2.REJECT
    u = bytearray(G2.uncompressed(G2.G))
    u[-1] ^= 1
    assert G2.from_uncompressed(bytes(u)) == G2.REJECT                                # y off the curve
    good = G2.uncompressed(G2.G)
    assert G2.from_uncompressed(bytes([good[0] | 0x80]) + good[1:]) == G2.REJECT
    assert G2.from_uncompressed(bytes([good[0] | 0x20]) + good[1:]) == G2.REJECT
    assert G2.from_uncompressed(bytes([0x40]) + bytes(190) + b"\x01") == G2.REJECT


def test_off_subgroup_vectors():
    for e in FIX["off_subgroup"]:
        c, u = bytes.fromhex(e["compressed"]), bytes.fromhex(e["uncompressed"])
        pt = G2.decompress(c)
        assert pt not in (None, G2.REJECT) and G2.from_uncompressed(u) == pt and G2.on_curve(pt)
        assert G2.compress(pt) == c and G2.uncompressed(pt) == u
        assert G2.mul(G2.R, pt) is not None and not G2.in_subgroup_psi(pt)
        assert G2.decompress(c, check_subgroup=True) == G2.REJECT and G2.from_uncompressed(u, check_subgroup=True) == G2.REJECT


def test_comb_samples():
    comb = FIX["comb"]
    assert comb["windows"] == 64 and sorted(comb["samples"]) == ["0", "1", "31", "63"]
    for w, entries in comb["samples"].items():
        assert len(entries) == 15
        base = G2.mul(16 ** int(w), G2.G)
        acc = None
        for j, (x, y) in enumerate(entries):
            acc = G2.add(acc, base)
            assert (_f2(x), _f2(y)) == acc, (w, j)


def test_psi_is_multiplication_by_the_seed_on_g2():
    x = G2.R - G2.SEED_ABS  # the seed is negative
    for k in (1, 2, 12345, G2.R - 1):
        q = G2.mul(k, G2.G)
        assert G2.psi(q) == G2.mul(x, q) and G2.in_subgroup_psi(q)
    assert G2.in_subgroup_psi(None)


def test_torsion_points_exist():
    for order in (13, 23):
        t = G2.torsion_point(order)
        assert G2.on_curve(t) and G2.mul(order, t) is None and not G2.in_subgroup(t)
        assert not G2.in_subgroup_psi(G2.add(G2.G, t))


# ---- the C ABI and its mirrors -----------------------------------------------------------------------------------
def test_abi_sizes():
    import eccoxide_amd as E
    from eccoxide_amd import _lib

    lib = _lib.load()
    assert E.BLS12_381_G2 == 7 and E.curve_id("bls12_381_g2") == 7 and E.CURVE_NAMES[7] == "bls12_381_g2"
    assert lib.eccx_field_bytes(7) == 96 and lib.eccx_scalar_bytes(7) == 32 and lib.eccx_compressed_bytes(7) == 96
    assert E.field_bytes("bls12_381_g2") == 96 and E.scalar_bytes("bls12_381_g2") == 32
    # id 6 stays unassigned, nothing follows 7
    for cid in (6, 8):
        assert lib.eccx_field_bytes(cid) < 0 and lib.eccx_scalar_bytes(cid) < 0 and lib.eccx_compressed_bytes(cid) < 0


def test_workload_order():
    from eccoxide_amd import workload as W

    assert W.order("bls12_381_g2") == G2.R == W.order("bls12_381_g1")
    ks = W.random_scalars("bls12_381_g2", 16, seed=1)
    assert ks.shape == (16, 32)


def test_unserved_entry_points_are_argument_errors_without_a_context():
    """Without a device there is no context; what can be pinned here is that nothing served or unserved crashes on id 7
    and that the answer is an argument error, not ECCX_ERR_CURVE (-1), which id 6 gets.  tests/test_g2_gpu.py repeats the
    unserved combinations on a live context."""
    from eccoxide_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(384)
    assert lib.eccx_double_scalarmul(None, 7, 1, buf, buf, buf, buf, buf, 0) == -2
    assert lib.eccx_scalarmul_var(None, 7, 1, buf, buf, buf, buf, buf, 0) == -2
    assert lib.eccx_scalarmul_base(None, 7, 1, buf, buf, buf, None, 1 << 10) == -2
    assert lib.eccx_ecdsa_verify(None, 7, 1, buf, 32, buf, buf, buf, 0) == -2
    assert lib.eccx_prepare(None, 7, 2) == -2
    assert lib.eccx_prepare(None, 6, 2) in (-1, -2)


def test_mirrors_carry_the_id():
    root = oracle_lib.ROOT
    hdr = open(os.path.join(root, "include", "eccx.h")).read()
    assert re.search(r"ECCX_BLS12_381_G2 = 7\b", hdr) and "id 6 stays unassigned" in hdr
    hpp = open(os.path.join(root, "include", "eccx.hpp")).read()
    assert re.search(r"struct Bls12381G2\b", hpp) and "ECCX_BLS12_381_G2" in hpp
    m = re.search(r"struct Bls12381G2 \{(.*?)\};", hpp, re.S)
    assert m and re.search(r"FB = 96\b", m.group(1)) and re.search(r"SB = 32\b", m.group(1))
    ffi = open(os.path.join(root, "rust", "eccoxide-gpu", "src", "ffi.rs")).read()
    assert "pub const ECCX_BLS12_381_G2: c_int = 7;" in ffi


def test_generated_constants_are_current():
    """curve_consts.inc carries the G2 struct the generator writes, with the fixture's generator and psi coefficients."""
    txt = open(os.path.join(oracle_lib.ROOT, "eccoxide_amd", "csrc", "curve_consts.inc")).read()
    body = txt[txt.index("struct BLS12_381_G2 {"):]
    body = body[: body.index("\n};")]
    rr = 1 << (28 * 14)

    def digits(v):
        v = v * rr % G2.P
        return ", ".join("0x%08xu" % ((v >> (28 * i)) & 0x0FFFFFFF) for i in range(14))

    for name, val in (("GX", G2.GX), ("GY", G2.GY), ("PSI_X", G2.PSI_X), ("PSI_Y", G2.PSI_Y)):
        for c in (0, 1):
            assert "%s%d[14] = {%s}" % (name, c, digits(val[c])) in body, name
    assert "CB[14] = {%s}" % digits(4) in body and "CB3[14] = {%s}" % digits(12) in body


def test_fixture_is_small_and_hash_is_a_sha256():
    path = os.path.join(os.path.dirname(__file__), "golden", "bls_g2.json")
    assert os.path.getsize(path) < 64 * 1024
    assert len(bytes.fromhex(FIX["comb"]["sha256_xy_concat"])) == hashlib.sha256().digest_size
