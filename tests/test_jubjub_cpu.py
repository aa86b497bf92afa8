"""Jubjub without a GPU: the Python model against the reference's vectors and comb table, the generated constants, the
ABI's sizes and argument errors for curve id 9, the mirrors of the id, and the codec model."""
import ctypes
import hashlib
import json
import os
import random
import re

import pytest

from tests import jubjub_ref as J
from tests import oracle_lib

with open(os.path.join(os.path.dirname(__file__), "golden", "jubjub.json")) as f:
    FIX = json.load(f)


def test_model_constants_match_the_fixture():
    p = FIX["params"]
    assert int(p["d"], 16) == J.D and int(p["d2"], 16) == 2 * J.D % J.Q and int(p["a"], 16) == J.Q - 1
    assert int(p["gx"], 16) == J.GX and int(p["gy"], 16) == J.GY and int(p["gt"], 16) == J.GX * J.GY % J.Q
    assert int(p["order"], 16) == J.R
    assert J.on_curve(J.G)
    # what makes the unified addition complete on the whole curve, and the decoder free of a v == 0 case
    assert J.is_square(-1) and not J.is_square(J.D) and not J.is_square(-pow(J.D, -1, J.Q))


def test_kat():
    assert len(FIX["kat"]) == 6
    for v in FIX["kat"]:
        want = (int(v["x"], 16), int(v["y"], 16))
        assert J.mul(J.G, v["k"]) == want
        k_be = v["k"].to_bytes(32, "big")
        assert J.batch_affine([J.scale_bytes_ext(J.G, k_be)])[0] == want
    assert J.add(J.G, J.G) == (int(FIX["kat"][0]["x"], 16), int(FIX["kat"][0]["y"], 16))  # plain affine arithmetic gives 2 G


def test_generator_has_order_r():
    assert J.mul(J.G, J.R) == J.NEUTRAL and J.mul(J.G, J.R - 1) == J.neg(J.G)
    assert J.mul(J.G, 0) == J.NEUTRAL and J.mul(J.G, 8 * J.R) == J.NEUTRAL


def test_comb_table_matches_the_reference():
    raw = J.comb_table_bytes()
    assert len(raw) == 64 * 15 * 64
    assert hashlib.sha256(raw).hexdigest() == FIX["comb"]["sha256_xy_concat"]
    for w, rows in FIX["comb"]["samples"].items():
        for j, (x, y) in enumerate(rows):
            at = (int(w) * 15 + j) * 64
            assert raw[at:at + 64].hex() == x + y, (w, j)


def test_fixture_is_small():
    path = os.path.join(os.path.dirname(__file__), "golden", "jubjub.json")
    assert os.path.getsize(path) < 32 * 1024
    assert len(bytes.fromhex(FIX["comb"]["sha256_xy_concat"])) == hashlib.sha256().digest_size
    assert sorted(FIX["comb"]["samples"]) == ["0", "1", "31", "63"]


def test_generated_constants_are_current():
    """curve_consts.inc carries the two Jubjub structs the generator writes: digits of GX, GY, D, D2, ONE and the
    Tonelli-Shanks constants in JUBJUBU (9 x 29, R = 2^261), limbs in JUBJUB (8 x 32, R = 2^256)."""
    txt = open(os.path.join(oracle_lib.ROOT, "eccoxide_amd", "csrc", "curve_consts.inc")).read()
    body = txt[txt.index("struct JUBJUBU {"):]
    body = body[: body.index("\n};")]

    def digits(v, bits, n, mont=True):
        v = v * (1 << (bits * n)) % J.Q if mont else v
        return ", ".join("0x%08xu" % ((v >> (bits * i)) & ((1 << bits) - 1)) for i in range(n))

    for name, val in (("GX", J.GX), ("GY", J.GY), ("D", J.D), ("D2", 2 * J.D % J.Q), ("ONE", 1), ("TS_Z", J.TS_Z)):
        assert "%s[9] = {%s}" % (name, digits(val, 29, 9)) in body, name
    assert "P[9] = {%s}" % digits(J.Q, 29, 9, mont=False) in body
    assert "RP = 70u" in body and "KIND = 1;" in body and "N = 9;" in body and "B = 29;" in body
    e = (J.TS_T - 1) // 2
    assert "ROOT_BITS = %d;" % e.bit_length() in body
    assert "ROOT_EXP[7] = {%s}" % ", ".join("0x%08xu" % ((e >> (32 * i)) & 0xFFFFFFFF) for i in range(7)) in body
    sat = txt[txt.index("struct JUBJUB {"):]
    sat = sat[: sat.index("\n};")]
    for name, val in (("GX", J.GX), ("GY", J.GY), ("D2", 2 * J.D % J.Q), ("ONE", 1)):
        assert "%s[8] = {%s}" % (name, digits(val, 32, 8)) in sat, name
    assert "IO_BE = true" in sat and "TS_S = 32" in sat and "FB = 32" in sat and "SB = 32" in sat


def test_abi_sizes():
    import eccoxide_amd as E
    from eccoxide_amd import _lib

    lib = _lib.load()
    assert E.JUBJUB == 9 and E.curve_id("jubjub") == 9 and E.CURVE_NAMES[9] == "jubjub"
    assert lib.eccx_field_bytes(9) == 32 and lib.eccx_scalar_bytes(9) == 32 and lib.eccx_compressed_bytes(9) == 32
    assert E.field_bytes("jubjub") == 32 and E.scalar_bytes("jubjub") == 32
    for cid in (6, 8, 10):  # 6 and 8 stay unassigned, nothing follows 9
        assert lib.eccx_field_bytes(cid) == -1 and lib.eccx_scalar_bytes(cid) == -1 and lib.eccx_compressed_bytes(cid) == -1


def test_workload_order():
    from eccoxide_amd import workload as W

    assert W.order("jubjub") == J.R
    ks = W.random_scalars("jubjub", 16, seed=1)
    assert ks.shape == (16, 32) and all(0 < int.from_bytes(k.tobytes(), "big") < J.R for k in ks)


def test_entry_points_are_argument_errors_without_a_context():
    """Without a device there is no context: nothing served or unserved crashes on id 9, and the answer is an argument
    error (-2), never ECCX_ERR_CURVE (-1).  tests/test_jubjub_gpu.py repeats the refused options on a live context."""
    from eccoxide_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    assert lib.eccx_scalarmul_var(None, 9, 1, buf, buf, buf, buf, None, 0) == -2
    assert lib.eccx_scalarmul_base(None, 9, 1, buf, buf, buf, None, 1 << 2) == -2      # ECCX_TABLE_IN_LDS
    assert lib.eccx_scalarmul_base(None, 9, 1, buf, buf, buf, None, (1 << 8) | (1 << 10)) == -2  # ECCX_CT_GATHER
    assert lib.eccx_point_decompress(None, 9, 1, buf, buf, buf, 1 << 6) == -2          # ECCX_CHECK_SUBGROUP
    assert lib.eccx_double_scalarmul(None, 9, 1, buf, buf, buf, buf, buf, 0) == -2
    assert lib.eccx_ecdsa_verify(None, 9, 1, buf, 32, buf, buf, buf, 0) == -2
    assert lib.eccx_prepare(None, 9, 2) == -2 and lib.eccx_reserve(None, 9, 1, 1) == -2
    assert lib.eccx_comb_table(None, 9, buf) == -2


def test_mirrors_carry_the_id():
    root = oracle_lib.ROOT
    hdr = open(os.path.join(root, "include", "eccx.h")).read()
    assert re.search(r"ECCX_JUBJUB = 9\b", hdr) and "id 6 stays unassigned" in hdr and "id 8 stays unassigned" in hdr
    hpp = open(os.path.join(root, "include", "eccx.hpp")).read()
    m = re.search(r"struct Jubjub \{(.*?)\};", hpp, re.S)
    assert m and "ECCX_JUBJUB" in m.group(1) and re.search(r"FB = 32\b", m.group(1)) and re.search(r"SB = 32\b", m.group(1))
    ffi = open(os.path.join(root, "rust", "eccoxide-gpu", "src", "ffi.rs")).read()
    assert "pub const ECCX_JUBJUB: c_int = 9;" in ffi


def test_sqrt_model():
    rng = random.Random(32)
    assert J.sqrt(0) == 0 and J.sqrt(1) in (1, J.Q - 1)
    assert J.sqrt(5) is None and J.sqrt(J.TS_Z) is None  # 5 and the root of unity of order 2^32 are non-residues
    for k in (0, 1, 2, 16, 31, 32):  # a^t of order exactly 2^k: z^(2^(32-k)) times a 2^32-th power; k = 32 is no square
        a = pow(J.TS_Z, 1 << (32 - k), J.Q) * pow(rng.randrange(1, J.Q), 1 << 32, J.Q) % J.Q
        assert pow(pow(a, J.TS_T, J.Q), 1 << k, J.Q) == 1 and (k == 0 or pow(pow(a, J.TS_T, J.Q), 1 << (k - 1), J.Q) != 1)
        x = J.sqrt(a)
        assert (x is None) if k == 32 else (x is not None and x * x % J.Q == a)
    for _ in range(50):
        a = rng.randrange(J.Q)
        x = J.sqrt(a)
        assert (x is not None) == J.is_square(a) and (x is None or x * x % J.Q == a)


def test_codec_model_roundtrips_and_rejects():
    rng = random.Random(216)
    small = J.small_order_points(rng)
    pts = [J.G, J.neg(J.G), J.NEUTRAL, small[2], small[4], small[8], J.add(J.G, small[8])] + [J.random_point(rng) for _ in range(20)]
    for P in pts:
        assert J.on_curve(P)
        enc = J.compress(P)
        assert len(enc) == 32 and J.decompress(enc) == P
    assert J.compress(J.NEUTRAL) == b"\x01" + bytes(31)
    # the three rejections: y >= q; no point above y; x = 0 (y = 1, y = -1) with the sign bit set
    assert J.decompress(J.Q.to_bytes(32, "little")) is None and J.decompress(((1 << 255) - 1).to_bytes(32, "little")) is None
    y = next(y for y in range(2, 100) if not J.is_square((y * y - 1) * pow(J.D * y * y + 1, -1, J.Q)))
    assert J.decompress(y.to_bytes(32, "little")) is None
    for y in (1, J.Q - 1):
        enc = bytearray(y.to_bytes(32, "little"))
        assert J.decompress(bytes(enc)) == (0, y)
        enc[31] |= 0x80
        assert J.decompress(bytes(enc)) is None
    # about half of all y have a point above them
    hits = sum(J.decompress(rng.randrange(J.Q).to_bytes(32, "little")) is not None for _ in range(200))
    assert 60 <= hits <= 140


def test_small_order_points():
    small = J.small_order_points(random.Random(8))
    assert small[2] == (0, J.Q - 1)
    for order in (4, 8):
        P = small[order]
        assert J.on_curve(P) and J.mul(P, order) == J.NEUTRAL and J.mul(P, order // 2) != J.NEUTRAL
