"""The device functions of hashing to BLS12-381 G2, through tests/hip_h2c_g2/libh2cg2check.so: expand_message_xmd at 8 and
4 blocks against the Python expander at every message length 0 .. 139 and tags of every kind of length; hash_to_field's
component order; sgn0 for m = 2; sqrt_ratio on seeded pairs that cover all eight classes of mu_8; the map against the
fixture's u -> Q pairs, the edge elements and random ones; the isogeny at its kernel; and the product's map and cofactor
kernels from given elements and given points (the identity, G, points of order 13 and 23, a point already in G2)."""
import ctypes
import os
import random

import numpy as np
import pytest

from tests import g2_ref as G2
from tests import h2c_g2_ref as H
from tests.h2c_ref import expand_message_xmd
from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "hip_h2c_g2", "libh2cg2check.so")
P = H.P


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime in the process, as eccoxide_amd._lib does)

    if not os.path.exists(LIB):
        pytest.fail("tests/hip_h2c_g2/libh2cg2check.so missing: run __graft_entry__.build()")
    h = ctypes.CDLL(LIB)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    h.h2cg2check_expand.argtypes = [ci, sz, vp, sz, vp, vp, sz, vp]
    h.h2cg2check_hash_to_field.argtypes = [ci, sz, vp, sz, vp, vp, sz, vp, vp]
    h.h2cg2check_sgn0.argtypes = [sz, vp, vp]
    h.h2cg2check_sqrt_ratio.argtypes = [sz, vp, vp, vp, vp]
    h.h2cg2check_iso.argtypes = [sz, vp, vp, vp, vp, vp]
    h.h2cg2check_map.argtypes = [ci, ci, sz, vp, vp, vp]
    h.h2cg2check_clear.argtypes = [sz, vp, vp, vp, vp]
    return h


def _pack(msgs):
    blob = b"".join(msgs)
    offsets = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=offsets[1:])
    return blob, offsets


def _fb(elems):
    return b"".join(G2.f2_to_bytes(e) for e in elems)


def _records(pts):
    recs = [G2.to_record(p) for p in pts]
    return b"".join(r[0] for r in recs), bytes(r[1] for r in recs)


MSGS = [bytes((37 * k + i) & 0xFF for i in range(k)) for k in range(140)]  # every block boundary of b_0
TAGS = [bytes((7 * i + k) & 0xFF for i in range(k)) for k in (0, 1, 43, 255, 300)]  # 300: hashed down on the host


@pytest.mark.parametrize("ell", [8, 4])
def test_expand_message_xmd(lib, ell):
    blob, offsets = _pack(MSGS)
    for dst in TAGS:
        out = ctypes.create_string_buffer(32 * ell * len(MSGS))
        assert lib.h2cg2check_expand(ell, len(MSGS), blob, len(blob), offsets.ctypes.data, dst if dst else None, len(dst), out) == 0
        for i, m in enumerate(MSGS):
            assert out.raw[32 * ell * i:32 * ell * (i + 1)] == expand_message_xmd(m, dst, 32 * ell), (len(dst), len(m))


@pytest.mark.parametrize("key,count", [("g2_ro", 2), ("g2_nu", 1)])
def test_hash_to_field_component_order(lib, key, count):
    """element j = e_2j + e_(2j+1) u: c0 from the earlier block; the fixture's u values and 300 lanes against the model"""
    fx = H.FIXTURE[key]
    dst = fx["dst"].encode()
    msgs = [v["msg"].encode() for v in fx["vectors"]] + MSGS + MSGS + MSGS[:15]
    blob, offsets = _pack(msgs)
    out, flags = ctypes.create_string_buffer(96 * count * len(msgs)), ctypes.create_string_buffer(len(msgs))
    assert lib.h2cg2check_hash_to_field(count, len(msgs), blob, len(blob), offsets.ctypes.data, dst, len(dst), out, flags) == 0
    assert flags.raw == bytes(len(msgs))
    want = {}
    for i, m in enumerate(msgs):
        if m not in want:
            want[m] = _fb(H.hash_to_field(m, dst, count))
        assert out.raw[96 * count * i:96 * count * (i + 1)] == want[m], i
    for i, v in enumerate(fx["vectors"]):
        assert out.raw[96 * count * i:96 * count * (i + 1)].hex() == "".join(v["u"])


def test_sgn0(lib):
    cases = [(0, 0), (0, 1), (0, 2), (1, 0), (2, 1), (0, P - 1), (P - 1, 0), (P - 1, P - 1)]
    rng = random.Random(4)
    cases += [(rng.randrange(P), rng.randrange(P)) for _ in range(56)]
    out = ctypes.create_string_buffer(len(cases))
    assert lib.h2cg2check_sgn0(len(cases), _fb(cases), out) == 0
    assert list(out.raw) == [H.sgn0(c) for c in cases]
    assert list(out.raw[:8]) == [0, 1, 0, 1, 0, 0, 0, 0]


def test_sqrt_ratio(lib):
    """the contract: the verdict is the squareness of u / v, and y^2 v = u or y^2 v = Z u.  The seeded pairs cover all
    eight classes of (u / v)^((q - 1) / 8) (tests/test_h2c_g2_cpu.py checks that); then u = 0: square, root 0."""
    pairs = H.sqrt_ratio_samples() + [(G2.ZERO, (3, 4)), (G2.ZERO, G2.ONE)]
    n = len(pairs)
    y, verdict = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(n)
    assert lib.h2cg2check_sqrt_ratio(n, _fb([p[0] for p in pairs]), _fb([p[1] for p in pairs]), y, verdict) == 0
    for i, (u, v) in enumerate(pairs):
        r = G2.f2_from_bytes(y.raw[96 * i:96 * i + 96])
        assert r is not None
        qr = H.is_square(G2.f2_mul(u, G2.f2_inv(v)))
        assert verdict.raw[i] == int(qr), i
        assert G2.f2_mul(G2.f2_sqr(r), v) == (u if qr else G2.f2_mul(H.Z, u)), i
    assert verdict.raw[256:] == b"\x01\x01" and y.raw[96 * 256:] == bytes(192)
    assert 0 < sum(verdict.raw[:256]) < 256


def _map(lib, count, clear, us):
    n = len(us) // count
    out, flags = ctypes.create_string_buffer(192 * n), ctypes.create_string_buffer(n)
    assert lib.h2cg2check_map(count, clear, n, _fb(us), out, flags) == 0
    return out.raw, flags.raw


def test_map_to_curve(lib):
    rng = random.Random(12)
    us, want = [], []
    for key in ("g2_ro", "g2_nu"):  # the 15 u -> Q pairs of appendix J.10
        for v in H.FIXTURE[key]["vectors"]:
            for u, q in zip(v["u"], v["q"]):
                us.append(H.fe(u))
                want.append((H.fe(q[0]), H.fe(q[1])))
    assert len(us) == 15
    more = [G2.ZERO, G2.ONE, (P - 1, 0), (0, 1), (0, P - 1), (P - 1, P - 1)]
    more += [(rng.randrange(P), rng.randrange(P)) for _ in range(250)]
    us += more
    want += [H.map_to_curve(u) for u in more]
    assert all(q is not None and G2.on_curve(q) for q in want)
    got = _map(lib, 1, 0, us)
    wb, wf = _records(want)
    for i in range(len(us)):
        assert (got[0][192 * i:192 * i + 192], got[1][i]) == (wb[192 * i:192 * i + 192], wf[i]), us[i]


def test_isogeny_at_its_kernel_is_the_identity(lib):
    """x' = x_T fed directly (no point of E' has it): both denominators vanish, Z = 0; beside it an ordinary point of E'
    as the fraction xn / xd with xd != 1"""
    xt = H.iso_kernel_x()
    pt = H.map_to_curve_sswu((3, 5))
    d = (7, 11)
    xn = [xt, G2.f2_mul(xt, d), G2.f2_mul(pt[0], d), pt[0]]
    xd = [G2.ONE, d, d, G2.ONE]
    ys = [G2.ONE, (2, 3), pt[1], pt[1]]
    out, flags = ctypes.create_string_buffer(192 * 4), ctypes.create_string_buffer(4)
    assert lib.h2cg2check_iso(4, _fb(xn), _fb(xd), _fb(ys), out, flags) == 0
    want = _records([None, None, H.iso_map(pt), H.iso_map(pt)])
    assert (out.raw, flags.raw) == want and flags.raw == bytes([1, 1, 0, 0])


def test_finish_special_pairs(lib):
    """130 lanes of ordinary pairs with the special ones at lanes 0, 63, 64 and 129: (u, u) doubles, (u, -u) is the
    identity (flag 1, 192 zero bytes), (0, 0) doubles the image of zero; then encode_to_curve's tail on two workgroups"""
    rng = random.Random(382)
    el = lambda: (rng.randrange(P), rng.randrange(P))
    pairs = [(el(), el()) for _ in range(130)]
    a, b = el(), el()
    pairs[0] = (a, a)
    pairs[63] = (b, G2.f2_neg(b))
    pairs[64] = (G2.ZERO, G2.ZERO)
    pairs[129] = (b, b)
    want = [H.finish(list(p)) for p in pairs]
    assert want[63] is None and want[0] is not None and want[64] is not None
    got = _map(lib, 2, 1, [u for p in pairs for u in p])
    wb, wf = _records(want)
    assert got[1] == wf and got[1][63] == 1 and got[0][192 * 63:192 * 64] == bytes(192)
    assert got[0] == wb
    singles = [el() for _ in range(258)] + [G2.ZERO]
    assert _map(lib, 1, 1, singles) == _records([H.finish([u]) for u in singles])


def test_clear_cofactor(lib):
    """the identity, G, the fixture's Q0 + Q1 (twist points outside G2), points of order 13 and 23 (cleared to the
    identity), a point already in G2 ([4x^2 - 2x - 1]P, not P), on two workgroups with the special points spread out"""
    rng = random.Random(7)
    sums = []
    for v in H.FIXTURE["g2_ro"]["vectors"]:
        (a, b), (c, d) = v["q"]
        sums.append(G2.add((H.fe(a), H.fe(b)), (H.fe(c), H.fe(d))))
    in_g2 = G2.mul(0x1234567, G2.G)
    t13, t23 = G2.torsion_point(13), G2.torsion_point(23)
    special = [None, G2.G, t13, t23, in_g2, G2.add(t13, G2.G)] + sums
    filler = [H.map_to_curve((rng.randrange(P), rng.randrange(P))) for _ in range(16)]
    pts = [filler[i % 16] for i in range(300)]
    for k, s in enumerate(special):
        pts[(k * 29) % 300] = s
    pts[63], pts[64], pts[255], pts[256], pts[299] = t13, None, G2.G, t23, in_g2
    cache = {}
    want = []
    for p in pts:
        if p not in cache:
            cache[p] = H.clear_cofactor(p)
        want.append(cache[p])
    assert cache[None] is None and cache[t13] is None and cache[t23] is None
    assert cache[in_g2] != in_g2 and cache[in_g2] == G2.mul((4 * G2.SEED_ABS ** 2 + 2 * G2.SEED_ABS - 1) % G2.R, in_g2)
    assert all(cache[s] == H.clear_cofactor_heff(s) for s in sums)
    recs, inf = _records(pts)
    out, flags = ctypes.create_string_buffer(192 * 300), ctypes.create_string_buffer(300)
    assert lib.h2cg2check_clear(300, recs, inf, out, flags) == 0
    wb, wf = _records(want)
    for i in range(300):
        assert (out.raw[192 * i:192 * i + 192], flags.raw[i]) == (wb[192 * i:192 * i + 192], wf[i]), i
