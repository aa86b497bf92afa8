"""The public a = -3 ladders (kernels_coz.hpp, CT = false) after two changes to what a unit shares and when it adds:
  shared inversion   the four waves of a workgroup leave their table denominators in LDS; one of them (the duty wave,
                     rotating over the grid-stride iterations) inverts the product of threads c, 64 + c, 128 + c and
                     192 + c and hands every lane its own inverse.  A degenerate unit enters the product as 1.
  aligned windows    P-256 and P-521 align their Booth windows to the top: S = 2 / 4 doublings and one addition from
                     a short bottom digit close the ladder (tests/test_booth_aligned_cpu.py is the recoding's model).
Every result is compared with the oracle byte for byte."""
import random

import numpy as np
import pytest

from eccoxide_amd import workload as W
from oracle import ecc_ref as R
from tests.test_booth_aligned_cpu import structured_scalars
from tests.test_p256_ladder_edges import edge_scalars

pytestmark = pytest.mark.gpu

CURVES = ["p256r1", "p384r1", "p521r1"]
SHAPES = [(c, False) for c in CURVES] + [("p256r1", True)]
SHAPE_IDS = [c + ("-fused" if f else "") for c, f in SHAPES]
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
# Waves per SIMD the ladders are compiled for (coz_occupancy), which is also their workgroups per CU; the host sizes
# the grid from the runtime's occupancy query, which the hardware caps at MAX_WAVES per SIMD whatever it answers.
OCCUPANCY = {"p256r1": 4, "p384r1": 3, "p521r1": 2}
MAX_WAVES = 8
POOL = 1024

_pool = {}


def base_pool(oracle, curve):
    """POOL valid points per curve, computed once: (bytes, width of a point)"""
    if curve not in _pool:
        _pool[curve] = oracle.base(curve, W.random_scalars(curve, POOL, seed=4100).tobytes(), threads=16)[0]
    return _pool[curve], 2 * R.CURVES[curve].fb


def bases(oracle, curve, n, shift=0):
    pool, pb = base_pool(oracle, curve)
    reps = (n + shift + POOL - 1) // POOL + 1
    return (pool * reps)[shift * pb:(shift + n) * pb]


def take(buf, width, idxs):
    return b"".join(buf[i * width:(i + 1) * width] for i in idxs)


def run(engine, oracle, curve, fused, ks, pts, u1=None, validate=False):
    """-> (bytes, flags) of the engine; u1: the fused shape's fixed-base scalars"""
    if fused:
        return engine.double_scalarmul(curve, u1, ks, pts, validate=validate)
    return engine.scalarmul_var(curve, ks, pts, validate=validate)


def expected(oracle, curve, fused, ks, pts, u1=None):
    """the oracle's (bytes, flags) for the units given"""
    want = oracle.var(curve, ks, pts, threads=16)
    if not fused:
        return want
    C = R.CURVES[curve]
    pb, n = 2 * C.fb, len(ks) // C.sb
    A = oracle.base(curve, u1, threads=16)

    def pt(buf, fl, i):
        return None if fl[i] else (int.from_bytes(buf[i * pb:i * pb + C.fb], "big"), int.from_bytes(buf[i * pb + C.fb:(i + 1) * pb], "big"))

    out, flags = bytearray(), bytearray()
    for i in range(n):
        s = R.affine_add(C, pt(A[0], A[1], i), pt(want[0], want[1], i))
        out += bytes(pb) if s is None else s[0].to_bytes(C.fb, "big") + s[1].to_bytes(C.fb, "big")
        flags.append(1 if s is None else 0)
    return bytes(out), bytes(flags)


def compare(got, want, pb, idxs, want_idxs=None):
    """units idxs of got against units want_idxs (default: the same) of want"""
    for i, j in zip(idxs, idxs if want_idxs is None else want_idxs):
        assert got[1][i] == want[1][j] and got[0][i * pb:(i + 1) * pb] == want[0][j * pb:(j + 1) * pb], i


@pytest.mark.parametrize("curve,fused", SHAPES, ids=SHAPE_IDS)
def test_sizes_around_waves_and_workgroups(engine, oracle, curve, fused):
    """fewer units than waves, a wave and a workgroup boundary, lanes that only compute the clamped unit"""
    C = R.CURVES[curve]
    nmax = max(SIZES)
    ks = W.random_scalars(curve, nmax, seed=4101).tobytes()
    u1 = W.random_scalars(curve, nmax, seed=4102).tobytes()
    pts = bases(oracle, curve, nmax)
    want = expected(oracle, curve, fused, ks, pts, u1)
    for n in SIZES:
        got = run(engine, oracle, curve, fused, ks[:n * C.sb], pts[:n * 2 * C.fb], u1[:n * C.sb])
        assert len(got[1]) == n
        compare(got, want, 2 * C.fb, range(n))


@pytest.mark.parametrize("curve,fused", SHAPES, ids=SHAPE_IDS)
def test_second_grid_stride_iteration(engine, oracle, curve, fused):
    """300 units more than one grid's worth of lanes: their lanes run a second iteration, with another duty wave.
    Every unit of the second pass and a seeded sample of 512 others against the oracle.  The host sizes the grid from
    the runtime's occupancy query; should that ever grant more workgroups than the ladders are compiled for, the
    second size still has a second pass: 300 units more than the largest grid the hardware can hold (today that is
    passes 2 .. MAX_WAVES / OCCUPANCY + 1; the first 300 units of each, the last 300 and a sample of 512)."""
    import torch

    C = R.CURVES[curve]
    pb = 2 * C.fb
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lanes = OCCUPANCY[curve] * cus * 256
    nmax = MAX_WAVES * cus * 256 + 300
    ks = W.random_scalars(curve, nmax, seed=4103).tobytes()
    u1 = W.random_scalars(curve, nmax, seed=4104).tobytes()
    pts = bases(oracle, curve, nmax)
    for n in (lanes + 300, nmax):
        later = set()
        for first in list(range(lanes, n, lanes)) + [n - 300]:
            later.update(range(first, min(first + 300, n)))
        idxs = sorted(later | set(random.Random(4105).sample(range(n), 512)))
        want = expected(oracle, curve, fused, take(ks, C.sb, idxs), take(pts, pb, idxs), take(u1, C.sb, idxs))
        got = run(engine, oracle, curve, fused, ks[:n * C.sb], pts[:n * pb], u1[:n * C.sb])
        assert len(got[1]) == n
        compare(got, want, pb, idxs, range(len(idxs)))


@pytest.mark.parametrize("validate", [False, True], ids=["plain", "validate"])
@pytest.mark.parametrize("curve,fused", SHAPES, ids=SHAPE_IDS)
def test_degenerate_units_do_not_poison_their_column(engine, oracle, curve, fused, validate):
    """Bases whose table build degenerates ((x, 0): the first doubling; (0, 0): every step) at one thread of a column
    (wave 1 only), at two and at all four: the other units of those columns, and every other unit, are the oracle's.
    The degenerate units themselves are redone by the generic ladder, which sees nothing but the unit's own bytes:
    they carry the flag and the bytes of a batch that holds the degenerate units alone, one to a column, which are the
    parent's; with validation they are rejected."""
    C = R.CURVES[curve]
    fb, pb = C.fb, 2 * C.fb
    n = 4 * 256 + 70
    pts = bytearray(bases(oracle, curve, n, shift=17))
    bad = [64 + 5]                                        # workgroup 0: thread 5 of wave 1 only
    bad += [256 + 64 * w + 9 for w in range(4)]           # workgroup 1: column 9 in all four waves
    bad += [512 + 64 * w + 63 for w in (0, 3)]            # workgroup 2: column 63, waves 0 and 3
    bad += [768 + 64 * w + 0 for w in (1, 2, 3)]          # workgroup 3: column 0, all but wave 0
    bad += [1024 + 64 + 2, n - 1]                         # workgroup 4 (partly filled); the unit its idle lanes clamp to
    for j, i in enumerate(bad):
        if j % 2 == 0:
            pts[i * pb + fb:(i + 1) * pb] = bytes(fb)     # (x, 0)
        else:
            pts[i * pb:(i + 1) * pb] = bytes(pb)          # (0, 0)
    pts = bytes(pts)
    good = bytearray(pts)
    for i in bad:                                         # the oracle gets a valid stand-in there
        good[i * pb:(i + 1) * pb] = pts[0:pb]
    ks = W.random_scalars(curve, n, seed=4106).tobytes()
    u1 = W.random_scalars(curve, n, seed=4107).tobytes()
    want = expected(oracle, curve, fused, ks, bytes(good), u1)
    got = run(engine, oracle, curve, fused, ks, pts, u1, validate=validate)
    compare(got, want, pb, [i for i in range(n) if i not in bad])
    if validate:
        for i in bad:
            assert got[1][i] == 2 and got[0][i * pb:(i + 1) * pb] == bytes(pb), i
    else:
        assert len(bad) <= 64  # one column each, all in wave 0; the other waves' lanes clamp to the last of them
        alone = run(engine, oracle, curve, fused, take(ks, C.sb, bad), take(pts, pb, bad), take(u1, C.sb, bad))
        assert all(f in (0, 1) for f in alone[1])
        compare(got, alone, pb, bad, range(len(bad)))


def _edge_set(curve):
    C = R.CURVES[curve]
    rng = random.Random(0x5A1 + C.sb)
    ks = structured_scalars(5, C.sb, curve)
    if curve == "p256r1":
        ks = edge_scalars(rng) + ks
    ks = [k for k in ks if 0 <= k < 1 << (8 * C.sb)]
    out = []
    for k in ks:  # ordinary lanes between them, in the same wavefronts
        out += [k, rng.randrange(1, C.n)]
    return out


@pytest.mark.parametrize("curve,fused", SHAPES, ids=SHAPE_IDS)
def test_edge_scalars_among_random_lanes(engine, oracle, curve, fused):
    """Scalars at which the ladder's incomplete additions are patched (k = n + j: accumulator == +-entry at the last
    addition, which is now the short bottom one; small k: the accumulator at infinity until the bottom digit; single
    digits followed by zero digits), every other lane an ordinary scalar"""
    C = R.CURVES[curve]
    ks = _edge_set(curve)
    n = len(ks)
    kb = b"".join(k.to_bytes(C.sb, "big") for k in ks)
    rng = random.Random(0x5A2)
    u1 = b"".join((rng.randrange(0, C.n) if i % 3 else 0).to_bytes(C.sb, "big") for i in range(n))
    pts = bases(oracle, curve, n, shift=3)
    want = expected(oracle, curve, fused, kb, pts, u1)
    got = run(engine, oracle, curve, fused, kb, pts, u1)
    compare(got, want, 2 * C.fb, range(n))
    if not fused:
        assert want[1][ks.index(C.n)] == 1  # k = n: the point at infinity
