"""Crafted X448 units, not a test module: low-order and non-canonical u-coordinates, points of the twist, one scalar
per bit position, every setting of the three clamped bits and the scalar extremes of the raw ladder, shared by
tests/test_x448_cpu.py (the model's own facts) and tests/test_x448_edges_gpu.py (the device agrees with the model).

A unit is (raw, scalar, u): `scalar` is the 56 bytes handed to eccx_x448 (little-endian under the RFC 7748 default,
big-endian under ECCX_X448_RAW_LADDER), `u` the 56 little-endian bytes or None for the base-point path.  Expected
values come from tests/x448_ref.py (Python integers) and are cached per distinct (raw, scalar, u), under 1500
evaluations (about 5 ms each) for everything here; larger batches repeat a small set of units."""
from __future__ import annotations

import functools
import random
from typing import List, NamedTuple, Optional, Sequence, Tuple

from tests import x448_ref as R

P, L = R.P, R.L
BASE_U = R.le(R.BASE_U)
ZERO = bytes(56)
CLAMPED_BITS = (0, 1, 447)
# RFC 7748 section 5.2: k = u = 5, then k, u = X448(k, u), k; after 1 and after 1000 steps
RFC_ITER_1 = "3f482c8a9f19b01e6c46ee9711d9dc14fd4bf67af30765c2ae2b846a4d23a8cd0db897086239492caf350b51f833868b9bc2b3bca9cf4113"
RFC_ITER_1000 = "aa3b4749d55b9daf1e5b00288826c467274ce3ebbdd5c17b975e09d4af6c67cf10d087202db88286e2b79fceea3ec353ef54faa26e219f38"

# the u-coordinates of the points of order 1, 2 and 4 on the curve (0, -1) and of order 2 and 4 on its twist (0, 1),
# with p and p + 1 as the non-canonical spellings of 0 and 1: every bit of u is taken, so all five are low order in
# both modes
LOW_ORDER = (0, 1, P - 1, P, P + 1)
# RFC mode's scalars for the "bit" group: around the clamp, the byte and the 28-bit limb boundaries, phi, the top
RFC_BITS = (0, 1, 2, 7, 8, 27, 28, 29, 55, 56, 57, 223, 224, 225, 439, 440, 446, 447)


class Case(NamedTuple):
    group: str               # low_order, non_canonical, twist, bit, clamp, extreme, ordinary
    label: str
    raw: bool                # ECCX_X448_RAW_LADDER
    scalar: bytes            # as the entry point takes it
    u: Optional[bytes]       # None: the base-point path (u = NULL)


le = R.le


def scalar_bytes(raw: bool, k: int) -> bytes:
    """The integer k as the mode's 56 scalar bytes."""
    return k.to_bytes(56, "big" if raw else "little")


def clamp(k: int) -> int:
    return (k & ~3) | (1 << 447)


@functools.lru_cache(maxsize=None)
def _model(raw: bool, scalar: bytes, u: bytes) -> bytes:
    if raw:
        return le(R.ladder(int.from_bytes(u, "little"), scalar))
    return R.x448(scalar, u)


def evaluations() -> int:
    """Distinct (raw, scalar, u) the model has been run on."""
    return _model.cache_info().currsize


def expected(c: Case) -> Tuple[bytes, int]:
    """(56 output bytes, flag): the flag is 1 exactly where the output is zero."""
    out = _model(c.raw, c.scalar, BASE_U if c.u is None else c.u)
    return out, 1 if out == ZERO else 0


def want(cases: Sequence[Case]) -> Tuple[bytes, bytes]:
    ex = [expected(c) for c in cases]
    return b"".join(e[0] for e in ex), bytes(e[1] for e in ex)


def pack(cases: Sequence[Case]) -> Tuple[bytes, Optional[bytes]]:
    """(scalars, u) of one call; the units must agree on the mode and on whether u is given."""
    assert len({(c.raw, c.u is None) for c in cases}) <= 1
    return b"".join(c.scalar for c in cases), (None if not cases or cases[0].u is None else b"".join(c.u for c in cases))


def _rand_scalar(rng: random.Random) -> int:
    return rng.getrandbits(448)


def _rand_u(rng: random.Random) -> int:
    return rng.randrange(2, P - 1)


on_twist = R.on_twist


def check_facts() -> None:
    """what the issue asks the builder to establish before it uses a value: the five low-order values give zero under
    any clamped scalar (a multiple of 4) in either mode, [2] and [4] of each are zero and [1] is u mod p in the raw
    ladder; u = -1 is on the curve and u = 1 on the twist; the base point has order L"""
    k = int.from_bytes(bytes(range(0xA1, 0xA1 + 56)), "big")   # arbitrary
    for u in LOW_ORDER:
        ub = le(u)
        assert _model(True, scalar_bytes(True, clamp(k)), ub) == ZERO, u
        assert _model(False, scalar_bytes(False, k), ub) == ZERO, u
        assert R.ladder(u, b"\x02") == 0 and R.ladder(u, b"\x04") == 0 and R.ladder(u, b"\x01") == u % P, u
    assert not on_twist(P - 1) and R.rhs(P - 1) != 0 and on_twist(1)
    assert R.ladder(R.BASE_U, L.to_bytes(56, "big")) == 0
    assert R.ladder(R.BASE_U, (L + 1).to_bytes(56, "big")) == R.BASE_U == R.ladder(R.BASE_U, (L - 1).to_bytes(56, "big"))


def _low_order(raw: bool, rng: random.Random) -> List[Case]:
    out = []
    ks = [_rand_scalar(rng), _rand_scalar(rng)]
    for u in LOW_ORDER:
        # RFC mode: every scalar is clamped on use (zero result).  raw mode: a clamped scalar (zero result), scalars
        # used as given and odd ones, which leave the low-order point itself
        for j, k in enumerate([clamp(ks[0])] + ks + ([ks[0] | 1, (ks[1] | 1) ^ 2] if raw else [])):
            out.append(Case("low_order", f"u={u:#x} k{j}", raw, scalar_bytes(raw, k), le(u)))
    return out


def _non_canonical(raw: bool, rng: random.Random) -> List[Case]:
    k = scalar_bytes(raw, _rand_scalar(rng))
    vals = [P + j for j in range(19)] + [2**448 - 1 - j for j in range(4)] + [2**224 - 1, 2**224 + 1, 2**447]
    return [Case("non_canonical", f"u={v:#x}", raw, k, le(v)) for v in vals]


def _twist(raw: bool, rng: random.Random) -> List[Case]:
    out = []
    while len(out) < 4:
        u = _rand_u(rng)
        if on_twist(u):
            out.append(Case("twist", f"u={u:#x}", raw, scalar_bytes(raw, _rand_scalar(rng)), le(u)))
    return out


def shared_u(raw: bool) -> bytes:
    """the one random u the scalar cases of a mode run against (besides the base point), so that their outputs compare"""
    return le(_rand_u(random.Random(0x448 + int(raw))))


def _bits(raw: bool, rng: random.Random) -> List[Case]:
    u = shared_u(raw)
    out = []
    for t in (range(448) if raw else RFC_BITS):
        k = scalar_bytes(raw, 1 << t)
        if not raw or t % 28 in (0, 27) or t % 8 in (0, 7):   # raw mode, base point: the limb and byte boundaries
            out.append(Case("bit", f"2^{t} base", raw, k, None))
        out.append(Case("bit", f"2^{t} u", raw, k, u))
    return out


def _clamp_variants(raw: bool, rng: random.Random) -> List[Case]:
    u = shared_u(raw)
    out = []
    for s in range(2):
        k0 = _rand_scalar(rng)
        for m in range(8):
            k = k0
            for j, t in enumerate(CLAMPED_BITS):
                k = (k & ~(1 << t)) | (((m >> j) & 1) << t)
            out.append(Case("clamp", f"s{s} m{m}", raw, scalar_bytes(raw, k), u))
    return out


EXTREMES = (0, 1, 2, 4, L - 1, L, L + 1, 4 * L, 2**447, 2**448 - 1)


def _extremes(raw: bool, rng: random.Random) -> List[Case]:
    u = shared_u(raw)
    out = []
    # the all-zero and the all-ff scalar in both modes; the rest are the raw ladder's
    for k in (EXTREMES if raw else (0, 2**448 - 1)):
        out.append(Case("extreme", f"k={k:#x} base", raw, scalar_bytes(raw, k), None))
        out.append(Case("extreme", f"k={k:#x} u", raw, scalar_bytes(raw, k), u))
    return out


@functools.lru_cache(maxsize=None)
def cases(raw: bool) -> Tuple[Case, ...]:
    """every crafted unit of one mode"""
    rng = random.Random(7748 + 448 + int(raw))
    out: List[Case] = []
    for build in (_low_order, _non_canonical, _twist, _bits, _clamp_variants, _extremes):
        out += build(raw, rng)
    return tuple(out)   # the raw extremes 1, 2, 4 and 2^447 are single-bit scalars too: listed as both


def select(raw: bool, with_u: bool, groups: Optional[Sequence[str]] = None) -> List[Case]:
    return [c for c in cases(raw) if (c.u is not None) == with_u and (groups is None or c.group in groups)]


@functools.lru_cache(maxsize=None)
def ordinary(raw: bool, with_u: bool, count: int = 29) -> Tuple[Case, ...]:
    """random scalars and random 56-byte strings for u: ordinary units (none of them yields zero)"""
    rng = random.Random(448 + 2 * int(raw) + int(with_u))
    out = tuple(Case("ordinary", str(i), raw, rng.randbytes(56), rng.randbytes(56) if with_u else None) for i in range(count))
    assert all(expected(c)[1] == 0 for c in out)
    return out


def interleaved(raw: bool, with_u: bool) -> List[Case]:
    """every crafted unit of (mode, u given or not) with an ordinary unit after each"""
    plain = ordinary(raw, with_u)
    out = [plain[-1], plain[-2], plain[-3]]
    for i, c in enumerate(select(raw, with_u)):
        out += [c, plain[i % len(plain)]]
    return out


def periodic(raw: bool, with_u: bool, period: int = 97) -> List[Case]:
    """`period` distinct units to repeat through a large batch: the ordinary ones and crafted ones spread evenly over
    the groups, zero results among them"""
    spread = lambda xs, m: xs if len(xs) <= m else [xs[(i * len(xs)) // m] for i in range(m)]
    plain = list(ordinary(raw, with_u))
    need = period - len(plain)
    picked = spread([c for c in select(raw, with_u) if c.group not in ("bit", "clamp")], need // 2)
    seen = {c.scalar for c in picked}
    picked += spread([c for c in select(raw, with_u, ("bit", "clamp")) if c.scalar not in seen], need - len(picked))
    if len(picked) < need:   # RFC mode on the base point has few crafted units: more ordinary ones make up the period
        plain += list(ordinary(raw, with_u, count=29 + need - len(picked)))[29:]
    out = []
    for i in range(period):   # crafted and ordinary units alternate while both last
        src = picked if (i % 2 == 0 and picked) or not plain else plain
        out.append(src.pop(0))
    assert len(out) == period and len({(c.scalar, c.u) for c in out}) == period
    return out


def low_order_units(raw: bool, count: int) -> List[Case]:
    """`count` units with a low-order u, the values cycling; under RFC clamping (and under the raw mode's clamped
    scalars used here) each yields zero"""
    rng = random.Random(8)
    ks = [_rand_scalar(rng) for _ in range(3)]
    return [Case("low_order", f"cycle {j}", raw, scalar_bytes(raw, clamp(ks[j % 3]) if raw else ks[j % 3]),
                 le(LOW_ORDER[j % len(LOW_ORDER)])) for j in range(count)]
