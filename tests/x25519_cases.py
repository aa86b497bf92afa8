"""Crafted X25519 units, not a test module: low-order and non-canonical u-coordinates, points of the twist, one scalar
per bit position, every setting of the five clamped bits and the scalar extremes of the raw ladder, shared by
tests/test_x25519_edges_cpu.py (the C oracle agrees with the Python model on each) and tests/test_x25519_edges_gpu.py
(the device agrees with the model).

A unit is (raw, scalar, u): `scalar` is the 32 bytes handed to eccx_x25519 (little-endian under the RFC 7748 default,
big-endian under ECCX_X25519_RAW_LADDER), `u` the 32 little-endian bytes or None for the base-point path.  Expected
values come from oracle/ecc_ref.py (ref_x25519 / ref_ladder, Python integers) and are cached per distinct
(raw, scalar, u), about 1500 evaluations for everything here; larger batches repeat a small set of units."""
from __future__ import annotations

import functools
import random
from typing import List, NamedTuple, Optional, Sequence, Tuple

from oracle import ecc_ref as R

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
A = 486662
BASE_U = (9).to_bytes(32, "little")
ZERO = bytes(32)
CLAMPED_BITS = (0, 1, 2, 254, 255)
# RFC 7748 section 5.2: k = u = 9, then k, u = X25519(k, u), k; after 1 and after 1000 steps
RFC_ITER_1 = "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"
RFC_ITER_1000 = "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"

# the seven u-coordinates of the points of order dividing 8 (RFC 7748 section 6.1 lists them), and p, p + 1 as their
# non-canonical spellings below 2^255
ORDER8 = (325606250916557431795983626356110631294008115727848805560023387167927233504,
          39382357235489614581723060781553021112529911719440698176882885853963445705823)
LOW_ORDER = (0, 1, ORDER8[0], ORDER8[1], P - 1, P, P + 1)
LOW_ORDER_RAW_ONLY = (2 * P - 1, 2 * P, 2 * P + 1)   # bit 255 set: low order only where the bit is not masked


class Case(NamedTuple):
    group: str               # low_order, non_canonical, twist, bit, clamp, extreme, ordinary
    label: str
    raw: bool                # ECCX_X25519_RAW_LADDER
    scalar: bytes            # as the entry point takes it
    u: Optional[bytes]       # None: the base-point path (u = NULL)


def le(v: int) -> bytes:
    return v.to_bytes(32, "little")


def scalar_bytes(raw: bool, k: int) -> bytes:
    """The integer k as the mode's 32 scalar bytes."""
    return k.to_bytes(32, "big" if raw else "little")


def clamp(k: int) -> int:
    return (k & ~7 & ~(1 << 255)) | (1 << 254)


@functools.lru_cache(maxsize=None)
def _model(raw: bool, scalar: bytes, u: bytes) -> bytes:
    if raw:
        return le(R.ref_ladder(int.from_bytes(u, "little"), scalar))
    return R.ref_x25519(scalar, u)


def evaluations() -> int:
    """Distinct (raw, scalar, u) the model has been run on."""
    return _model.cache_info().currsize


def expected(c: Case) -> Tuple[bytes, int]:
    """(32 output bytes, flag): the flag is 1 exactly where the output is zero."""
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
    return rng.getrandbits(256)


def _rand_u(rng: random.Random) -> int:
    return rng.randrange(2, P - 1)


def on_twist(u: int) -> bool:
    """u^3 + A u^2 + u is a non-square: no point of the curve has this u, a point of the quadratic twist does."""
    v = (u * u * u + A * u * u + u) % P
    return v != 0 and pow(v, (P - 1) // 2, P) == P - 1


def montgomery_u(pt: Tuple[int, int]) -> int:
    """u = (1 + y) / (1 - y) of an Edwards point; the neutral element (y = 1) maps to 0, as invert_or_zero makes it"""
    y = pt[1]
    return (1 + y) * pow((1 - y) % P, P - 2, P) % P


def low_order_values(raw: bool) -> Tuple[int, ...]:
    return LOW_ORDER + (LOW_ORDER_RAW_ONLY if raw else ())


def _check_low_order(u: int) -> None:
    """what the issue asks the builder to establish before it uses a value: order dividing 8 in the raw ladder, and a
    zero result under a clamped scalar in either mode wherever the mode leaves the value low-order"""
    k = int.from_bytes(bytes(range(0xA1, 0xC1)), "big")   # arbitrary
    assert R.ref_ladder(u, b"\x08") == 0, u
    assert _model(True, scalar_bytes(True, clamp(k)), u.to_bytes(32, "little")) == ZERO, u
    if u < 2**255:
        assert _model(False, scalar_bytes(False, k), u.to_bytes(32, "little")) == ZERO, u


def _low_order(raw: bool, rng: random.Random) -> List[Case]:
    out = []
    ks = [_rand_scalar(rng), _rand_scalar(rng)]
    for u in LOW_ORDER + LOW_ORDER_RAW_ONLY:
        _check_low_order(u)
        # RFC mode: the three values above 2^255 lose their top bit and are ordinary points; kept as such.
        # raw mode: a clamped scalar (zero result) and scalars used as given (an odd one leaves a point of order 4 or 8)
        for j, k in enumerate([clamp(ks[0])] + ks if raw else ks):
            out.append(Case("low_order", f"u={u:#x} k{j}", raw, scalar_bytes(raw, k), le(u)))
    return out


def _non_canonical(raw: bool, rng: random.Random) -> List[Case]:
    k = scalar_bytes(raw, _rand_scalar(rng))
    if raw:
        vals = [2**255] + [2**255 + j for j in (1, 18, 19, 20)] + [2 * P + j for j in range(38)] + [2**256 - 1]
        vals += [P + j for j in range(19)]
    else:
        vals = [P + j for j in range(19)] + [(P + j) | (1 << 255) for j in range(19)]
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
    return le(_rand_u(random.Random(0x75 + int(raw))))


def _bits(raw: bool, rng: random.Random) -> List[Case]:
    u = shared_u(raw)
    out = []
    for t in range(256):
        k = scalar_bytes(raw, 1 << t)
        out.append(Case("bit", f"2^{t} base", raw, k, None))
        out.append(Case("bit", f"2^{t} u", raw, k, u))
    return out


def _clamp_variants(raw: bool, rng: random.Random) -> List[Case]:
    u = shared_u(raw)
    out = []
    for s in range(2):
        k0 = _rand_scalar(rng)
        for m in range(32):
            k = k0
            for j, t in enumerate(CLAMPED_BITS):
                k = (k & ~(1 << t)) | (((m >> j) & 1) << t)
            out.append(Case("clamp", f"s{s} m{m}", raw, scalar_bytes(raw, k), u))
    return out


EXTREMES = (0, 1, 2, 8, L - 1, L, L + 1, 8 * L, 2**255, 2**256 - 1)


def _extremes(raw: bool, rng: random.Random) -> List[Case]:
    u = shared_u(raw)
    out = []
    # the all-zero and the all-ff scalar in both modes; the rest are the raw ladder's
    for k in (EXTREMES if raw else (0, 2**256 - 1)):
        out.append(Case("extreme", f"k={k:#x} base", raw, scalar_bytes(raw, k), None))
        out.append(Case("extreme", f"k={k:#x} u", raw, scalar_bytes(raw, k), u))
    return out


@functools.lru_cache(maxsize=None)
def cases(raw: bool) -> Tuple[Case, ...]:
    """every crafted unit of one mode"""
    rng = random.Random(7748 + int(raw))
    out: List[Case] = []
    for build in (_low_order, _non_canonical, _twist, _bits, _clamp_variants, _extremes):
        out += build(raw, rng)
    return tuple(out)   # the raw extremes 1, 2, 8 and 2^255 are single-bit scalars too: listed as both


def select(raw: bool, with_u: bool, groups: Optional[Sequence[str]] = None) -> List[Case]:
    return [c for c in cases(raw) if (c.u is not None) == with_u and (groups is None or c.group in groups)]


@functools.lru_cache(maxsize=None)
def ordinary(raw: bool, with_u: bool, count: int = 29) -> Tuple[Case, ...]:
    """random scalars and random 32-byte strings for u: ordinary units (none of them yields zero)"""
    rng = random.Random(255 + 2 * int(raw) + int(with_u))
    out = tuple(Case("ordinary", str(i), raw, rng.randbytes(32), rng.randbytes(32) if with_u else None) for i in range(count))
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
    us = low_order_values(raw)
    return [Case("low_order", f"cycle {j}", raw, scalar_bytes(raw, clamp(ks[j % 3]) if raw else ks[j % 3]), le(us[j % len(us)]))
            for j in range(count)]
