"""Model of booth_digit_aligned<WB, SB, S> (kernels_unsat.hpp): the public ladder's signed windows aligned to the TOP of
the 8 SB + 1 Booth positions.  S = (8 SB + 1) mod WB scalar bits stay below the main windows:
  main window w   bits WB w + S .. WB w + S + WB - 1, borrow bit WB w + S - 1
  bottom digit    bits S - 1 .. 0, no borrow below bit 0
The model reads the same bytes with the same shifts and masks as the device function."""
import random

import pytest

from oracle import ecc_ref as R

CASES = [(5, 32, "p256r1"), (5, 66, "p521r1")]


def aligned_digit(kb: bytes, wb: int, sb: int, s: int, w: int) -> int:
    """booth_digit_aligned, statement by statement; w = -1 is the bottom digit"""
    bottom = w < 0
    pos = 7 if bottom else wb * w + s - 1 + 8
    width = s if bottom else wb
    bi = pos >> 3
    b0 = kb[sb - bi] if 1 <= bi <= sb else 0
    b1 = kb[sb - bi - 1] if bi + 1 <= sb else 0
    wv = ((b0 | (b1 << 8)) >> (pos & 7)) & ((2 << width) - 1)
    neg = (wv >> width) & 1
    m = ((2 << width) - wv - 1) if neg else wv
    d = (m >> 1) + (m & 1)
    return -d if neg else d


def recode(k: int, wb: int, sb: int):
    s = (8 * sb + 1) % wb
    nmain = (8 * sb + 1) // wb
    kb = k.to_bytes(sb, "big")
    return s, [aligned_digit(kb, wb, sb, s, w) for w in range(nmain)], aligned_digit(kb, wb, sb, s, -1)


def structured_scalars(wb, sb, curve):
    """small values, single digits 2^S d 32^w and their neighbours, all ones, n + j, 2^256 - 1"""
    n = R.CURVES[curve].n
    s = (8 * sb + 1) % wb
    top = 1 << (8 * sb)
    ks = [0, 1, 2, 3, top - 1, (1 << 256) - 1]
    for w in (0, 1, 7, 25, 50, (8 * sb + 1) // wb - 1):
        for d in (1, 15, 16, 17):
            v = (d << s) << (wb * w)
            ks += [v - 1, v, v + 1]
    ks += [n + j for j in range(-40, 41)]
    return [k for k in ks if 0 <= k < top]


def scalars(wb, sb, curve):
    rng = random.Random(0xB007 + sb)
    return structured_scalars(wb, sb, curve) + [rng.randrange(1 << (8 * sb)) for _ in range(2000)]


@pytest.mark.parametrize("wb,sb,curve", CASES)
def test_aligned_digits_reconstruct_the_scalar(wb, sb, curve):
    assert (8 * sb + 1) % wb == {32: 2, 66: 4}[sb]
    for k in scalars(wb, sb, curve):
        s, main, bot = recode(k, wb, sb)
        assert sum(d << (wb * w + s) for w, d in enumerate(main)) + bot == k, hex(k)
        assert all(abs(d) <= 1 << (wb - 1) for d in main), hex(k)
        assert main[-1] >= 0, hex(k)  # the ladder starts from the top entry as it stands
        assert abs(bot) <= 1 << (s - 1), hex(k)


def test_p384_keeps_its_windows():
    assert (8 * 48 + 1) % 5 == 0  # S = 0: the ladder keeps booth_digit there
