"""The models of the batched multi-scalar multiplication (tests/msm_batch_ref.py) against themselves and against the C
ABI's pure function: the sort key's round trip, the width function's contract and the limit rule.  eccx_msm_batch_window_bits
touches no device, so it is called here too; on the code before eccx_msm_batch the symbol is missing and the library does
not bind."""
import pytest

from tests import msm_batch_ref as MB
from tests import msm_ref as M

MS = (1, 2, 64, 1 << 20)


@pytest.fixture(scope="module")
def lib():
    from eccoxide_amd import _lib

    return _lib.load()


@pytest.mark.parametrize("c", range(MB.MIN_BITS, MB.MAX_BITS + 1))
def test_key_round_trip(c):
    W, B = M.windows(c), 1 << (c - 1)
    m = 5
    seen = []
    for g in (0, m - 1):
        for w in (0, W - 1):
            for d in (1, B):
                key = MB.key_of(g, w, d, c)
                assert MB.key_inverse(key, c) == (g, w, d)
                seen.append(key)
    assert seen == sorted(seen) and len(set(seen)) == len(seen)  # (vector, window, bucket) orders the keys
    assert seen[0] == 0 and seen[-1] == m * W * B - 1            # the key space is exactly m * W * B
    # a vector's last key and the next vector's first are neighbours
    assert MB.key_of(1, 0, 1, c) == MB.key_of(0, W - 1, B, c) + 1


def test_width_function_properties(lib):
    for m in MS:
        last = 0
        for lg in range(28):
            for n in ((1 << lg), (2 << lg) - 1):
                c = MB.window_bits(n, m)
                assert MB.MIN_BITS <= c <= MB.MAX_BITS, (n, m)
                assert c >= last, (n, m)  # non-decreasing in n for fixed m
                last = c
                assert lib.eccx_msm_batch_window_bits(n, m) == c, (n, m)
                if m == 1:
                    assert c == M.window_bits(n) == lib.eccx_msm_window_bits(n), n


def test_width_is_a_function_of_the_floors_of_the_logarithms(lib):
    for lg in (0, 5, 12, 16, 20):
        for lgm in (0, 1, 4, 8):
            cs = {lib.eccx_msm_batch_window_bits(n, m) for n in ((1 << lg), (2 << lg) - 1) for m in ((1 << lgm), (2 << lgm) - 1)}
            assert len(cs) == 1, (lg, lgm)


def _why(n, m):
    """which of the three limits refuses (n, m): a set of names, empty where it is accepted"""
    c = MB.window_bits(n, m)
    W, B = M.windows(c), 1 << (c - 1)
    out = set()
    if m * n > MB.MAX_UNITS:
        out.add("units")
    if W * m * n > MB.MAX_U32:
        out.add("list")
    if m * W * B > MB.MAX_U32:
        out.add("keys")
    return out


def test_limit_rule():
    cases = {
        (1 << 27, 1): set(),                 # what eccx_msm takes, one vector takes
        ((1 << 27) + 1, 1): {"units"},
        (1 << 14, 1 << 13): set(),           # m * n = 2^27 at a width whose list still fits
        (1 << 14, (1 << 13) + 1): {"units"},
        (128, 1 << 18): set(),
        (128, 1 << 19): {"list"},            # 4-bit windows: 65 slots per unit, 65 * 2^26 leaves 32 bits though m * n does not
        (1, 1 << 22): set(),
        (1, 1 << 23): {"keys"},              # one term per vector: 65 * 8 keys per vector against 65 slots
    }
    for (n, m), why in cases.items():
        assert _why(n, m) == why, (n, m)
        assert MB.fits(n, m) == (not why), (n, m)
    assert MB.MAX_UNITS == 1 << 27 and MB.MAX_U32 == (1 << 32) - (1 << 12)
