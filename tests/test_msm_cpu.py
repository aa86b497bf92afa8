"""The model of eccx_msm (tests/msm_ref.py) against itself: no GPU."""
import random

import pytest

from tests import msm_ref as M

R_ORDER = M.ORDER
WIDTHS = list(range(M.MIN_BITS, M.MAX_BITS + 1))


def test_direct_sum_and_shortcut_agree():
    rng = random.Random(1)
    rs = [rng.randrange(1, R_ORDER) for _ in range(6)]
    ks = [rng.randrange(1 << 256) for _ in range(6)]
    pts = [M.R.affine_mul(M.C, r, M.G) for r in rs]
    assert M.msm(ks, pts) == M.msm_of_multiples(ks, rs)
    # scalars that cancel: k (r G) + (r - k) (r G) ... = infinity
    assert M.msm_of_multiples([5, R_ORDER - 5], [7, 7]) is None
    assert M.msm([5, R_ORDER - 5], [pts[0], pts[0]]) is None


def test_point_off_subgroup_is_on_the_curve_and_outside_g1():
    P = M.point_off_subgroup()
    assert M.R.on_curve(M.C, P)
    assert M.R.affine_mul(M.C, R_ORDER, P) is not None
    assert M.R.affine_mul(M.C, R_ORDER, M.G) is None


def _alternating(c, first_high):
    """Windows alternately 100..0 and 011..1 (first_high: window 0 is 100..0), cut to 256 bits.  A window 100..0 above a
    window whose top bit is clear recodes to -2^(c-1); a window 011..1 above one whose top bit is set to +2^(c-1)."""
    half = 1 << (c - 1)
    return sum((half if (i % 2 == 0) == first_high else half - 1) << (c * i) for i in range(M.windows(c))) % (1 << 256)


def _patterns(c):
    top = 1 << 256
    return [0, 1, 2, top - 1, R_ORDER - 1, R_ORDER, R_ORDER + 1, _alternating(c, True), _alternating(c, False), (top - 1) // 3, top >> 1]


@pytest.mark.parametrize("c", WIDTHS)
def test_recoding_reconstructs_the_scalar(c):
    rng = random.Random(c)
    half = 1 << (c - 1)
    for k in _patterns(c) + [rng.randrange(1 << 256) for _ in range(50)]:
        ds = M.recode(k, c)
        assert len(ds) == M.windows(c) == -(-257 // c)
        assert all(-half <= d <= half for d in ds)
        assert sum(d << (c * w) for w, d in enumerate(ds)) == k


@pytest.mark.parametrize("c", WIDTHS)
def test_extreme_digits_in_every_window(c):
    half, w = 1 << (c - 1), M.windows(c)
    full = 256 // c  # windows that lie wholly inside the scalar's 256 bits
    a, b = M.recode(_alternating(c, True), c), M.recode(_alternating(c, False), c)
    # between them the two patterns put -2^(c-1) into every full window and +2^(c-1) into every full window but the
    # lowest, which has no borrow below it and so never exceeds 2^(c-1) - 1
    for i in range(full):
        assert {a[i], b[i]} == ({-half, half} if i else {-half, half - 1})
    ds = M.recode((1 << 256) - 1, c)  # all ones: -1 at the bottom, zeros between, the carry alone on top
    assert ds[0] == -1 and all(d == 0 for d in ds[1:-1]) and ds[-1] == 1 << (256 - c * (w - 1))


def test_width_function():
    prev = 0
    ns = sorted(set(list(range(1, 5000)) + [1 << e for e in range(12, 28)] + [(1 << e) - 1 for e in range(12, 28)]))
    for n in ns:
        c = M.window_bits(n)
        assert M.MIN_BITS <= c <= M.MAX_BITS and c >= prev
        prev = c
    assert M.window_bits(1) == 4 and M.window_bits(1 << 20) == 16 and M.window_bits((1 << 13) - 1) == 4 and M.window_bits(1 << 13) == 5
    assert [M.window_bits(1 << e) for e in (12, 16, 18, 20, 22)] == [4, 11, 15, 16, 16]  # the sizes the sweep measured
    assert sorted({M.window_bits(n) for n in ns}) == M.widths_returned() and set(M.widths_returned()) <= set(WIDTHS)


def test_width_function_of_the_library_is_the_models():
    """eccx_msm_window_bits is host code: it runs without a GPU."""
    from eccoxide_amd import _lib

    lib = _lib.load()
    for n in [0, 1, 2, 255, 256, 257, 4099, (1 << 19) - 1, 1 << 19, 1 << 20, 1 << 27] + [1 << e for e in range(4, 20)] + [(1 << e) - 1 for e in range(4, 20)]:
        assert lib.eccx_msm_window_bits(n) == M.window_bits(n), n
