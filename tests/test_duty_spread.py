"""The public a = -3 ladders (kernels_coz.hpp, CT = false) at the shapes where the shared table inversion's duty wave
and the ladder's nested loops (windows around doublings, the equal-points fix-up behind the addition) could go wrong:
batches that leave whole waves without a unit of their own, one degenerate unit in an inversion column on each side
of the duty wave, and more grid-stride iterations than the duty rotation has slots.  Every result is compared with
the oracle byte for byte, as tests/test_gpu_parity.py does."""
import numpy as np
import pytest

from eccoxide_amd import workload as W
from oracle import ecc_ref as R
from tests.test_coz_shared_inverse_gpu import SHAPES, SHAPE_IDS, bases, compare, expected, run, take

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 191, 256, 257, 1000)
WORKGROUPS_PER_CU = 4  # the P-256 ladder's persistent grid (coz_occupancy)


@pytest.mark.parametrize("curve,fused", SHAPES, ids=SHAPE_IDS)
def test_small_and_ragged_batches(engine, oracle, curve, fused):
    """one wave only; workgroups with whole waves that run the clamped unit; a ragged last workgroup: every unit"""
    C = R.CURVES[curve]
    nmax = max(SIZES)
    ks = W.random_scalars(curve, nmax, seed=5201).tobytes()
    u1 = W.random_scalars(curve, nmax, seed=5202).tobytes()
    pts = bases(oracle, curve, nmax, shift=5)
    want = expected(oracle, curve, fused, ks, pts, u1)
    for n in SIZES:
        got = run(engine, oracle, curve, fused, ks[:n * C.sb], pts[:n * 2 * C.fb], u1[:n * C.sb])
        assert len(got[1]) == n
        compare(got, want, 2 * C.fb, range(n))


@pytest.mark.parametrize("wave", [1, 0, 3])
@pytest.mark.parametrize("curve,fused", SHAPES, ids=SHAPE_IDS)
def test_one_bad_unit_in_a_column(engine, oracle, curve, fused, wave):
    """One workgroup; the unit at lane 64 wave + 6 has a base with y = 0: its table build degenerates at the first
    doubling and it enters the column's shared product as 1.  The other three members of column 6 (and every other
    unit) are the oracle's.  The bad unit is redone by the generic ladder behind, which sees nothing but the unit's own
    bytes, so its flag and bytes are those of a batch that holds it alone, and the flag is the one the parent commit
    returns."""
    C = R.CURVES[curve]
    fb, pb, n = C.fb, 2 * C.fb, 256
    bad = 64 * wave + 6
    column = [64 * w + 6 for w in range(4) if w != wave]
    pts = bytearray(bases(oracle, curve, n, shift=11))
    good = bytes(pts)
    pts[bad * pb + fb:(bad + 1) * pb] = bytes(fb)  # (x, 0)
    pts = bytes(pts)
    ks = W.random_scalars(curve, n, seed=5203).tobytes()
    u1 = W.random_scalars(curve, n, seed=5204).tobytes()
    want = expected(oracle, curve, fused, ks, good, u1)
    got = run(engine, oracle, curve, fused, ks, pts, u1)
    compare(got, want, pb, column)
    compare(got, want, pb, [i for i in range(n) if i != bad])
    alone = run(engine, oracle, curve, fused, take(ks, C.sb, [bad]), take(pts, pb, [bad]), take(u1, C.sb, [bad]))
    compare(got, alone, pb, [bad], [0])
    assert got[1][bad] == 1  # recorded from the parent commit's build: all twelve cases, the point at infinity


def test_more_iterations_than_duty_slots(engine, oracle):
    """5 * 4 * CUs * 256 + 77 units: every workgroup of the persistent grid runs five or six iterations, so the duty
    rotation wraps.  A seeded sample of 512 units, the first and the last 64 among them, against the oracle."""
    import torch

    curve = "p256r1"
    C = R.CURVES[curve]
    pb = 2 * C.fb
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 5 * WORKGROUPS_PER_CU * cus * 256 + 77
    ks = W.random_scalars(curve, n, seed=5205).tobytes()
    pts = bases(oracle, curve, n, shift=2)
    ends = list(range(64)) + list(range(n - 64, n))
    middle = np.random.Generator(np.random.PCG64(5206)).choice(np.arange(64, n - 64), size=512 - len(ends), replace=False)
    idxs = sorted(ends + [int(i) for i in middle])
    assert len(idxs) == 512
    want = expected(oracle, curve, False, take(ks, C.sb, idxs), take(pts, pb, idxs))
    got = run(engine, oracle, curve, False, ks, pts)
    assert len(got[1]) == n
    compare(got, want, pb, idxs, range(len(idxs)))
