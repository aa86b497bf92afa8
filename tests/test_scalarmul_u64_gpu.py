"""eccx_scalarmul_u64 on bls12_381_g1 and bls12_381_g2 through the engine layer and libeccx.so: every digit of the signed
2-bit recoding and its top carry, points in and outside the subgroup, the flag and validation rules, the sizes around a wave
and a workgroup, byte for byte against the model (tests/bls_batch_ref.py) and against eccx_scalarmul_var on the
zero-padded scalar; the _dev form on a side stream, at odd addresses and in place; the argument checks."""
import ctypes

import numpy as np
import pytest

import eccoxide_amd as E
from eccoxide_amd import engine as EN
from tests import bls_batch_ref as BR
from tests import bls_sig_ref as B
from tests import g2_ref as G2
from tests import msm_ref as M

pytestmark = pytest.mark.gpu

ERR_ARG = -2
COEFFS = [0, 1, 2, 3, 15, 16, 17, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555]


@pytest.fixture(scope="module")
def eng():
    with E.Engine(0) as e:
        yield e


class Curve:
    def __init__(self, name):
        self.name = name
        self.group = B._G2 if name == "bls12_381_g2" else B._G1
        self.pb = 192 if name == "bls12_381_g2" else 96
        self.off = G2.point_of_x((1, 2)) if name == "bls12_381_g2" else M.point_off_subgroup()
        assert self.group.mul(B.R, self.off) is not None   # outside the subgroup

    def rec(self, p):
        return BR.record(self.group, p)

    def want(self, coeffs, points, inf=None):
        out = [self.rec(None if (inf and inf[i] == 1) else BR.scalarmul_u64(self.group, c, p)) for i, (c, p) in enumerate(zip(coeffs, points))]
        return b"".join(o[0] for o in out), bytes(o[1] for o in out)


@pytest.fixture(scope="module", params=["bls12_381_g1", "bls12_381_g2"])
def cv(request):
    return Curve(request.param)


def cbytes(coeffs):
    return b"".join(int(c).to_bytes(8, "big") for c in coeffs)


def random_points(eng, cv, n, seed):
    """n points of the subgroup from the library's fixed-base comb (pinned to the models by its own tests), as model points"""
    rng = np.random.default_rng(seed)
    ks = rng.bytes(32 * n)
    ks = b"".join((int.from_bytes(ks[32 * i:32 * i + 32], "big") % B.R or 1).to_bytes(32, "big") for i in range(n))
    recs, fl = eng.scalarmul_base(cv.name, ks)
    assert fl == bytes(n)
    return recs


def test_every_digit_and_the_top_carry(eng, cv):
    """the listed coefficients on the generator, on a point outside the subgroup and on a random point"""
    rnd = cv.group.mul(0x1234567890ABCDEF1122334455667788, cv.group.gen)
    for p in (cv.group.gen, cv.off, rnd):
        pts = cv.rec(p)[0] * len(COEFFS)
        assert eng.scalarmul_u64(cv.name, cbytes(COEFFS), pts) == cv.want(COEFFS, [p] * len(COEFFS))
    # the coefficient 0 is the identity: flag 1 over zero bytes
    got = eng.scalarmul_u64(cv.name, cbytes([0]), cv.rec(cv.group.gen)[0])
    assert got == (bytes(cv.pb), b"\1")


def test_against_scalarmul_var_on_the_padded_scalar(eng, cv):
    pts = cv.rec(cv.group.gen)[0] + cv.rec(cv.off)[0]
    pts = pts * len(COEFFS)
    cs = [c for c in COEFFS for _ in range(2)]
    padded = b"".join(int(c).to_bytes(32, "big") for c in cs)
    assert eng.scalarmul_u64(cv.name, cbytes(cs), pts) == eng.scalarmul_var(cv.name, padded, pts)


def test_flags_and_validation(eng, cv):
    g = cv.rec(cv.group.gen)[0]
    garbage = bytes((7 + 3 * i) % 256 for i in range(cv.pb))
    # an input flagged 1 over garbage bytes is the identity; an input flagged 2 stays rejected; both with and without validation
    for validate in (False, True):
        out, fl = eng.scalarmul_u64(cv.name, cbytes([5, 5, 5]), g + garbage + g, bytes([0, 1, 2]), validate=validate)
        assert fl == bytes([0, 1, 2])
        assert out == cv.rec(cv.group.mul(5, cv.group.gen))[0] + bytes(2 * cv.pb)
    # ECCX_VALIDATE_POINTS: a coordinate that is not below p, and a point off the curve
    p48 = G2.P.to_bytes(48, "big")
    big_x = p48 + g[48:]
    y = int.from_bytes(g[cv.pb - 48:], "big")
    off_curve = g[:cv.pb - 48] + ((y + 1) % G2.P).to_bytes(48, "big")
    out, fl = eng.scalarmul_u64(cv.name, cbytes([3, 3, 3]), big_x + off_curve + g, validate=True)
    assert fl == bytes([2, 2, 0]) and out == bytes(2 * cv.pb) + cv.rec(cv.group.mul(3, cv.group.gen))[0]
    # a point outside the subgroup is a legal input under validation too
    out, fl = eng.scalarmul_u64(cv.name, cbytes([(1 << 64) - 1]), cv.rec(cv.off)[0], validate=True)
    assert (out, fl) == cv.want([(1 << 64) - 1], [cv.off])
    # n = 0 and 1
    assert eng.scalarmul_u64(cv.name, b"", b"") == (b"", b"")
    assert eng.scalarmul_u64(cv.name, cbytes([17]), g) == cv.want([17], [cv.group.gen])


SIZES = [63, 64, 65, 257]


@pytest.fixture(scope="module")
def shared(eng, cv):
    """257 random points and coefficients with the model's products, computed once for the size cases"""
    n = max(SIZES)
    recs = random_points(eng, cv, n, 64 + cv.pb)
    rng = np.random.default_rng(9 + cv.pb)
    coeffs = [int.from_bytes(rng.bytes(8), "big") for _ in range(n)]
    from_rec = (lambda b: G2.from_record(b)) if cv.pb == 192 else (lambda b: (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big")))
    pts = [from_rec(recs[cv.pb * i:cv.pb * i + cv.pb]) for i in range(n)]
    return recs, coeffs, cv.want(coeffs, pts)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_a_wave_and_a_workgroup(eng, cv, shared, n):
    recs, coeffs, want = shared
    assert eng.scalarmul_u64(cv.name, cbytes(coeffs[:n]), recs[:cv.pb * n]) == (want[0][:cv.pb * n], want[1][:n])


def test_dev_form_side_stream_odd_addresses_in_place(eng, cv, shared):
    import torch

    recs, coeffs, want = shared
    n = 65
    d = lambda b, pad: torch.frombuffer(bytearray(bytes(pad) + b), dtype=torch.uint8).cuda()[pad:]
    dc, dp = d(cbytes(coeffs[:n]), 1), d(recs[:cv.pb * n], 3)
    inf = d(bytes(n), 5)
    out = torch.full((n * cv.pb + 7,), 0x5A, dtype=torch.uint8, device="cuda")[7:]
    fl = torch.full((n + 1,), 0x5A, dtype=torch.uint8, device="cuda")[1:]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.scalarmul_u64_t(cv.name, dc, dp, inf, out, fl, stream=side.cuda_stream)
    side.synchronize()
    assert out.cpu().numpy().tobytes() == want[0][:cv.pb * n] and fl.cpu().numpy().tobytes() == want[1][:n]
    # in place: out is points and the flags are the input flags
    eng.scalarmul_u64_t(cv.name, dc, dp, inf, dp, inf, stream=side.cuda_stream)
    side.synchronize()
    assert dp.cpu().numpy().tobytes() == want[0][:cv.pb * n] and inf.cpu().numpy().tobytes() == want[1][:n]


def test_argument_checks_write_nothing(eng, cv):
    import torch

    lib, ctx = eng._lib, eng._ctx
    err = lambda: lib.eccx_last_error(ctx).decode()
    cid = EN.CURVE_IDS[cv.name]
    g = cv.rec(cv.group.gen)[0]
    out, fl = ctypes.create_string_buffer(b"\x5a" * cv.pb, cv.pb), ctypes.create_string_buffer(b"\x5a", 1)
    for bad in (EN.CT_SCAN, EN.CT_SCAN | EN.VALIDATE_POINTS, EN.MIRROR_REFERENCE, EN.ASSUME_SUBGROUP, 1 << 31):
        assert lib.eccx_scalarmul_u64(ctx, cid, 1, cbytes([1]), g, None, out, fl, bad) == ERR_ARG and "opts" in err()
    for curve in (EN.P256R1, EN.ED25519, EN.JUBJUB, 6, 99):
        assert lib.eccx_scalarmul_u64(ctx, curve, 1, cbytes([1]), g, None, out, fl, 0) == ERR_ARG and "ECCX_BLS12_381_G1" in err()
    assert lib.eccx_scalarmul_u64(ctx, cid, 1, None, g, None, out, fl, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_scalarmul_u64(ctx, cid, 1, cbytes([1]), None, None, out, fl, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_scalarmul_u64(ctx, cid, 1, cbytes([1]), g, None, None, fl, 0) == ERR_ARG
    assert lib.eccx_scalarmul_u64(ctx, cid, 1, cbytes([1]), g, None, out, None, 0) == ERR_ARG
    assert out.raw == b"\x5a" * cv.pb and fl.raw == b"\x5a"
    # the _dev form refuses ECCX_CT_SCAN before anything is launched
    dout = torch.full((cv.pb,), 0x5A, dtype=torch.uint8, device="cuda")
    dfl = torch.full((1,), 0x5A, dtype=torch.uint8, device="cuda")
    dc = torch.frombuffer(bytearray(cbytes([1])), dtype=torch.uint8).cuda()
    dp = torch.frombuffer(bytearray(g), dtype=torch.uint8).cuda()
    assert lib.eccx_scalarmul_u64_dev(ctx, cid, 1, dc.data_ptr(), dp.data_ptr(), None, dout.data_ptr(), dfl.data_ptr(), EN.CT_SCAN, None) == ERR_ARG
    torch.cuda.synchronize()
    assert dout.cpu().numpy().tobytes() == b"\x5a" * cv.pb and dfl.cpu().numpy().tobytes() == b"\x5a"
    assert lib.eccx_scalarmul_u64(ctx, cid, 0, None, None, None, None, None, 0) == 0
