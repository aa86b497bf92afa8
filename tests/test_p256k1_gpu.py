"""secp256k1 (p256k1) on the GPU against the Python reference (tests/p256k1_ref.py): the default variable base (the
endomorphism ladder), the reference-mirroring kernels, fixed base, the secret-scalar kernels, the group law, the verify
shape (ECDSA), the SEC1 codecs and the host-buffer path."""
import hashlib
import random

import numpy as np
import pytest

from eccoxide_amd import workload as W
from tests import p256k1_ref as K
from tests.oracle_lib import golden

pytestmark = pytest.mark.gpu
C = "p256k1"
N = K.N


def kb(k: int) -> bytes:
    return (k % (1 << 256)).to_bytes(32, "big")


def rand_points(rng, count):
    return [K.mul(rng.randrange(1, N)) for _ in range(count)]


def check_var(got, ks, pts, label=""):
    out, flags = got
    for i, (k, Pt) in enumerate(zip(ks, pts)):
        want, wf = K.affine_bytes(K.mul(k, Pt))
        assert flags[i] == wf and out[64 * i: 64 * i + 64] == want, f"{label} unit {i}: k = {k:#x}"


def run_var(engine, ks, pts, **kw):
    return engine.scalarmul_var(C, b"".join(kb(k) for k in ks), b"".join(K.point_bytes(P) for P in pts), **kw)


@pytest.mark.parametrize("n", [1, 63, 257, 1500])
def test_var_default_matches_reference(engine, n):
    rng = random.Random(1000 + n)
    ks = [rng.getrandbits(256) for _ in range(n)]
    pts = rand_points(rng, n)
    check_var(run_var(engine, ks, pts), ks, pts, "glv")


def test_var_mirror_proj_matches_reference_ladder(engine):
    rng = random.Random(5)
    ks = [rng.getrandbits(256) for _ in range(40)] + [0, 1, N - 1, N]
    pts = rand_points(rng, len(ks))
    out, flags, proj = run_var(engine, ks, pts, want_proj=True)
    check_var((out, flags), ks, pts, "mirror")
    for i, (k, Pt) in enumerate(zip(ks, pts)):
        X, Y, Z = K.ladder_proj(kb(k), Pt)
        p = K.P
        want = b"".join((v % p).to_bytes(32, "big") for v in (X, Y, Z))
        assert proj[96 * i: 96 * i + 96] == want, f"unit {i}: un-normalised residues differ from the reference's"


def _edge_scalars():
    n, lam = N, K.LAMBDA
    ks = [0, 1, 2, n - 1, n, n + 1, 2**256 - 1, lam, n - lam, n - 2, 2**255, 2**128, 2**128 - 1]
    ks += [c * lam % n for c in (1, 2, 3, 17, 2**64 + 1)]                  # k1 = 0
    ks += [5, 2**100 + 7, 2**127 - 1]                                        # k2 = 0
    for k1 in (2**127 - 1, -(2**127), 2**128 - 1, -(2**128 - 1), 1, -1):     # halves near +-2^128 and +-1
        for k2 in (2**127 - 1, -(2**127 - 1), 2**128 - 1, -(2**128 - 1), 1, -1, 0):
            ks.append((k1 + k2 * lam) % n)
    for a, b in ((K.A1, K.B1), (K.A2, K.B2)):
        ks += [a % n, (b * lam) % n, (-a) % n, (a + b * lam) % n, (2 * (a + b * lam)) % n]
    return ks


def test_edge_scalars_and_bases(engine):
    ks = _edge_scalars()
    splits = [K.glv_split_lattice(k % (1 << 256)) for k in ks]
    assert any(k1 == 0 for k1, _ in splits) and any(k2 == 0 for _, k2 in splits)
    assert max(max(abs(a), abs(b)) for a, b in splits).bit_length() == 128
    rng = random.Random(9)
    bases = [K.G, K.neg(K.G), K.sigma(K.G), K.sigma(K.sigma(K.G))] + rand_points(rng, 3)
    all_k, all_p = [], []
    for Pt in bases:
        all_k += ks
        all_p += [Pt] * len(ks)
    check_var(run_var(engine, all_k, all_p), all_k, all_p, "edge")
    check_var(run_var(engine, all_k, all_p, mirror=True), all_k, all_p, "edge mirror")


def test_sampled_full_batch(engine):
    import torch

    n = 1 << 20
    ks_b = W.random_scalars(C, n, seed=11)
    pts, pf = engine.scalarmul_base_t(C, torch.from_numpy(ks_b).cuda())
    ks_v = W.random_scalars(C, n, seed=12)
    ks_v[::4096] = 0xFF  # a few scalars above n (used as given)
    out, flags = engine.scalarmul_var_t(C, torch.from_numpy(ks_v).cuda(), pts)
    out, flags, pts_h, pf = out.cpu().numpy(), flags.cpu().numpy(), pts.cpu().numpy(), pf.cpu().numpy()
    assert not pf.any() and not flags.any()
    rng = random.Random(13)
    for i in sorted(rng.sample(range(n), 96)) + [0, 4096, n - 1]:
        Pb = K.mul_bytes(ks_b[i].tobytes())
        assert pts_h[i].tobytes() == K.point_bytes(Pb), f"base unit {i}"
        assert out[i].tobytes() == K.point_bytes(K.mul_bytes(ks_v[i].tobytes(), Pb)), f"var unit {i}"


def test_mul_base_and_comb_table(engine):
    rng = random.Random(21)
    ks = [rng.getrandbits(256) for _ in range(300)] + [0, 1, 2, N - 1, N, N + 1, 2**256 - 1, K.LAMBDA]
    got = engine.scalarmul_base(C, b"".join(kb(k) for k in ks))
    check_var(got, ks, [K.G] * len(ks), "mul_base")
    assert run_var(engine, ks, [K.G] * len(ks)) == got  # var on G agrees
    tab = engine.comb_table(C)
    assert hashlib.sha256(tab).hexdigest() == golden("p256k1.json")["comb"]["sha256_xy_concat"]


def test_sage_vectors_both_paths(engine):
    kats = golden("p256k1.json")["sage_kg"]
    ks = b"".join(kb(kv["k"]) for kv in kats)
    want = b"".join(bytes.fromhex(kv["x"]) + bytes.fromhex(kv["y"]) for kv in kats)
    out, flags = engine.scalarmul_base(C, ks)
    assert out == want and not any(flags)
    out, flags = engine.scalarmul_var(C, ks, K.point_bytes(K.G) * len(kats))
    assert out == want and not any(flags)


def test_validate_points(engine):
    rng = random.Random(31)
    good = rand_points(rng, 6)
    off = (good[0][0], (good[0][1] + 1) % K.P)
    big_x = (good[1][0] + K.P, good[1][1])  # x >= p (only representable when x < 2^256 - p)
    if big_x[0] >= 1 << 256:
        big_x = (K.P, good[1][1])
    recs = [K.point_bytes(good[2]), off[0].to_bytes(32, "big") + off[1].to_bytes(32, "big"),
            big_x[0].to_bytes(32, "big") + big_x[1].to_bytes(32, "big"), K.point_bytes(good[3])]
    ks = [rng.getrandbits(256) for _ in recs]
    out, flags = engine.scalarmul_var(C, b"".join(kb(k) for k in ks), b"".join(recs), validate=True)
    assert list(flags) == [0, 2, 2, 0]
    assert out[64:192] == bytes(128)
    assert out[:64] == K.point_bytes(K.mul(ks[0], good[2])) and out[192:] == K.point_bytes(K.mul(ks[3], good[3]))


def test_point_add(engine):
    rng = random.Random(41)
    Pa = rand_points(rng, 3)
    a = b"".join(K.point_bytes(P) for P in (Pa[0], Pa[1], Pa[2], Pa[0]))
    b = b"".join(K.point_bytes(P) for P in (Pa[0], K.neg(Pa[1]), Pa[2], Pa[1]))
    b_inf = bytes([0, 0, 1, 0])
    for mirror in (False, True):
        out, flags = engine.point_add(C, a, b, b_inf=b_inf, mirror=mirror)
        want = [K.mul(2, Pa[0]), None, Pa[2], R_add(Pa[0], Pa[1])]
        for i, Wp in enumerate(want):
            wb, wf = K.affine_bytes(Wp)
            assert flags[i] == wf and out[64 * i: 64 * i + 64] == wb, (mirror, i)


def R_add(P1, P2):
    from oracle import ecc_ref as R

    return R.affine_add(K.K1, P1, P2)


def test_ecdsa_verify_shape(engine):
    """ECDSA verification (src/protocol/ecdsa.rs): R = u1 G + u2 Q with u1 = e / s, u2 = r / s; valid iff R.x = r mod n."""
    rng = random.Random(51)
    n = 64
    e_l, r_l, s_l, q_l, valid = [], [], [], [], []
    for i in range(n):
        d = rng.randrange(1, N)
        Q = K.mul(d)
        e = int.from_bytes(hashlib.sha256(b"msg %d" % i).digest(), "big")
        while True:
            k = rng.randrange(1, N)
            r = K.mul(k)[0] % N
            s = pow(k, -1, N) * (e + r * d) % N
            if r and s:
                break
        ok = i % 4 != 3
        if not ok:  # tampered: another message, or r / s changed
            e = (e + 1) if i % 8 == 3 else e
            s = s if i % 8 == 3 else (s + 1) % N or 1
        e_l.append(e), r_l.append(r), s_l.append(s), q_l.append(Q), valid.append(ok)
    u1 = [e * pow(s, -1, N) % N for e, s in zip(e_l, s_l)]
    u2 = [r * pow(s, -1, N) % N for r, s in zip(r_l, s_l)]
    out, flags = engine.double_scalarmul(C, b"".join(map(kb, u1)), b"".join(map(kb, u2)),
                                         b"".join(K.point_bytes(Q) for Q in q_l), x_only=True)
    for i in range(n):
        x = int.from_bytes(out[32 * i: 32 * i + 32], "big")
        assert (flags[i] == 0 and x % N == r_l[i]) == valid[i], i
    full, _ = engine.double_scalarmul(C, b"".join(map(kb, u1)), b"".join(map(kb, u2)), b"".join(K.point_bytes(Q) for Q in q_l))
    for i in range(n):
        want = R_add(K.mul(u1[i]), K.mul(u2[i], q_l[i]))
        assert full[64 * i: 64 * i + 64] == K.affine_bytes(want)[0]


def test_fused_accumulation_special_cases(engine):
    """tests/test_double_scalarmul.py's test of the same name, for the curve the C oracle does not have: (u1, u2) that make
    the comb of u1 G and the ladder's u2 Q collide (accumulator == table entry: the doubling branch; == its negative:
    infinity) or leave a half at infinity, with Q = G, -G, sigma(G), sigma^2(G) (Q = q G for q = 1, n - 1, lambda,
    lambda^2), both signs, plain and with the options ECDSA verification passes (x only, keys validated)."""
    from tests import ecdsa_ref as E

    rng = random.Random(99)
    pairs = []
    for w, d in ((0, 1), (0, 200), (1, 7), (5, 255), (30, 3)):
        k = d << (8 * w)
        pairs += [(k, k), (N - k, k), (k, N - k)]
    pairs += [(0, 0), (0, N), (N, 0), (5, 0), (0, 5), (N - 1, 1), (1, N - 1)]
    for _ in range(8):
        k = rng.randrange(1, N)
        pairs += [(N - k, k), (k, k)]
    lam = K.LAMBDA
    bases = [(1, K.G), (N - 1, K.neg(K.G)), (lam, K.sigma(K.G)), (lam * lam % N, K.sigma(K.sigma(K.G)))]
    for q, Q in bases:
        assert E.mul(K.K1, q) == Q
        # the same collisions where Q is not G: u2 Q = +-k G
        qi = pow(q, -1, N)
        extra = []
        for w, d in ((0, 1), (0, 200), (1, 7), (2, 65535), (5, 255), (30, 3)):
            k = d << (8 * w)
            extra += [(k, k * qi % N), (N - k, k * qi % N), (k, (N - k) * qi % N), (0, k * qi % N)]
        these = pairs + extra
        n = len(these)
        u1 = b"".join(kb(a) for a, _ in these)
        u2 = b"".join(kb(b) for _, b in these)
        qs = K.point_bytes(Q) * n
        for subtract in (False, True):
            out, flags = engine.double_scalarmul(C, u1, u2, qs, subtract=subtract)
            for i, (a, b) in enumerate(these):
                B = E.mul(K.K1, b, Q)
                want, wf = K.affine_bytes(R_add(E.mul(K.K1, a), K.neg(B) if subtract else B))
                assert flags[i] == wf and out[64 * i: 64 * i + 64] == want, (hex(q), subtract, i, hex(a), hex(b))
            assert any(f == 1 for f in flags) and any(f == 0 for f in flags)
            xs, flx = engine.double_scalarmul(C, u1, u2, qs, subtract=subtract, x_only=True, validate=True)
            assert flx == flags and xs == b"".join(out[64 * i: 64 * i + 32] for i in range(n)), (hex(q), subtract, "x_only")


def test_sec1_codec(engine):
    rng = random.Random(61)
    pts = rand_points(rng, 200) + [K.G, K.neg(K.G)]
    xy = b"".join(K.point_bytes(P) for P in pts) + bytes(64)
    inf = bytes(len(pts)) + b"\x01"
    assert engine.compressed_bytes(C) == 33
    enc = engine.point_compress(C, xy, inf)
    assert enc == b"".join(K.compress(P) for P in pts) + bytes(33)
    back, flags = engine.point_decompress(C, enc)
    assert back == xy and list(flags) == [0] * len(pts) + [1]
    # an x with no point (x^3 + 7 a non-residue), and x >= p
    x = next(x for x in range(1, 100) if K.decompress(bytes([2]) + x.to_bytes(32, "big")) is None)
    bad = bytes([2]) + x.to_bytes(32, "big") + bytes([3]) + K.P.to_bytes(32, "big")
    _, flags = engine.point_decompress(C, bad)
    assert list(flags) == [2, 2]


def test_secret_scalar_kernels_agree(engine):
    rng = random.Random(71)
    ks = [rng.getrandbits(256) for _ in range(400)] + [0, 1, N - 1, N, 2**256 - 1, K.LAMBDA]
    pts = rand_points(rng, len(ks))
    want_v = run_var(engine, ks, pts)
    check_var(want_v, ks, pts, "default")
    assert run_var(engine, ks, pts, ct_scan=True) == want_v
    kbytes = b"".join(kb(k) for k in ks)
    want_b = engine.scalarmul_base(C, kbytes)
    assert engine.scalarmul_base(C, kbytes, ct_scan=True) == want_b
    assert engine.scalarmul_base(C, kbytes, ct_gather=True) == want_b
    # ECCX_ASSUME_SUBGROUP changes nothing on a prime-order curve
    assert run_var(engine, ks, pts, assume_subgroup=True) == want_v


def test_host_buffer_path_in_chunks(engine):
    """The host-buffer entry points pipeline large batches in chunks; a batch spanning several chunks."""
    rng = random.Random(81)
    n = 300_000
    ks = W.random_scalars(C, n, seed=82)
    pts_b, _ = engine.scalarmul_base(C, ks.tobytes())
    out, flags = engine.scalarmul_var(C, W.random_scalars(C, n, seed=83).tobytes(), pts_b)
    ks2 = W.random_scalars(C, n, seed=83)
    assert not any(flags)
    for i in sorted(rng.sample(range(n), 24)) + [n - 1]:
        Pb = K.mul_bytes(ks[i].tobytes())
        assert pts_b[64 * i: 64 * i + 64] == K.point_bytes(Pb)
        assert out[64 * i: 64 * i + 64] == K.point_bytes(K.mul_bytes(ks2[i].tobytes(), Pb))
