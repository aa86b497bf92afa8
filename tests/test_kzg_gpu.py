"""KZG commitments through the C ABI and the Engine against expectations taken IN THE EXPONENT: under the insecure setup of
a known tau (tests/kzg_ref.py), C = [p(tau)]G1 and pi = [(p(tau) - y) / (tau - z)]G1 cost one model multiplication each and
owe nothing to the code under test.  The setup's Lagrange points are put on the device by the fixed-base entry point."""
import ctypes
import random

import pytest

from tests import g2_ref as G2
from tests import kzg_ref as K
from tests import msm_ref as MS

pytestmark = pytest.mark.gpu

Q = K.Q
TAU = 0x1234_5678_9ABC_DEF0_0FED_CBA9_8765_4321_1357_9BDF
ERR_ARG = -2


@pytest.fixture(scope="module")
def eng():
    import eccoxide_amd as E

    with E.Engine(0) as e:
        yield e


_SETUPS = {}


def setup_of(eng, N, bit_reversed=True, tau=TAU):
    """(model setup, the domain's bytes, the Lagrange points on the device's word, [tau]G2's record), once per shape"""
    key = (N, bit_reversed, tau)
    if key not in _SETUPS:
        s = K.Setup(tau, K.domain(N, bit_reversed))
        srs, fl = eng.scalarmul_base("bls12_381_g1", s.lagrange_scalars())
        assert fl == bytes(N)
        _SETUPS[key] = (s, K.fr_bytes(s.dom), srs, s.tau_g2_record())
    return _SETUPS[key]


def t(b):
    import torch

    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def raw(x):
    return bytes(x.cpu().numpy().reshape(-1))


def cases(N, dom, seed):
    """Four polynomials with their points: z outside the domain, z inside it, a constant (its proof is the point at
    infinity), and one with an element of r, refused beside the others."""
    rng = random.Random(f"kzg gpu {N} {seed}")
    polys = [[rng.randrange(Q) for _ in range(N)] for _ in range(2)] + [[Q - 3] * N]
    bad = list(polys[0])
    bad[N // 2] = Q
    polys.insert(1, bad)
    zs = [rng.randrange(Q), 17, dom[N - 1], rng.randrange(Q)]
    return polys, zs


def expected(setup, polys, zs):
    ys, proofs, commits, flags = [], [], [], []
    for poly, z in zip(polys, zs):
        if any(p >= Q for p in poly) or z >= Q:
            ys.append(bytes(32)); proofs.append(bytes(48)); commits.append(bytes(48)); flags.append(2)
            continue
        y, pi = setup.open(poly, z)
        ys.append(y.to_bytes(32, "big")); proofs.append(K.compress(pi)); commits.append(K.compress(setup.commit(poly))); flags.append(0)
    return b"".join(ys), b"".join(proofs), b"".join(commits), bytes(flags)


@pytest.mark.parametrize("N", (1, 64, 512))
def test_commit_open_eval(eng, N):
    setup, dom_b, srs, _ = setup_of(eng, N)
    polys, zs = cases(N, setup.dom, 1)
    pb, zb = K.fr_bytes([p for poly in polys for p in poly]), K.fr_bytes(zs)
    want_y, want_pi, want_c, want_fl = expected(setup, polys, zs)
    assert want_pi[3 * 48:] == K.INFINITY_ENC and want_fl == bytes([0, 2, 0, 0])  # the constant's proof; the refused one
    assert eng.kzg_commit(pb, srs) == (want_c, want_fl)
    assert eng.kzg_open(pb, zb, dom_b, srs) == (want_y, want_pi, want_fl)
    assert eng.kzg_eval(pb, zb, dom_b) == (want_y, want_fl)
    # the device-tensor forms: the same bytes
    d_p, d_z, d_d, d_s = t(pb), t(zb), t(dom_b), t(srs)
    assert tuple(map(raw, eng.kzg_commit_t(d_p, d_s))) == (want_c, want_fl)
    assert tuple(map(raw, eng.kzg_open_t(d_p, d_z, d_d, d_s))) == (want_y, want_pi, want_fl)
    assert tuple(map(raw, eng.kzg_eval_t(d_p, d_z, d_d))) == (want_y, want_fl)


def test_zero_polynomial_commits_to_infinity(eng):
    setup, dom_b, srs, _ = setup_of(eng, 64)
    assert eng.kzg_commit(bytes(64 * 32), srs) == (K.INFINITY_ENC, b"\0")
    assert eng.kzg_open(bytes(64 * 32), K.fr_bytes([5]), dom_b, srs) == (bytes(32), K.INFINITY_ENC, b"\0")


def test_eip4844_shape(eng):
    N = 4096
    setup, dom_b, srs, tau_rec = setup_of(eng, N)
    rng = random.Random("kzg blob")
    polys = [[rng.randrange(Q) for _ in range(N)] for _ in range(2)]
    zs = [rng.randrange(Q), setup.dom[1234]]
    pb, zb = K.fr_bytes([p for poly in polys for p in poly]), K.fr_bytes(zs)
    want_y, want_pi, want_c, want_fl = expected(setup, polys, zs)
    got_c = eng.kzg_commit(pb, srs)
    got = eng.kzg_open(pb, zb, dom_b, srs)
    assert got_c == (want_c, want_fl)
    assert got == (want_y, want_pi, want_fl)
    assert eng.kzg_verify(got_c[0], zb, got[0], got[1], tau_rec) == bytes([K.SIG_VALID] * 2)


def test_verify_verdicts(eng):
    N = 64
    setup, dom_b, srs, tau_rec = setup_of(eng, N)
    rng = random.Random("kzg verify")
    p1, p2 = ([rng.randrange(Q) for _ in range(N)] for _ in range(2))
    const, zero = [Q - 9] * N, [0] * N
    c1, c2, cc, cz = (K.compress(setup.commit(p)) for p in (p1, p2, const, zero))
    assert cz == K.INFINITY_ENC
    z1, z2 = rng.randrange(Q), setup.dom[37]

    def opening(poly, z):
        y, pi = setup.open(poly, z)
        return y.to_bytes(32, "big"), K.compress(pi)

    def fr(v):
        return v.to_bytes(32, "big")

    y11, pi11 = opening(p1, z1)
    y12, pi12 = opening(p1, z2)
    y21, pi21 = opening(p2, z1)
    y10, pi10 = opening(p1, 0)
    yc, pic = opening(const, z1)
    assert pic == K.INFINITY_ENC and y12 == fr(p1[37])
    off = K.compress(MS.point_off_subgroup())
    V, I, M = K.SIG_VALID, K.SIG_INVALID, K.SIG_MALFORMED
    units = [  # commitment, z, y, proof, verdict
        (c1, fr(z1), y11, pi11, V),
        (c1, fr(z2), y12, pi12, V),                              # z in the domain
        (cc, fr(z1), yc, K.INFINITY_ENC, V),                     # a constant: the proof is the identity
        (cz, fr(z1), bytes(32), K.INFINITY_ENC, V),              # the zero polynomial: the commitment is the identity too
        (c2, fr(z1), y21, pi21, V),
        (c1, fr(z1), fr((int.from_bytes(y11, "big") + 1) % Q), pi11, I),   # a wrong y
        (c1, fr((z1 + 1) % Q), y11, pi11, I),                    # a wrong z
        (c1, fr(z1), y11, pi21, I),                              # a proof for another polynomial
        (pi11, fr(z1), y11, c1, I),                              # commitment and proof swapped
        (c1, fr(z1), fr(Q), pi11, M),                            # y = r
        (c1, fr(Q), y11, pi11, M),                               # z = r
        (off, fr(z1), y11, pi11, M),                             # a commitment outside G1
        (c1, fr(z1), y11, bytes(48), M),                         # proof bytes that do not decode
        (c1, fr(0), y10, pi10, V),                               # z = 0
        (cz, fr(z1), fr(1), K.INFINITY_ENC, I),                  # the identity does not open to 1
        (cc, fr(z2), yc, K.INFINITY_ENC, V),                     # the constant at a domain element
    ]
    assert len(units) == 16
    cs, zs, ys, ps = (b"".join(u[i] for u in units) for i in range(4))
    want = bytes(u[4] for u in units)
    assert eng.kzg_verify(cs, zs, ys, ps, tau_rec) == want
    assert raw(eng.kzg_verify_t(t(cs), t(zs), t(ys), t(ps), tau_rec)) == want
    # [tau]G2 may come in its 96-byte encoding; a point outside G2 is refused by the Engine
    assert eng.kzg_verify(cs, zs, ys, ps, G2.compress(setup.tau_g2)) == want
    with pytest.raises(ValueError):
        eng.kzg_verify(cs, zs, ys, ps, G2.to_record(G2.point_of_x((1, 2)))[0])
    # a good opening under another tau
    other = G2.to_record(G2.mul(TAU + 1, G2.G))[0]
    assert eng.kzg_verify(c1, fr(z1), y11, pi11, other) == bytes([I])
    assert eng.kzg_verify(c1, fr(z1), y11, pi11, tau_rec) == bytes([V])


def test_refusals_and_empty_calls(eng):
    lib, ctx = eng._lib, eng._ctx
    b = ctypes.create_string_buffer(64 * 96)
    for N, m in ((3, 1), (0, 1), (1 << 21, 1), (1 << 20, (1 << 7) + 1)):
        assert lib.eccx_kzg_eval(ctx, N, m, b, b, b, b, b, 0) == ERR_ARG
        assert lib.eccx_kzg_commit(ctx, N, m, b, b, b, b, 0) == ERR_ARG
        assert lib.eccx_kzg_open(ctx, N, m, b, b, b, b, b, b, b, 0) == ERR_ARG
        assert lib.eccx_kzg_reserve(ctx, N, m) == ERR_ARG
    assert lib.eccx_kzg_open(ctx, 8, 1, b, b, b, b, b, b, b, 4) == ERR_ARG
    assert lib.eccx_kzg_verify(ctx, 1, b, b, b, b, b, b, 1) == ERR_ARG
    assert lib.eccx_kzg_open(ctx, 8, 1, b, b, None, b, b, b, b, 0) == ERR_ARG
    assert lib.eccx_kzg_verify(ctx, 1, b, b, b, b, None, b, 0) == ERR_ARG
    # nothing to do is no error, whatever N is
    for N in (0, 3, 64):
        assert lib.eccx_kzg_eval(ctx, N, 0, None, None, None, None, None, 0) == 0
        assert lib.eccx_kzg_commit(ctx, N, 0, None, None, None, None, 0) == 0
        assert lib.eccx_kzg_open(ctx, N, 0, None, None, None, None, None, None, None, 0) == 0
    assert lib.eccx_kzg_verify(ctx, 0, None, None, None, None, None, None, 0) == 0
    assert lib.eccx_kzg_reserve(ctx, 64, 0) == 0
