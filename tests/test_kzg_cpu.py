"""The model of the KZG entry points (tests/kzg_ref.py) against direct Lagrange interpolation and the opening identity
p(tau) - y = q(tau) (tau - z), in both domain orders; one full verification of a good and of a bad opening through the
pairing model; and the refusals of the host entry points that need no GPU.  On the code before eccx_kzg_* the symbols are
missing and the library does not bind."""
import ctypes
import random

import pytest

from tests import kzg_ref as K

Q = K.Q
SIZES = (1, 2, 8, 64)
TAU = 0x5EED_0F_7A0 * 0x1_0000_0001 + 12345


def _poly(N, seed):
    rng = random.Random(f"kzg cpu {N} {seed}")
    return [rng.randrange(Q) for _ in range(N)]


@pytest.mark.parametrize("bit_reversed", (False, True))
@pytest.mark.parametrize("N", SIZES)
def test_domain(N, bit_reversed):
    dom = K.domain(N, bit_reversed)
    assert len(set(dom)) == N and all(pow(w, N, Q) == 1 for w in dom) and dom[0] == 1
    if N > 1:
        assert dom[1] == (Q - 1 if bit_reversed else pow(K.ROOT, (Q - 1) // N, Q))
    from eccoxide_amd.engine import Engine

    assert Engine.kzg_domain(N, bit_reversed) == K.fr_bytes(dom)


@pytest.mark.parametrize("bit_reversed", (False, True))
@pytest.mark.parametrize("N", SIZES)
def test_evaluate_is_lagrange_interpolation(N, bit_reversed):
    dom = K.domain(N, bit_reversed)
    poly = _poly(N, 1)
    rng = random.Random(f"kzg z {N}")
    for z in list(dom) + [0, rng.randrange(Q), Q - 1]:
        want = K.interpolate_direct(poly, dom, z)
        assert K.evaluate(poly, dom, z) == want, (N, z)
    for i, w in enumerate(dom):
        assert K.evaluate(poly, dom, w) == poly[i]


@pytest.mark.parametrize("bit_reversed", (False, True))
@pytest.mark.parametrize("N", SIZES)
def test_quotient_satisfies_the_opening_identity(N, bit_reversed):
    dom = K.domain(N, bit_reversed)
    poly = _poly(N, 2)
    setup = K.Setup(TAU, dom)
    p_tau = setup.at_tau(poly)
    assert p_tau == K.interpolate_direct(poly, dom, setup.tau)
    rng = random.Random(f"kzg q {N}")
    for z in list(dom) + [0, rng.randrange(Q)]:
        y, q = K.quotient(poly, dom, z)
        assert y == K.interpolate_direct(poly, dom, z)
        assert (p_tau - y) % Q == setup.at_tau(q) * (setup.tau - z) % Q, (N, z)


def test_constant_and_zero_polynomials():
    dom = K.domain(8)
    for c in (0, 5, Q - 1):
        y, q = K.quotient([c] * 8, dom, 1234567)
        assert y == c and q == [0] * 8
        y, q = K.quotient([c] * 8, dom, dom[3])
        assert y == c and q == [0] * 8


def test_model_verifies_a_good_opening_and_refuses_a_bad_one():
    dom = K.domain(8)
    poly = _poly(8, 3)
    setup = K.Setup(TAU, dom)
    C = K.commit(poly, setup)
    y, proof = K.open(poly, 77, setup)
    # the expectations in the exponent agree with the sums over the setup's points
    assert setup.at_tau(K.quotient(poly, dom, 77)[1]) == (setup.at_tau(poly) - y) * pow(setup.tau - 77, -1, Q) % Q
    assert K.verify(C, 77, y, proof, setup.tau_g2)
    assert not K.verify(C, 77, (y + 1) % Q, proof, setup.tau_g2)


def test_host_entry_points_refuse_bad_shapes_without_a_gpu():
    """Shapes, options and null buffers are refused with ECCX_ERR_ARG (-2) before a device is touched: no context exists on
    a machine without a GPU, and none is needed to be told no."""
    from eccoxide_amd import _lib

    lib = _lib.load()
    b = ctypes.create_string_buffer(64 * 96)
    ERR_ARG = -2
    for N, m in ((3, 1), (6, 2), (0, 1), (1 << 21, 1), (1 << 20, (1 << 7) + 1), (4096, (1 << 15) + 1)):
        assert lib.eccx_kzg_eval(None, N, m, b, b, b, b, b, 0) == ERR_ARG, (N, m)
        assert lib.eccx_kzg_commit(None, N, m, b, b, b, b, 0) == ERR_ARG, (N, m)
        assert lib.eccx_kzg_open(None, N, m, b, b, b, b, b, b, b, 0) == ERR_ARG, (N, m)
        assert lib.eccx_kzg_reserve(None, N, m) == ERR_ARG, (N, m)
    for opts in (1, 1 << 6, 1 << 31):
        assert lib.eccx_kzg_eval(None, 8, 1, b, b, b, b, b, opts) == ERR_ARG
        assert lib.eccx_kzg_commit(None, 8, 1, b, b, b, b, opts) == ERR_ARG
        assert lib.eccx_kzg_open(None, 8, 1, b, b, b, b, b, b, b, opts) == ERR_ARG
        assert lib.eccx_kzg_verify(None, 1, b, b, b, b, b, b, opts) == ERR_ARG
    assert lib.eccx_kzg_eval(None, 8, 1, None, b, b, b, b, 0) == ERR_ARG
    assert lib.eccx_kzg_commit(None, 8, 1, b, None, b, b, 0) == ERR_ARG
    assert lib.eccx_kzg_open(None, 8, 1, b, b, b, b, b, None, b, 0) == ERR_ARG
    assert lib.eccx_kzg_verify(None, 1, b, b, b, b, None, b, 0) == ERR_ARG
    assert lib.eccx_kzg_eval_dev(None, 8, 1, None, None, None, None, None, 0, None) == ERR_ARG
    assert lib.eccx_kzg_verify_dev(None, 1, None, None, None, None, None, None, 0, None) == ERR_ARG
