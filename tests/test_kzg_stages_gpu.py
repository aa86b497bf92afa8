"""KZG's evaluation-and-quotient kernel run alone (tests/hip_kzg/libkzgcheck.so) against the Python model, byte for byte:
the values, the quotient evaluations and the flags.  One workgroup of 256 lanes takes a polynomial, lane l the evaluations
l, l + 256, ...: N = 1, 2 and 64 leave lanes idle, 256 fills them once, 512 and 1024 give every lane a run of 2 and 4;
with z_g = domain[g] for N = 512 every position of every lane's run is the one in-domain element once."""
import ctypes
import os
import random

import pytest

from tests import kzg_ref as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "hip_kzg", "libkzgcheck.so")
Q = K.Q


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("tests/hip_kzg/libkzgcheck.so missing: run __graft_entry__.build()")
    import torch  # noqa: F401  (one HIP runtime per process: the one torch brings)

    h = ctypes.CDLL(LIB)
    h.kzgcheck_eval_quotient.restype = ctypes.c_int
    h.kzgcheck_eval_quotient.argtypes = [ctypes.c_size_t, ctypes.c_size_t] + [ctypes.c_void_p] * 7
    return h


def run(lib, polys, zs, dom, quot=True):
    N, m = len(dom), len(zs)
    ys, fl = ctypes.create_string_buffer(m * 32), ctypes.create_string_buffer(m)
    q = ctypes.create_string_buffer(m * N * 32) if quot else None
    ninv = pow(N, -1, Q).to_bytes(32, "big")
    rc = lib.kzgcheck_eval_quotient(N, m, K.fr_bytes([p for poly in polys for p in poly]), K.fr_bytes(zs), K.fr_bytes(dom), ninv, ys, q, fl)
    assert rc == 0, f"hip error {rc}"
    return ys.raw, (q.raw if quot else None), fl.raw


def check(lib, polys, zs, dom):
    want = K.expected_eval_quotient(polys, zs, dom)
    got = run(lib, polys, zs, dom)
    assert got[2] == want[2], "flags"
    assert got[0] == want[0], "values"
    assert got[1] == want[1], "quotient evaluations"
    assert run(lib, polys, zs, dom, quot=False)[::2] == want[::2], "the evaluation alone"


@pytest.mark.parametrize("bit_reversed", (True, False))
@pytest.mark.parametrize("N", (1, 2, 64, 256, 512, 1024))
def test_eval_quotient_sizes(lib, N, bit_reversed):
    rng = random.Random(f"kzg stages {N}")
    dom = K.domain(N, bit_reversed)
    polys = [[rng.randrange(Q) for _ in range(N)] for _ in range(3)]
    zs = [rng.randrange(Q), dom[rng.randrange(N)], rng.randrange(Q)]  # outside, inside, outside the domain
    check(lib, polys, zs, dom)


def test_every_position_is_the_in_domain_element_once(lib):
    N = m = 512
    rng = random.Random("kzg hits")
    dom = K.domain(N)
    base = [rng.randrange(Q) for _ in range(N)]
    polys = [base[g:] + base[:g] for g in range(m)]  # distinct polynomials at the cost of one draw
    check(lib, polys, list(dom), dom)


def test_edge_points_and_polynomials(lib):
    N = 512
    rng = random.Random("kzg edges")
    dom = K.domain(N)
    rnd = [rng.randrange(Q) for _ in range(N)]
    ends = [0, Q - 1] * (N // 2)
    polys = [rnd, rnd, [0] * N, [0] * N, [7] * N, [Q - 1] * N, [Q - 1] * N, ends, ends]
    zs = [0, Q - 1, 12345, dom[5], dom[300], 99, dom[511], 0, dom[0]]
    check(lib, polys, zs, dom)


def test_values_not_below_r_reject(lib):
    N = 512
    rng = random.Random("kzg reject")
    dom = K.domain(N)
    good = [rng.randrange(Q) for _ in range(N)]
    bad_first, bad_last, bad_mid = [Q] + good[1:], good[:-1] + [(1 << 256) - 1], good[:300] + [Q + 5] + good[301:]
    polys = [good, bad_first, good, bad_last, bad_mid, good, good]
    zs = [5, 6, dom[9], 7, 8, Q, 9]
    want = K.expected_eval_quotient(polys, zs, dom)
    assert want[2] == bytes([0, 2, 0, 2, 2, 2, 0])
    check(lib, polys, zs, dom)
    # one domain element of r rejects every polynomial
    for at in (0, 255, 511):
        bad_dom = list(dom)
        bad_dom[at] = Q
        got = run(lib, polys[:3], zs[:3], bad_dom)
        assert got == (bytes(3 * 32), bytes(3 * N * 32), bytes([2, 2, 2])), at
