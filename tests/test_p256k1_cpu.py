"""secp256k1 (p256k1), CPU side: the extracted fixture against the Python reference, the generated constants, the
endomorphism and its signed lattice split (model of kernels_coz.hpp glv_split_lattice), an exhaustive model of the
two-half ladder's exceptional cases on small curves of the same family, and the C ABI's sizes.  No GPU."""
import hashlib
import random
import re

from oracle import ecc_ref as R
from tests import ct_model as M
from tests import oracle_lib
from tests import p256k1_ref as K
from tests.oracle_lib import golden

FIX = golden("p256k1.json")


# ---- fixture (src/params/sec2.rs mod p256k1, src/tests/sage.rs, src/params/comb/p256k1.rs) ----------------------
def test_params_match_reference():
    f, c = FIX["params"], K.K1
    assert int(f["p"], 16) == c.p == 2**256 - 2**32 - 977 and int(f["order"], 16) == c.n
    assert int(f["a"], 16) == c.a == 0 and int(f["b"], 16) == c.b == 7 and int(f["b3"], 16) == c.b3 == 21
    assert int(f["gx"], 16) == c.gx and int(f["gy"], 16) == c.gy
    assert R.on_curve(c, K.G)
    assert K.mul(c.n) is None and K.mul(c.n - 1) == K.neg(K.G)  # cofactor 1: G has the curve's prime order


def test_sage_kg_vectors():
    kats = FIX["sage_kg"]
    assert len(kats) == 100
    for kv in kats:
        want = (int(kv["x"], 16), int(kv["y"], 16))
        k = kv["k"]
        assert K.mul(k) == want, k
        # the reference's own comb algorithm and fixed-window ladder reach the same point
        kb = k.to_bytes(32, "big")
        assert K.mul_base_ref(kb) == want
        if k % 10 == 1:
            assert R.ref_to_affine(K.K1, K.ladder_proj(kb, K.G)) == want


def test_comb_table_hash():
    comb = FIX["comb"]
    table = K.comb_table()
    assert comb["windows"] == len(table) == 64
    h = hashlib.sha256()
    for row in table:
        for x, y in row:
            h.update(x.to_bytes(32, "big"))
            h.update(y.to_bytes(32, "big"))
    assert h.hexdigest() == comb["sha256_xy_concat"]
    for w, row in comb["samples"].items():
        for j, (x, y) in enumerate(row):
            assert table[int(w)][j] == (int(x, 16), int(y, 16))


# ---- generated constants (tools/gen_curve_consts.py -> curve_consts.inc) ---------------------------------------------
def _struct(name):
    txt = open(oracle_lib.ROOT + "/eccoxide_amd/csrc/curve_consts.inc").read()
    body = txt[txt.index("struct %s {" % name):]
    return body[: body.index("\n};")]


def _num(body, f):
    return int(re.search(r"\b%s = (-?\w+?)u?;" % f, body).group(1), 0)


def _arr(body, f):
    m = re.search(r"(?:uint32_t|int) %s\[\d+\] = \{([^}]*)\}" % f, body)
    return [int(v.strip().rstrip("u"), 0) for v in m.group(1).split(",")]


def test_saturated_constants():
    body, c = _struct("P256K1"), K.K1
    val = lambda f: sum(v << (32 * i) for i, v in enumerate(_arr(body, f)))
    L = _num(body, "L")
    assert L == 8 and _num(body, "FB") == 32 and _num(body, "SB") == 32
    assert _num(body, "A0") == 1 and _num(body, "PRIME_ORDER") == 1 and _num(body, "NBITS") == 256
    assert _num(body, "MERSENNE") == 0 and _num(body, "PM19") == 0
    Rm = 1 << 256
    assert val("P") == c.p and val("ONE") == Rm % c.p and val("R2") == Rm * Rm % c.p and val("PM2") == c.p - 2
    assert _num(body, "N0") == (-pow(c.p, -1, 1 << 32)) % (1 << 32)
    assert val("B") == 7 * Rm % c.p and val("B3") == 21 * Rm % c.p
    assert val("GX") == c.gx * Rm % c.p and val("GY") == c.gy * Rm % c.p


def test_unsaturated_constants():
    body, c = _struct("P256K1U"), K.K1
    N, B = _num(body, "N"), _num(body, "B")
    assert (N, B, _num(body, "KIND")) == (9, 29, 1)  # general Montgomery: p = 0x1ffffc2f mod 2^29, not -1
    assert c.p % (1 << B) == 0x1FFFFC2F
    val = lambda f: sum(v << (B * i) for i, v in enumerate(_arr(body, f)))
    p, Rm = c.p, 1 << (B * N)
    assert val("P") == p and val("PP1") == p + 1 and val("P2") == 2 * p
    assert all(d < (1 << B) for f in ("P", "ONE", "R2", "GX", "GY", "CB", "CB3", "BETA") for d in _arr(body, f)[:-1])
    assert val("ONE") == Rm % p and val("R2") == Rm * Rm % p
    assert val("GX") == c.gx * Rm % p and val("GY") == c.gy * Rm % p
    assert val("CB") == 7 * Rm % p and val("CB3") == 21 * Rm % p and val("BETA") == K.BETA * Rm % p
    bias = _arr(body, "BIAS")
    assert val("BIAS") == 4 * p and all(d >= (1 << B) - 1 for d in bias[:-1])
    assert _num(body, "N0B") == (-pow(p, -1, 1 << B)) % (1 << B)
    assert _num(body, "TOPSHIFT") == 256 - B * (N - 1) and _num(body, "QMUL") == 0  # top digit of p all ones
    assert _num(body, "RP") == Rm // p
    root = sum(v << (32 * i) for i, v in enumerate(_arr(body, "ROOT_EXP")))
    assert root == (p + 1) // 4 and p % 4 == 3
    segs = list(zip(_arr(body, "ROOT_ONES"), _arr(body, "ROOT_ZEROS")))
    e = 0
    for ones, zeros in segs:
        e = (((e << ones) | ((1 << ones) - 1)) << zeros)
    assert e == root
    # the column budget the 9 x 29 layout leaves a general Montgomery product: N products of K1 K2 tight limbs plus N
    # reduction products and a carry fit 64 bits for K1 K2 <= 6 (ufe.hpp UB<C>::KKMAX)
    kk = (2**64 - 1) // (N * (1 << (2 * B))) - 1
    assert kk == 6 and N * (kk + 1) * ((1 << B) - 1) ** 2 + (1 << 40) < 2**64


def test_glv_constants():
    body = _struct("P256K1_GLV")
    w = lambda f: sum(v << (32 * i) for i, v in enumerate(_arr(body, f)))
    assert w("N") == K.N and w("G1") == K.G1 and w("G2") == K.G2
    assert w("A1") == K.A1 and w("B1N") == -K.B1 and w("A2") == K.A2 and w("B2") == K.B2
    assert _num(body, "K_BITS") == 128


# ---- the endomorphism ---------------------------------------------------------------------------------------------
def test_glv_identities():
    n, p = K.N, K.P
    assert (K.LAMBDA**2 + K.LAMBDA + 1) % n == 0
    assert pow(K.BETA, 3, p) == 1 and K.BETA != 1
    assert K.mul(K.LAMBDA) == K.sigma(K.G) == (K.BETA * K.G[0] % p, K.G[1])
    # sigma acts as [lambda] on every point (cofactor 1): random multiples of G
    rng = random.Random(7)
    for _ in range(4):
        Pt = K.mul(rng.randrange(1, n))
        assert K.mul(K.LAMBDA, Pt) == K.sigma(Pt)
        assert K.sigma(K.sigma(K.sigma(Pt))) == Pt
    # the basis: both vectors in the lattice, determinant n
    assert (K.A1 + K.B1 * K.LAMBDA) % n == 0 and (K.A2 + K.B2 * K.LAMBDA) % n == 0
    assert K.A1 * K.B2 - K.A2 * K.B1 == n
    assert max(abs(v) for v in (K.A1, K.B1, K.A2, K.B2)).bit_length() <= 129


def _edge_scalars():
    n, lam = K.N, K.LAMBDA
    ks = [0, 1, 2, n - 1, n, n + 1, 2**256 - 1, lam, n - lam, (lam * lam) % n, n - 2, 2**255, 2**128, 2**128 - 1]
    for a, b in ((K.A1, K.B1), (K.A2, K.B2), (K.A1 + K.A2, K.B1 + K.B2), (K.A1 - K.A2, K.B1 - K.B2)):
        for m in (1, 2, 3, -1, -2):
            ks.append((m * (a + b * lam)) % n)  # lattice multiples: k = 0 mod n in disguise
            ks.append((m * a) % n)
            ks.append((m * b * lam) % n)
    # halves near +-2^127, 2^128 - 1 and 0 by construction: k = k1 + k2 lambda
    for k1 in (0, 1, -1, 2**127, -(2**127), 2**128 - 1, -(2**128 - 1), 2**126 + 12345):
        for k2 in (0, 1, -1, 2**127 - 1, -(2**127), 2**128 - 1, -(2**128 - 1)):
            ks.append((k1 + k2 * lam) % n)
    return ks


def test_split_model_edges_and_random():
    rng = random.Random(20)
    ks = _edge_scalars() + [rng.getrandbits(256) for _ in range(20000)] + [rng.randrange(K.N) for _ in range(5000)]
    for k in ks:
        k1, k2 = K.glv_split_lattice(k)
        assert (k1 + k2 * K.LAMBDA - k) % K.N == 0, hex(k)
        assert abs(k1) < 2**128 and abs(k2) < 2**128, hex(k)


def test_split_zero_halves_exist():
    """Scalars whose split has k1 = 0 or k2 = 0 (the GPU test feeds them): small k, and k = c lambda for small c."""
    assert K.glv_split_lattice(5)[1] == 0
    for c in (1, 2, 3, 1000):
        k1, k2 = K.glv_split_lattice(c * K.LAMBDA % K.N)
        assert k1 == 0 and k2 == c


# ---- exceptional cases of the signed two-half ladder (kernels_coz.hpp GLV, non-CT) --------------------------------
def _small_curves(count=3, lo=1000, hi=6000):
    """a = 0 curves y^2 = x^3 + b over p = 1 mod 3 with PRIME order r (cofactor 1), which carry the order-3
    endomorphism (beta x, y) = [lambda]."""
    out = []
    p = lo
    while len(out) < count and p < hi:
        p += 1
        if p % 3 != 1 or any(p % q == 0 for q in range(2, int(p**0.5) + 1)):
            continue
        sq = [0] * p
        for y in range(p):
            sq[y * y % p] += 1
        for b in range(1, 8):
            r = 1 + sum(sq[(x * x * x + b) % p] for x in range(p))
            if r < 50 or any(r % q == 0 for q in range(2, int(r**0.5) + 1)):
                continue
            c = R.WeierstrassParams("small", p=p, n=r, a=0, b=b, gx=0, gy=0, fb=2, sb=2, flavour="a0")
            gx = next(x for x in range(p) if sq[(x * x * x + b) % p])
            gy = next(y for y in range(p) if y * y % p == (gx**3 + b) % p)
            out.append((c, (gx, gy)))
            break
    return out


def _split_basis(r, lam):
    """Short basis of {(x, y): x + y lam = 0 mod r} (extended Euclid, as for secp256k1's)."""
    import math

    s0, t0, r0 = 1, 0, r
    s1, t1, r1 = 0, 1, lam
    rows = []
    while r1:
        q = r0 // r1
        r0, r1 = r1, r0 - q * r1
        s0, s1 = s1, s0 - q * s1
        t0, t1 = t1, t0 - q * t1
        rows.append((r1, t1, r0, t0))
    sq = math.isqrt(r)
    i = next(i for i, (ri, _, _, _) in enumerate(rows) if ri < sq)
    a1, b1 = rows[i][0], -rows[i][1]
    cand = [(rows[i - 1][0], -rows[i - 1][1]) if i > 0 else (r, 0)]
    if i + 1 < len(rows):
        cand.append((rows[i + 1][0], -rows[i + 1][1]))
    a2, b2 = min(cand, key=lambda v: v[0] ** 2 + v[1] ** 2)
    if a1 * b2 - a2 * b1 < 0:
        a2, b2 = -a2, -b2
    for a, b in ((a1, b1), (a2, b2)):
        assert (a + b * lam) % r == 0
    return a1, b1, a2, b2


def _split_small(r, basis, k):
    """The split of the kernel with exact rounding (the 2^384 fixed point of the real curve is a detail of its size)."""
    a1, b1, a2, b2 = basis
    kk = k - r if k >= r else k
    c1 = (2 * b2 * kk + r) // (2 * r)
    c2 = (-2 * b1 * kk + r) // (2 * r)
    return kk - c1 * a1 - c2 * a2, -c1 * b1 - c2 * b2


def _ladder_events(r, lam, k1, k2, kbits, wb=5):
    """Runs the kernel's schedule for the halves (k1, k2) in the exponent group Z/r: the accumulator starts at the top
    window's first signed addend, then (second half of the top window), per window wb doublings, + d1 P, + d2 sigma(P),
    each half's sign folded into its digits.  An addition whose accumulator equals +-entry (both not the neutral
    element) is an EVENT; the kernel resolves 'twice' by doubling (fix_lane) and 'cancel' by Z = 0, in every window.
    Returns (result exponent, events)."""
    assert abs(k1) < 1 << kbits and abs(k2) < 1 << kbits
    nwin = (kbits + 1 + wb - 1) // wb
    s1, s2 = (-1 if k1 < 0 else 1), (-1 if k2 < 0 else 1)
    d1, d2 = M.glv_digits(abs(k1), nwin, wb), M.glv_digits(abs(k2), nwin, wb)
    ev = []
    acc = None  # None: the point at infinity

    def add(win, half, e):
        nonlocal acc
        e %= r
        if e == 0:           # digit 0: kept
            return
        if acc is None:      # accumulator at infinity: the sum is the entry
            acc = e
            return
        if acc == e:
            ev.append((win, half, "twice"))
            acc = 2 * acc % r          # the doubling of the fix-up step
        elif (acc + e) % r == 0:
            ev.append((win, half, "cancel"))
            acc = None
        else:
            acc = (acc + e) % r

    for win in range(nwin - 1, -1, -1):
        if win != nwin - 1:
            for _ in range(wb):
                acc = None if acc is None else 2 * acc % r
        add(win, 0, s1 * d1[win])
        add(win, 1, s2 * d2[win] * lam)
    return (0 if acc is None else acc), ev


def test_two_half_ladder_exceptional_cases_exhaustive():
    curves = _small_curves()
    assert len(curves) >= 2
    seen = {"twice": 0, "cancel": 0}
    for c, G in curves:
        r, p = c.n, c.p
        # the endomorphism on this curve: beta a primitive cube root of 1 mod p, lambda the matching root mod r
        beta = next(x for x in range(2, p) if pow(x, 3, p) == 1)
        lams = [x for x in range(2, r) if (x * x + x + 1) % r == 0]
        sG = (beta * G[0] % p, G[1])
        lam = next(x for x in lams if R.affine_mul(c, x, G) == sG)
        # sigma = [lambda] on EVERY point (cofactor 1): all multiples of G
        pts = [None, G]
        for _ in range(2, r):
            pts.append(R.affine_add(c, pts[-1], G))
        for e in range(1, r):
            P_ = pts[e]
            assert pts[lam * e % r] == (beta * P_[0] % p, P_[1])
        basis = _split_basis(r, lam)
        kbits = 0
        for k in range(0, 2 * r):
            k1, k2 = _split_small(r, basis, k)
            assert (k1 + k2 * lam - k) % r == 0
            kbits = max(kbits, abs(k1).bit_length(), abs(k2).bit_length())
        # every pair of halves the ladder can be handed (not only what the split returns), both signs
        span = range(-(1 << kbits) + 1, 1 << kbits)
        for k1 in span:
            for k2 in span:
                got, ev = _ladder_events(r, lam, k1, k2, kbits)
                assert got == (k1 + k2 * lam) % r, (p, r, k1, k2)
                for win, half, kind in ev:  # resolved in every window and either half by the kernel
                    assert kind in ("twice", "cancel") and win >= 0 and half in (0, 1)
                    seen[kind] += 1
        # the split's own output, scalar by scalar, at point level: k * G
        kmax = min(1 << r.bit_length(), 2 * r)  # below 2^bits(r): one conditional subtraction reduces them
        for k in range(kmax):
            k1, k2 = _split_small(r, basis, k)
            e, _ = _ladder_events(r, lam, k1, k2, kbits)
            assert pts[e] == (R.affine_mul(c, k % r, G) if k % (kmax // 32) == 0 else pts[k % r])
    # the model is not vacuous: both kinds of collision happen on these curves
    assert seen["twice"] > 0 and seen["cancel"] > 0, seen


# ---- the C ABI ----------------------------------------------------------------------------------------------------
def test_abi_sizes():
    import eccoxide_amd as E
    from eccoxide_amd import _lib

    lib = _lib.load()
    assert E.P256K1 == 5 and E.curve_id("p256k1") == 5 and E.CURVE_NAMES[5] == "p256k1"
    assert lib.eccx_field_bytes(5) == 32 and lib.eccx_scalar_bytes(5) == 32
    assert lib.eccx_compressed_bytes(5) == 33
    assert E.field_bytes(5) == 32 and E.scalar_bytes(5) == 32
    assert lib.eccx_field_bytes(6) < 0  # still the last curve


def test_workload_order():
    from eccoxide_amd import workload as W

    assert W.order("p256k1") == K.N == int(FIX["params"]["order"], 16)


def test_rust_wrapper_sizes():
    """The Rust binding instantiates the sec2 macro for p256k1 with the sizes the library reports."""
    import os

    from eccoxide_amd import _lib

    lib = _lib.load()
    src = open(os.path.join(oracle_lib.ROOT, "rust", "eccoxide-gpu", "src", "lib.rs")).read()
    m = re.search(r"gpu_weierstrass_curve!\(p256k1, eccoxide::curve::sec2::p256k1, crate::ffi::ECCX_P256K1, (\d+), (\d+)\);", src)
    assert m and int(m.group(1)) == lib.eccx_field_bytes(5) and int(m.group(2)) == lib.eccx_scalar_bytes(5)
    assert "Curve::P256k1 => ffi::ECCX_P256K1" in src
    ffi = open(os.path.join(oracle_lib.ROOT, "rust", "eccoxide-gpu", "src", "ffi.rs")).read()
    assert "pub const ECCX_P256K1: c_int = 5;" in ffi
