#!/usr/bin/env python3
"""Generate eccoxide_amd/csrc/curve_consts.inc: per-curve Montgomery constants as
32-bit little-endian limb arrays for the HIP kernels.

Self-contained (standard SEC 2 / BLS12-381 / RFC 8032 constants, plain big-int
math); does not import oracle/ or read /root/reference.  tests/ cross-check the
generated values against tests/golden/params.json.  The inputs are tests/golden/bls_h2c.json and
tests/golden/bls_h2c_g2.json: RFC 9380's constants for hashing to BLS12-381 G1 and G2 (sections
8.8.1 and 8.8.2, appendices E.2 and E.3), checked here for what makes them the right constants
before they are emitted; and tests/golden/jubjub.json for Jubjub's generator.

    python tools/gen_curve_consts.py > eccoxide_amd/csrc/curve_consts.inc
"""
import json
import os
import random
import sys

CURVES = [
    # name, p, b, gx, gy, field bytes, scalar bytes, flavour(0 = a=-3, 1 = a=0); the order n of the
    # generator is in ORDERS below (only its bit length reaches the kernels)
    ("P256", 2**256 - 2**224 + 2**192 + 2**96 - 1,
     0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B,
     0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296,
     0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5, 32, 32, 0),
    ("P384", 2**384 - 2**128 - 2**96 + 2**32 - 1,
     0xB3312FA7E23EE7E4988E056BE3F82D19181D9C6EFE8141120314088F5013875AC656398D8A2ED19D2A85C8EDD3EC2AEF,
     0xAA87CA22BE8B05378EB1C71EF320AD746E1D3B628BA79B9859F741E082542A385502F25DBF55296C3A545E3872760AB7,
     0x3617DE4A96262C6F5D9E98BF9292DC29F8F41DBD289A147CE9DA3113B5F0B8C00A60B1CE1D7E819D7A431D7C90EA0E5F, 48, 48, 0),
    ("P521", 2**521 - 1,
     0x0051953EB9618E1C9A1F929A21A0B68540EEA2DA725B99B315F3B8B489918EF109E156193951EC7E937B1652C0BD3BB1BF073573DF883D2C34F1EF451FD46B503F00,
     0x00C6858E06B70404E9CD9E3ECB662395B4429C648139053FB521F828AF606B4D3DBAA14B5E77EFE75928FE1DC127A2FFA8DE3348B3C1856A429BF97E7E31C2E5BD66,
     0x011839296A789A3BC0045C8A5FB42C7D1BD998F54449579B446817AFBD17273E662C97EE72995EF42640C550B9013FAD0761353C7086A272C24088BE94769FD16650, 66, 66, 0),
    ("BLS12_381", 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB,
     4,
     0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
     0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1, 48, 32, 1),
]

# order of the generator (prime) and cofactor of the curve
ORDERS = {
    "P256": (0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551, 1),
    "P384": (0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFC7634D81F4372DDF581A0DB248B0A77AECEC196ACCC52973, 1),
    "P521": (0x01FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFA51868783BF2F966B7FCC0148F709A5D03BB5C9B8899C47AEBB6FB71E91386409, 1),
    "BLS12_381": (0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001, 0x396C8C005555E1568C00AAAB0000AAAB),
}

# secp256k1 (SEC 2 v2 section 2.4.1; eccoxide's sec2::p256k1): a = 0, b = 7, cofactor 1.  Kept out of CURVES so
# that the blocks of the five original curves come out as before; emitted after them.
P256K1_CURVE = ("P256K1", 2**256 - 2**32 - 977, 7,
                0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
                0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8, 32, 32, 1)
ORDERS["P256K1"] = (0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141, 1)
# its endomorphism sigma(x, y) = (beta x, y) = [lambda](x, y) on every point, and the reduced basis
# (a1, b1), (a2, b2) of the lattice {(x, y): x + y lambda = 0 mod n} the scalar split rounds against
K1_LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
K1_BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
K1_A1 = 0x3086D221A7D46BCDE86C90E49284EB15
K1_B1 = -0xE4437ED6010E88286F547FA90ABFE4C3
K1_A2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8
K1_B2 = K1_A1

P25519 = 2**255 - 19
ED_D = (-121665 * pow(121666, -1, P25519)) % P25519
ED_GX = 0x216936D3CD6E53FEC0A4E231FDD6DC5C692CC7609525A7B2C9562D608F25D51A
ED_GY = 0x6666666666666666666666666666666666666666666666666666666666666658
ED25519_L = 2**252 + 27742317777372353535851937790883648493  # order of the base point (cofactor 8)


def limbs(x, n):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


# ---- BLS12-381 G1 endomorphism (subgroup test, GLV split) ------------------------------------
# seed x = -0xd201000000010000; group order r = x^4 - x^2 + 1, so lambda = -x^2 satisfies
# lambda^2 + lambda + 1 = 0 mod r and sigma(X, Y) = (beta X, Y) acts on G1 as [lambda] for one of
# the two primitive cube roots of unity beta in Fp.  Which one is settled by computing [x^2]G with
# textbook affine arithmetic: [x^2]G = -sigma(G) = (beta Gx, -Gy).
BLS_X_ABS = 0xD201000000010000


def _bls_beta():
    _, p, _, gx, gy, _, _, _ = CURVES[3]

    def add(P, Q):
        if P is None:
            return Q
        if Q is None:
            return P
        (x1, y1), (x2, y2) = P, Q
        if x1 == x2:
            if (y1 + y2) % p == 0:
                return None
            lam = 3 * x1 * x1 * pow(2 * y1, -1, p) % p
        else:
            lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
        x3 = (lam * lam - x1 - x2) % p
        return x3, (lam * (x1 - x3) - y1) % p

    acc = None
    for bit in bin(BLS_X_ABS * BLS_X_ABS)[2:]:
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, (gx, gy))
    beta = acc[0] * pow(gx, -1, p) % p
    assert pow(beta, 3, p) == 1 and beta != 1 and (p - acc[1]) % p == gy
    return beta


def _affine_mul(p, P, k):
    """k * P with textbook affine arithmetic on y^2 = x^3 + b (a = 0); None is the point at infinity."""
    def add(P, Q):
        if P is None:
            return Q
        if Q is None:
            return P
        (x1, y1), (x2, y2) = P, Q
        if x1 == x2:
            if (y1 + y2) % p == 0:
                return None
            lam = 3 * x1 * x1 * pow(2 * y1, -1, p) % p
        else:
            lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
        x3 = (lam * lam - x1 - x2) % p
        return x3, (lam * (x1 - x3) - y1) % p

    acc = None
    for bit in bin(k)[2:]:
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, P)
    return acc


def _k1_glv():
    """The P256K1_GLV constants, checked: lambda a cube root of unity mod n matching beta on G, and both
    basis vectors in the lattice.  g1 = round(2^384 b2 / n), g2 = round(-2^384 b1 / n): the split rounds
    c1 = k g1 / 2^384 and c2 = k g2 / 2^384 (kernels_coz.hpp glv_split_lattice)."""
    _, p, _, gx, gy, _, _, _ = P256K1_CURVE
    n = ORDERS["P256K1"][0]
    assert (K1_LAMBDA * K1_LAMBDA + K1_LAMBDA + 1) % n == 0
    assert pow(K1_BETA, 3, p) == 1 and K1_BETA != 1
    assert _affine_mul(p, (gx, gy), K1_LAMBDA) == (K1_BETA * gx % p, gy)
    assert (K1_A1 + K1_B1 * K1_LAMBDA) % n == 0 and (K1_A2 + K1_B2 * K1_LAMBDA) % n == 0
    g1 = ((K1_B2 << 384) + n // 2) // n
    g2 = ((-K1_B1 << 384) + n // 2) // n
    return n, g1, g2


def arr(name, vals):
    body = ", ".join("0x%08xu" % v for v in vals)
    return "  static constexpr uint32_t %s[%d] = {%s};" % (name, len(vals), body)


def emit_field(out, p, L, mersenne=0, pm19=0, plain=False):
    # Mersenne (2^k - 1) and pseudo-Mersenne (2^255 - 19) fields are kept in plain
    # (non-Montgomery) form: R = 1; so is 2^448 - 2^224 - 1 (plain)
    R = 1 if (mersenne or pm19 or plain) else 1 << (32 * L)
    out.append("  static constexpr int MERSENNE = %d;  // k if p = 2^k - 1 (plain representation, fold reduction), else 0" % mersenne)
    out.append("  static constexpr int PM19 = %d;  // 1 if p = 2^255 - 19 (plain representation, fold by 38), else 0" % pm19)
    out.append(arr("P", limbs(p, L)))
    out.append(arr("ONE", limbs(R % p, L)))
    out.append(arr("R2", limbs(R * R % p, L)))
    out.append(arr("PM2", limbs(p - 2, L)))
    out.append("  static constexpr uint32_t N0 = 0x%08xu;  // -p^-1 mod 2^32" % ((-pow(p, -1, 1 << 32)) % (1 << 32)))
    # p + 1 (used when N0 == 1: "+ m*p" is then "drop the low limb, + m*(p+1)")
    out.append(arr("PP1", limbs((p + 1) % (1 << (32 * L)), L)))
    out.append("  static constexpr int PBITS = %d;" % p.bit_length())
    # constants of the division-step inversion (inv_gcd.hpp): the modulus in 30-bit limbs,
    # p^-1 mod 2^30, and the number of 30-step batches that the Bernstein-Yang bound
    # floor((49 bits + 57) / 17) divsteps (delta = 1 variant, any odd modulus) rounds up to (but see INV30_HD)
    nl = (p.bit_length() + 1 + 29) // 30 + (1 if (p.bit_length() + 1) % 30 == 0 else 0)
    nl = max(nl, (p.bit_length() + 2 + 29) // 30)  # room for values in (-2p, p) with a sign bit
    out.append("  static constexpr int INV30_N = %d;" % nl)
    out.append("  static constexpr int32_t P30[%d] = {%s};" % (nl, ", ".join("0x%08x" % ((p >> (30 * i)) & 0x3FFFFFFF) for i in range(nl))))
    out.append("  static constexpr uint32_t P30_INV = 0x%08xu;  // p^-1 mod 2^30" % pow(p, -1, 1 << 30))
    # moduli of at most 256 bits: the division step started at delta = 1/2, for which 590 steps are PROVEN
    # to suffice for every odd modulus below 2^256 (convex-hull bound of github.com/sipa/safegcd-bounds, the
    # figure libsecp256k1's modinv32 relies on: 20 batches of 30) -- against 724 / 741 with delta = 1
    hd = p.bit_length() <= 256
    out.append("  static constexpr bool INV30_HD = %s;  // %s" % (
        ("true", "division steps start at delta = 1/2 (590-step bound below 2^256)") if hd else
        ("false", "division steps start at delta = 1 (Bernstein-Yang bound)")))
    out.append("  static constexpr int INV30_BATCHES = %d;" % (20 if hd else ((49 * p.bit_length() + 57) // 17 + 29) // 30))
    return R


def digits(x, bits, n):
    return [(x >> (bits * i)) & ((1 << bits) - 1) for i in range(n)]


def runs_of(e):
    """Binary expansion of e from the top bit as (ones, zeros) runs."""
    segs, b = [], bin(e)[2:]
    i = 0
    while i < len(b):
        j = i
        while j < len(b) and b[j] == "1":
            j += 1
        k = j
        while k < len(b) and b[k] == "0":
            k += 1
        segs.append((j - i, k - j))
        i = k
    assert sum(o + z for o, z in segs) == e.bit_length()
    return segs


def emit_unsat(out, name, sat_name, p, gx, gy, bits, n, kind, extra=(), solinas=(), sparse=False, root_exp=0):
    """Constants of the unsaturated representation: n limbs of `bits` bits in 32-bit registers.
    kind 0: Montgomery, R = 2^(bits*n), p = -1 mod 2^bits (reduce with the digits of p + 1)
    kind 1: Montgomery, general p (m = acc * N0B mod 2^bits)
    kind 2: p = 2^k - 1, plain representation, 2^(bits*n) = 2^(bits*n - k) mod p folded into the product
    kind 3: p = 2^255 - 19, plain representation, 2^(bits*n) = 19 * 2^(bits*n - 255) mod p
    (kind 4, 2^448 - 2^224 - 1, has an emitter of its own: emit_goldilocks)
    BIAS is 4p written with every limb >= 2^bits - 1 (the largest tight limb) so that
    a + BIAS - b never borrows for tight b < 3p."""
    mont = kind in (0, 1)
    R = (1 << (bits * n)) if mont else 1
    pbits = p.bit_length()
    if kind == 0:
        assert p % (1 << bits) == (1 << bits) - 1, "needs p = -1 mod 2^bits (m = low limb)"
    d = digits(4 * p, bits, n)
    assert sum(x << (bits * i) for i, x in enumerate(d)) == 4 * p or 4 * p >= 1 << (bits * n)
    d[n - 1] = (4 * p) >> (bits * (n - 1))  # the top digit takes whatever is left
    bias = [d[0] + (1 << bits)] + [d[i] + (1 << bits) - 1 for i in range(1, n - 1)] + [d[n - 1] - 1]
    assert sum(b << (bits * i) for i, b in enumerate(bias)) == 4 * p
    assert all(b >= (1 << bits) - 1 for b in bias[:-1]) and all(b < (1 << (bits + 1)) for b in bias)
    # a tight value below 3p (Montgomery kinds) or below 2^(bits*n) (plain kinds) has a top digit <= bias top
    top_tight = ((3 * p) >> (bits * (n - 1))) if (mont or kind == 3) else (1 << bits) - 1
    assert bias[-1] >= top_tight, (name, hex(bias[-1]), hex(top_tight))
    topshift = pbits - bits * (n - 1)
    assert 0 < topshift < bits
    ptop = p >> (bits * (n - 1))
    # quotient estimate for the weak reduction: q = top >> TOPSHIFT when the top digit of p is
    # all ones below bit TOPSHIFT (Solinas / Mersenne), else q = mulhi(top, QMUL) (never too large)
    qmul = 0 if ptop == (1 << topshift) - 1 else (1 << 32) // (ptop + 1)
    out.append("struct %s {" % name)
    out.append("  using Sat = %s;          // saturated twin (byte I/O, validation, normalisation)" % sat_name)
    out.append("  static constexpr int N = %d;     // limbs" % n)
    out.append("  static constexpr int B = %d;    // bits per limb" % bits)
    out.append("  static constexpr int KIND = %d;  // 0 Montgomery p = -1 mod 2^B, 1 Montgomery general, 2 Mersenne (plain), 3 2^255-19 (plain)" % kind)
    out.append("  static constexpr uint32_t FOLD = %du;  // 2^(B*N) mod p where that is small (kinds 2, 3), else 0" % ((1 << (bits * n)) % p if kind in (2, 3) else 0))
    out.append("  static constexpr int PBITS = %d;" % pbits)
    out.append("  static constexpr int TOPSHIFT = %d;  // bit PBITS inside the top limb" % topshift)
    out.append("  static constexpr uint32_t QMUL = 0x%08xu;  // 0: quotient estimate is a shift" % qmul)
    out.append("  static constexpr uint32_t RP = %du;  // floor(R / p), capped" % min(R // p, 1 << 20))
    out.append("  static constexpr uint32_t MASK = 0x%08xu;" % ((1 << bits) - 1))
    out.append("  static constexpr uint32_t N0B = 0x%08xu;  // -p^-1 mod 2^B" % ((-pow(p, -1, 1 << bits)) % (1 << bits)))
    out.append(arr("P", digits(p, bits, n)))
    # p + 1: adding m*p with m = the low limb of the accumulator is "drop that limb, add
    # m*(p+1)", and p + 1 has far fewer non-zero digits (p = -1 mod 2^96 for P-256)
    out.append(arr("PP1", digits(p + 1, bits, n)))
    out.append(arr("P2", digits(2 * p, bits, n)))
    out.append(arr("ONE", digits(R % p, bits, n)))
    out.append(arr("R2", digits(R * R % p, bits, n)))
    out.append(arr("BIAS", bias))
    # R of the saturated twin (2^(32 L) mod p, plain digits): multiplying by it on the way out
    # yields the twin's Montgomery form directly
    Ls = (pbits + 31) // 32
    out.append(arr("RS", digits(((1 << (32 * Ls)) % p) if mont else 1, bits, n)))
    # Solinas form p + 1 = 2^PBITS + sum(sign * 2^e): lets the weak reduction take off q*p with
    # shifts of q instead of multiplications (kind 0 only); terms as (limb, shift, sign)
    if solinas:
        assert (1 << pbits) + sum(sg << e for e, sg in solinas) == p + 1
        terms = [(e // bits, e % bits, sg) for e, sg in solinas]
        assert all(l < n - 1 for l, _, _ in terms)
        pos = [l for l, _, sg in terms if sg > 0]   # a positive term is subtracted: may borrow
        out.append("  static constexpr int SOL_N = %d;" % len(terms))
        out.append("  static constexpr int SOL_LIMB[%d] = {%s};" % (len(terms), ", ".join(str(t[0]) for t in terms)))
        out.append("  static constexpr int SOL_SHIFT[%d] = {%s};" % (len(terms), ", ".join(str(t[1]) for t in terms)))
        out.append("  static constexpr int SOL_SIGN[%d] = {%s};" % (len(terms), ", ".join(str(t[2]) for t in terms)))
        out.append("  static constexpr int SOL_BIAS_FROM = %d;  // lowest limb a subtraction touches" % (min(pos) if pos else n))
    else:
        out.append("  static constexpr int SOL_N = 0;")
    # sparse Montgomery reduction: m*(p+1) added as signed shifted copies of m, one per term of
    # p + 1 (column offset, shift inside the column, sign) instead of one product per non-zero
    # digit -- pays when p + 1 has long runs of ones (P-384: 4 terms against 12 digits)
    if sparse:
        allterms = [(pbits, 1)] + list(solinas)
        out.append("  static constexpr int SPARSE_N = %d;" % len(allterms))
        out.append("  static constexpr int SPARSE_OFF[%d] = {%s};" % (len(allterms), ", ".join(str(e // bits) for e, _ in allterms)))
        out.append("  static constexpr int SPARSE_SHIFT[%d] = {%s};" % (len(allterms), ", ".join(str(e % bits) for e, _ in allterms)))
        out.append("  static constexpr int SPARSE_SIGN[%d] = {%s};" % (len(allterms), ", ".join(str(sg) for _, sg in allterms)))
        assert all(0 < e // bits < n for e, _ in allterms)
    else:
        out.append("  static constexpr int SPARSE_N = 0;")
    out.append(arr("GX", digits(gx * R % p, bits, n)))
    out.append(arr("GY", digits(gy * R % p, bits, n)))
    for cname, val in extra:
        out.append(arr(cname, digits(val * R % p, bits, n)))
    # exponent of the square-root candidate (point decompression): (p + 1) / 4 for p = 3 mod 4,
    # (p - 5) / 8 for 2^255 - 19.  As runs of ones and zeros from the top bit (a few long runs
    # for the Solinas / Mersenne primes: addition chain on x^(2^k - 1)), and as 32-bit words
    # for the 2-bit-window loop used when the pattern is irregular (BLS12-381).
    segs = runs_of(root_exp)
    out.append("  static constexpr int ROOT_BITS = %d;" % root_exp.bit_length())
    out.append("  static constexpr int ROOT_CHAIN = %d;  // 1: few long runs, use the run chain" % (1 if len(segs) <= 8 else 0))
    if len(segs) <= 8:
        out.append("  static constexpr int ROOT_SEGS = %d;" % len(segs))
        out.append("  static constexpr int ROOT_ONES[%d] = {%s};" % (len(segs), ", ".join(str(o) for o, _ in segs)))
        out.append("  static constexpr int ROOT_ZEROS[%d] = {%s};" % (len(segs), ", ".join(str(z) for _, z in segs)))
    else:
        out.append("  static constexpr int ROOT_SEGS = 0;")
    nw = (root_exp.bit_length() + 31) // 32
    out.append("  static constexpr uint32_t ROOT_EXP[%d] = {%s};" % (nw, ", ".join("0x%08xu" % ((root_exp >> (32 * i)) & 0xFFFFFFFF) for i in range(nw))))
    out.append("};")
    out.append("")


P448 = 2**448 - 2**224 - 1
X448_A24 = 39082  # (156326 + 2) / 4: the ladder adds a24 * E to BB (RFC 7748 section 5 writes AA + 39081 * E)
X448_U = 5        # the base point's u


def emit_goldilocks(out):
    """CURVE448 / CURVE448U: p = 2^448 - 2^224 - 1 in plain representation, 16 limbs of 28 bits (kind 4, ufe.hpp).
    phi = 2^224 is the boundary of limb 8 and 2^448 = phi + 1 (mod p), so the product's columns 16..30 fold onto columns
    0..14 and 8..22 inside the accumulators.  BIAS is 2p (not 4p: 4p does not fit 16 limbs below 2^29) spread so that
    every limb is at least 2^28 + 2^27: a + BIAS - b has no negative limb for any b whose limbs stay below that, and is
    non-negative as a value because such a b is below 2p."""
    p, bits, n, L = P448, 28, 16, 14
    assert p.bit_length() == 448 == bits * n == 32 * L
    assert ((1 << 448) - (1 << 224) - 1) % p == 0 and ((1 << 448) % p) == (1 << 224) + 1
    # prime (Miller-Rabin on fixed bases is enough for a constant everybody knows), p = 3 mod 4
    assert p % 4 == 3 and all(pow(a, p - 1, p) == 1 for a in (2, 3, 5, 7, 11))
    d = digits(2 * p, bits, n)
    d[n - 1] = (2 * p) >> (bits * (n - 1))
    bias = [d[0] + (1 << bits)] + [d[i] + (1 << bits) - 1 for i in range(1, n - 1)] + [d[n - 1] - 1]
    assert sum(b << (bits * i) for i, b in enumerate(bias)) == 2 * p
    assert all((1 << bits) + (1 << (bits - 1)) <= b < (1 << (bits + 1)) for b in bias)
    out.append("")
    out.append("struct CURVE448;")
    out.append("struct CURVE448U {")
    out.append("  using Sat = CURVE448;          // saturated twin (byte I/O, normalisation)")
    out.append("  static constexpr int N = %d;     // limbs" % n)
    out.append("  static constexpr int B = %d;    // bits per limb" % bits)
    out.append("  static constexpr int KIND = 4;  // 4: 2^448 - 2^224 - 1 (plain), 2^448 = 2^224 + 1 folded inside the columns")
    out.append("  static constexpr uint32_t FOLD = 0u;")
    out.append("  static constexpr int PBITS = %d;" % p.bit_length())
    out.append("  static constexpr int TOPSHIFT = %d;  // bit PBITS inside the top limb: the limb's whole width" % (448 - bits * (n - 1)))
    out.append("  static constexpr uint32_t QMUL = 0x00000000u;")
    out.append("  static constexpr uint32_t RP = 1u;  // plain representation")
    out.append("  static constexpr uint32_t MASK = 0x%08xu;" % ((1 << bits) - 1))
    out.append("  static constexpr uint32_t N0B = 0x%08xu;  // -p^-1 mod 2^B" % ((-pow(p, -1, 1 << bits)) % (1 << bits)))
    out.append("  static constexpr int PHI_LIMB = %d;  // 2^224 = 2^(B * PHI_LIMB)" % (224 // bits))
    out.append(arr("P", digits(p, bits, n)))
    out.append(arr("PP1", digits(p + 1, bits, n)))
    out.append(arr("P2", digits(p, bits, n)) + "  // 2p has 449 bits: a reduced value (below 2^448 + 2^226) is never 2p; p again")
    out.append(arr("ONE", digits(1, bits, n)))
    out.append(arr("R2", digits(1, bits, n)))
    out.append(arr("BIAS", bias) + "  // 2p")
    out.append(arr("RS", digits(1, bits, n)))
    out.append("  static constexpr int SOL_N = 0;")
    out.append("  static constexpr int SPARSE_N = 0;")
    out.append(arr("GU", digits(X448_U, bits, n)) + "  // u of the base point")
    out.append("  static constexpr uint32_t A24 = %du;  // (A + 2) / 4, A = 156326" % X448_A24)
    out.append("};")
    out.append("struct CURVE448 {")
    out.append("  static constexpr int L = %d;" % L)
    out.append("  static constexpr int FB = 56;")
    out.append("  static constexpr int SB = 56;")
    emit_field(out, p, L, 0, 0, plain=True)
    out.append("};")


JUBJUB_Q = ORDERS["BLS12_381"][0]  # the BLS12-381 scalar field Fr is Jubjub's base field
JUBJUB_R = 0x0E7DB4EA6533AFA906673B0101343B00A6682093CCC81082D0970E5ED6F72CB7  # order of the generator (cofactor 8)


def emit_jubjub(out):
    """JUBJUBU / JUBJUB: the twisted Edwards curve -x^2 + y^2 = 1 + d x^2 y^2 over Fr, d = -10240/10241 (computed here),
    the generator from tests/golden/jubjub.json, checked here for what makes them the right constants.  JUBJUBU is general
    Montgomery on 9 x 29 bits (R = 2^261), JUBJUB its saturated twin (R = 2^256) with big-endian byte I/O.  Fr has
    2-adicity 32: ROOT_EXP is (t - 1) / 2 for q - 1 = 2^32 t, TS_Z = 5^t the root of unity of order 2^32 the
    Tonelli-Shanks loop of the decoder starts from."""
    q, r = JUBJUB_Q, JUBJUB_R
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "jubjub.json")
    with open(path) as f:
        c = json.load(f)["params"]
    gx, gy = int(c["gx"], 16), int(c["gy"], 16)
    d = (-10240 * pow(10241, -1, q)) % q
    leg = lambda v: pow(v, (q - 1) // 2, q)
    assert all(pow(a, q - 1, q) == 1 for a in (2, 3, 5, 7, 11)) and q.bit_length() == 255
    assert d == int(c["d"], 16) and 2 * d % q == int(c["d2"], 16) and int(c["a"], 16) == q - 1 and int(c["order"], 16) == r
    # a = -1 is a square and d is not: the unified addition is complete on the whole curve, cofactor part included
    assert leg(q - 1) == 1 and leg(d) == q - 1
    # -1/d is not a square: d y^2 + 1 never vanishes, the decoder has no v == 0 case
    assert leg((-pow(d, -1, q)) % q) == q - 1
    assert (gy * gy - gx * gx - 1 - d * gx * gx % q * gy * gy) % q == 0, "the generator is off the curve"

    def add(P, Q):
        (x1, y1), (x2, y2) = P, Q
        k = d * x1 * x2 * y1 * y2 % q
        return ((x1 * y2 + y1 * x2) * pow(1 + k, -1, q) % q, (y1 * y2 + x1 * x2) * pow(1 - k, -1, q) % q)

    acc = (0, 1)
    for bit in bin(r)[2:]:
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, (gx, gy))
    assert acc == (0, 1), "r G is not the neutral element"
    S = 32
    assert (q - 1) % (1 << S) == 0 and ((q - 1) >> S) & 1
    t = (q - 1) >> S
    z = pow(5, t, q)
    assert leg(5) == q - 1 and pow(z, 1 << (S - 1), q) == q - 1
    out.append("")
    out.append("struct JUBJUB;")
    emit_unsat(out, "JUBJUBU", "JUBJUB", q, gx, gy, 29, 9, 1, extra=(("D2", 2 * d % q), ("D", d), ("TS_Z", z)),
               root_exp=(t - 1) // 2)
    assert out[-1] == "" and out[-2] == "};"
    del out[-1]
    L = 8
    out.append("struct JUBJUB {")
    out.append("  static constexpr int L = 8;")
    out.append("  static constexpr int FB = 32;")
    out.append("  static constexpr int SB = 32;")
    out.append("  static constexpr bool EDWARDS = true;  // a = -1 twisted Edwards, as ED25519")
    out.append("  static constexpr bool IO_BE = true;    // field elements travel big-endian (ED25519: little-endian)")
    out.append("  static constexpr int TS_S = %d;         // 2-adicity of q - 1" % S)
    R = emit_field(out, q, L)
    out.append(arr("D2", limbs(2 * d * R % q, L)))
    out.append(arr("GX", limbs(gx * R % q, L)))
    out.append(arr("GY", limbs(gy * R % q, L)))
    out.append("};")


def emit_sat(out, name, p, b, gx, gy, fb, sb, a0):
    """The saturated parameter struct of a short-Weierstrass curve (fe.hpp / curve.hpp)."""
    L = (p.bit_length() + 31) // 32
    out.append("struct %s {" % name)
    out.append("  static constexpr int L = %d;   // 32-bit limbs" % L)
    out.append("  static constexpr int FB = %d;  // field bytes" % fb)
    out.append("  static constexpr int SB = %d;  // scalar bytes" % sb)
    out.append("  static constexpr int A0 = %d;  // 1: a = 0 (uses B3), 0: a = -3 (uses B)" % a0)
    order, cof = ORDERS[name]
    out.append("  static constexpr int NBITS = %d;  // bit length of the generator's (prime) order" % order.bit_length())
    out.append("  static constexpr int PRIME_ORDER = %d;  // 1: cofactor 1, every curve point has that order" % (1 if cof == 1 else 0))
    R = emit_field(out, p, L, 521 if name == "P521" else 0)
    out.append(arr("B", limbs(b * R % p, L)))
    out.append(arr("B3", limbs(3 * b * R % p, L)))
    out.append(arr("GX", limbs(gx * R % p, L)))
    out.append(arr("GY", limbs(gy * R % p, L)))
    out.append("};")
    out.append("")


def arr2(name, rows):
    body = ",\n".join("      {%s}" % ", ".join("0x%08xu" % v for v in r) for r in rows)
    return "  static constexpr uint32_t %s[%d][%d] = {\n%s};" % (name, len(rows), len(rows[0]), body)


def emit_bls_h2c(out):
    """BLS12_381_H2C: the constants of hash_to_curve / encode_to_curve for G1 (kernels_h2c.hpp) in the working form of
    BLS12_381U (14 x 28-bit Montgomery digits): the isogenous curve E': y^2 = x^3 + A'x + B', Z = 11, sqrt(-Z), the
    11-isogeny's four polynomials (ascending; the denominators monic, leading 1 not stored), 2^256 R^2 for the
    512-bit reduction and the exponent (p - 3) / 4 of sqrt_ratio_3mod4."""
    _, p, b, _, _, _, _, _ = CURVES[3]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "bls_h2c.json")
    with open(path) as f:
        c = json.load(f)["constants"]
    z = c["z"]
    ia, ib, c2 = int(c["iso_a"], 16), int(c["iso_b"], 16), int(c["sqrt_minus_z"], 16)
    polys = {k: [int(h, 16) for h in c[k]] for k in ("x_num", "x_den", "y_num", "y_den")}
    # what makes them the right constants
    assert p % 4 == 3 and all(0 <= v < p for v in [ia, ib, c2] + sum(polys.values(), []))
    assert c2 * c2 % p == (-z) % p, "c2 is not a square root of -Z"
    assert pow(z, (p - 1) // 2, p) == p - 1, "Z is a square"
    assert ia * ib % p != 0
    assert [len(polys[k]) for k in ("x_num", "x_den", "y_num", "y_den")] == [12, 10, 16, 15], "degrees of the 11-isogeny"
    assert polys["x_num"][-1] != 0 and polys["y_num"][-1] != 0

    def ev(co, x, monic):
        acc = sum(v * pow(x, i, p) for i, v in enumerate(co))
        return (acc + (pow(x, len(co), p) if monic else 0)) % p

    rng = random.Random(9380)
    seen = 0
    while seen < 16:  # random points of E' land on y^2 = x^3 + 4
        x = rng.randrange(p)
        g = (x * x * x + ia * x + ib) % p
        y = pow(g, (p + 1) // 4, p)
        if y * y % p != g:
            continue
        xd, yd = ev(polys["x_den"], x, True), ev(polys["y_den"], x, True)
        if xd == 0 or yd == 0:
            continue
        X = ev(polys["x_num"], x, False) * pow(xd, -1, p) % p
        Y = y * ev(polys["y_num"], x, False) * pow(yd, -1, p) % p
        assert (Y * Y - X * X * X - b) % p == 0, "the isogeny misses the curve"
        seen += 1
    bits, n = 28, 14
    R = 1 << (bits * n)
    mont = lambda v: digits(v * R % p, bits, n)
    out.append("")
    out.append("struct BLS12_381_H2C {  // RFC 9380 8.8.1 / E.2: hashing to G1, working form of BLS12_381U")
    out.append(arr("A", mont(ia)))
    out.append(arr("B", mont(ib)))
    out.append(arr("Z", mont(z)))
    out.append(arr("SQRT_MZ", mont(c2)) + "  // sqrt(-Z)")
    out.append(arr("R2_256", digits((1 << 256) * R * R % p, bits, n)) + "  // 2^256 R^2: a * R2_256 / R = a 2^256 R")
    for k in ("x_num", "x_den", "y_num", "y_den"):
        out.append(arr2(k.upper().replace("_", ""), [mont(v) for v in polys[k]]))
    e = (p - 3) // 4
    nw = (e.bit_length() + 31) // 32
    out.append("  static constexpr int ROOT_BITS = %d;  // of (p - 3) / 4" % e.bit_length())
    out.append("  static constexpr uint32_t ROOT_EXP[%d] = {%s};" % (nw, ", ".join("0x%08xu" % ((e >> (32 * i)) & 0xFFFFFFFF) for i in range(nw))))
    out.append("};")


def emit_bls_g2(out):
    """BLS12_381_G2: the twist E'(Fp2): y^2 = x^3 + 4(1 + u) in the working form of BLS12_381U (14 x 28-bit Montgomery
    digits per component, c0 then c1): b and the real part of 3b = 12 + 12u (both components are equal), the generator,
    the two coefficients of psi = twist o Frobenius o untwist (xi^-((p-1)/3), xi^-((p-1)/2) for xi = 1 + u, computed here
    and pinned against the reference's bytes by tests/test_g2_cpu.py), and the two public exponents of the complex-method
    square root."""
    p = CURVES[3][1]
    gx = (0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
          0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E)
    gy = (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
          0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE)

    def mul(a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)

    def power(a, e):
        r = (1, 0)
        while e:
            if e & 1:
                r = mul(r, a)
            a = mul(a, a)
            e >>= 1
        return r

    def inv(a):
        n = pow(a[0] * a[0] + a[1] * a[1], -1, p)
        return (a[0] * n % p, -a[1] * n % p)

    # the generator is on the twist, and psi maps it to the twist
    rhs = lambda x: tuple((c + 4) % p for c in mul(mul(x, x), x))
    assert mul(gy, gy) == rhs(gx)
    psi_x, psi_y = inv(power((1, 1), (p - 1) // 3)), inv(power((1, 1), (p - 1) // 2))
    conj = lambda a: (a[0], -a[1] % p)
    px, py = mul(conj(gx), psi_x), mul(conj(gy), psi_y)
    assert mul(py, py) == rhs(px)
    bits, n = 28, 14
    R = 1 << (bits * n)
    mont = lambda v: digits(v * R % p, bits, n)
    out.append("")
    out.append("struct BLS12_381_G2 {  // the twist y^2 = x^3 + 4(1 + u) over Fp2, working form of BLS12_381U")
    out.append(arr("CB", mont(4)) + "  // b = 4 + 4u: both components")
    out.append(arr("CB3", mont(12)) + "  // 3b = 12 + 12u: both components")
    for name, v in (("GX", gx), ("GY", gy), ("PSI_X", psi_x), ("PSI_Y", psi_y)):
        out.append(arr(name + "0", mont(v[0])))
        out.append(arr(name + "1", mont(v[1])))
    for name, e, what in (("PM3D4", (p - 3) // 4, "(p - 3) / 4"), ("PM1D2", (p - 1) // 2, "(p - 1) / 2")):
        nw = (e.bit_length() + 31) // 32
        out.append("  static constexpr int %s_BITS = %d;  // of %s" % (name, e.bit_length(), what))
        out.append("  static constexpr uint32_t %s[%d] = {%s};" % (name, nw, ", ".join("0x%08xu" % ((e >> (32 * i)) & 0xFFFFFFFF) for i in range(nw))))
    out.append("};")


def emit_bls_g2_h2c(out):
    """BLS12_381_G2_H2C: the constants of hash_to_curve / encode_to_curve for G2 (kernels_h2c_g2.hpp) in the working form
    of BLS12_381U, each Fp2 element as its c0 digits then its c1 digits: the isogenous curve E': y^2 = x^3 + A'x + B'
    with A' = 240u, B' = 1012(1 + u), Z = -(2 + u), the exponent c3 and the constants c6, c7 of the any-field sqrt_ratio
    (appendix F.2.1.1; q = p^2 = 9 mod 16, c1 = 3), and the 3-isogeny's four polynomials (appendix E.3; ascending, the
    denominators monic, leading 1 not stored).  The one input is tests/golden/bls_h2c_g2.json, checked here for what makes
    these the right constants before they are emitted."""
    p = CURVES[3][1]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "bls_h2c_g2.json")
    with open(path) as f:
        c = json.load(f)["constants"]

    def fe(h):  # hex of c1 || c0
        raw = bytes.fromhex(h)
        assert len(raw) == 96
        v = (int.from_bytes(raw[48:], "big"), int.from_bytes(raw[:48], "big"))
        assert v[0] < p and v[1] < p
        return v

    def mul(a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)

    def add(a, b):
        return ((a[0] + b[0]) % p, (a[1] + b[1]) % p)

    def power(a, e):
        r = (1, 0)
        while e:
            if e & 1:
                r = mul(r, a)
            a = mul(a, a)
            e >>= 1
        return r

    def inv(a):
        n = pow(a[0] * a[0] + a[1] * a[1], -1, p)
        return (a[0] * n % p, -a[1] * n % p)

    def is_square(a):  # by the norm
        n = (a[0] * a[0] + a[1] * a[1]) % p
        return n == 0 or pow(n, (p - 1) // 2, p) == 1

    ia, ib, z, c6, c7 = (fe(c[k]) for k in ("iso_a", "iso_b", "z", "c6", "c7"))
    c3 = int(c["c3"], 16)
    polys = {k: [fe(h) for h in c[k]] for k in ("k1", "k2", "k3", "k4")}
    q = p * p
    assert ia == (0, 240) and ib == (1012, 1012) and z == (p - 2, p - 1)
    assert (q - 1) % 16 == 8, "c1 = 3"
    assert c3 == ((q - 1) // 8 - 1) // 2, "c3"
    assert c6 == power(z, (q - 1) // 8), "c6"
    assert c7 == power(z, ((q - 1) // 8 + 1) // 2), "c7"
    assert not is_square(z), "Z is a square"
    assert [len(polys[k]) for k in ("k1", "k2", "k3", "k4")] == [4, 2, 4, 3], "degrees of the 3-isogeny"

    def ev(co, x, monic):
        acc = (1, 0) if monic else (0, 0)
        for v in reversed(co):
            acc = add(mul(acc, x), v)
        return acc

    rng = random.Random(9380)
    while True:  # one random point of E' lands on the twist y^2 = x^3 + 4(1 + u)
        x = (rng.randrange(p), rng.randrange(p))
        g = add(add(mul(mul(x, x), x), mul(ia, x)), ib)
        if not is_square(g):
            continue
        # a root by the complex method (p = 3 mod 4)
        a1 = power(g, (p - 3) // 4)
        alpha, x0 = mul(mul(a1, a1), g), mul(a1, g)
        y = mul(x0, (0, 1)) if alpha == (p - 1, 0) else mul(power(add((1, 0), alpha), (p - 1) // 2), x0)
        assert mul(y, y) == g
        xd, yd = ev(polys["k2"], x, True), ev(polys["k4"], x, True)
        if xd == (0, 0) or yd == (0, 0):
            continue
        X = mul(ev(polys["k1"], x, False), inv(xd))
        Y = mul(mul(y, ev(polys["k3"], x, False)), inv(yd))
        assert mul(Y, Y) == add(mul(mul(X, X), X), (4, 4)), "the isogeny misses the twist"
        break
    bits, n = 28, 14
    R = 1 << (bits * n)
    mont = lambda v: digits(v * R % p, bits, n)
    out.append("")
    out.append("struct BLS12_381_G2_H2C {  // RFC 9380 8.8.2 / E.3: hashing to G2, working form of BLS12_381U, c0 then c1")
    for name, v in (("A", ia), ("B", ib), ("Z", z), ("C6", c6), ("C7", c7)):
        out.append(arr(name + "0", mont(v[0])))
        out.append(arr(name + "1", mont(v[1])))
    out.append(arr("R2_256", digits((1 << 256) * R * R % p, bits, n)) + "  // 2^256 R^2: a * R2_256 / R = a 2^256 R")
    for k, name in (("k1", "XNUM"), ("k2", "XDEN"), ("k3", "YNUM"), ("k4", "YDEN")):
        out.append(arr2(name + "0", [mont(v[0]) for v in polys[k]]))
        out.append(arr2(name + "1", [mont(v[1]) for v in polys[k]]))
    nw = (c3.bit_length() + 31) // 32
    out.append("  static constexpr int C3_BITS = %d;  // of c3 = ((p^2 - 1) / 8 - 1) / 2" % c3.bit_length())
    out.append("  static constexpr uint32_t C3[%d] = {%s};" % (nw, ", ".join("0x%08xu" % ((c3 >> (32 * i)) & 0xFFFFFFFF) for i in range(nw))))
    out.append("};")


def emit_bls_pairing(out):
    """BLS12_381_PAIRING: what the tower above Fp2 and the final exponentiation need (ufe12.hpp, kernels_pairing.hpp), in
    the working form of BLS12_381U, all derived here from p, the seed and xi = 1 + u.  Fp12 is held in the basis 1, w, ..,
    w^5 over Fp2 (w^6 = xi), so the Frobenius multiplies the conjugated coefficient of w^k by gamma^k with
    gamma = xi^((p - 1) / 6); the Fp6 coefficients xi^((p - 1) / 3) and xi^(2 (p - 1) / 3) are gamma^2 and gamma^4.
    LAMBDA3 = (x - 1)^2 / 3, the one long exponent of the hard part (p^4 - p^2 + 1) / r = lambda3 (p + x)(p^2 + x^2 - 1) + 1."""
    p = CURVES[3][1]
    r = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    x_abs = 0xD201000000010000

    def mul(a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)

    def power(a, e):
        acc = (1, 0)
        while e:
            if e & 1:
                acc = mul(acc, a)
            a = mul(a, a)
            e >>= 1
        return acc

    xi = (1, 1)
    assert (p - 1) % 6 == 0
    gamma = power(xi, (p - 1) // 6)
    g = [(1, 0)]
    for _ in range(5):
        g.append(mul(g[-1], gamma))
    assert mul(g[5], gamma) == power(xi, p - 1)           # gamma^6 = xi^(p-1)
    assert g[2] == power(xi, (p - 1) // 3) and g[4] == power(xi, 2 * (p - 1) // 3)
    assert power(xi, (p * p - 1) // 2) != (1, 0)          # w^2 = v, v^3 = xi defines a field: xi is no square ...
    assert power(xi, (p * p - 1) // 3) != (1, 0)          # ... and no cube in Fp2
    lam3, rem = divmod((x_abs + 1) ** 2, 3)               # x = -x_abs
    assert rem == 0
    assert (p ** 4 - p ** 2 + 1) % r == 0
    assert lam3 * (p - x_abs) * (p * p + x_abs * x_abs - 1) + 1 == (p ** 4 - p ** 2 + 1) // r
    bits, n = 28, 14
    R = 1 << (bits * n)
    mont = lambda v: digits(v * R % p, bits, n)
    out.append("")
    out.append("struct BLS12_381_PAIRING {  // the tower above Fp2 and the final exponentiation, working form of BLS12_381U")
    out.append(arr2("GAMMA0", [mont(g[k][0]) for k in range(6)]) + "  // row k: gamma^k = xi^(k (p-1) / 6), real parts")
    out.append(arr2("GAMMA1", [mont(g[k][1]) for k in range(6)]) + "  // ... imaginary parts; rows 2, 4: the Fp6 coefficients")
    nw = (lam3.bit_length() + 31) // 32
    out.append("  static constexpr int LAMBDA3_BITS = %d;  // of (x - 1)^2 / 3" % lam3.bit_length())
    out.append("  static constexpr uint32_t LAMBDA3[%d] = {%s};" % (nw, ", ".join("0x%08xu" % ((lam3 >> (32 * i)) & 0xFFFFFFFF) for i in range(nw))))
    out.append("};")


def main():
    out = ["// @generated by tools/gen_curve_consts.py -- do not edit.",
           "// Montgomery constants, 32-bit little-endian limbs, R = 2^(32*L).", ""]
    for curve in CURVES:
        emit_sat(out, *curve)
    bb = lambda i: (("CB", CURVES[i][2]), ("CB3", 3 * CURVES[i][2] % CURVES[i][1]))   # curve constant b and 3b
    emit_unsat(out, "P256U", "P256", CURVES[0][1], CURVES[0][3], CURVES[0][4], 29, 9, 0,
               solinas=((224, -1), (192, 1), (96, 1)), extra=bb(0), root_exp=(CURVES[0][1] + 1) // 4)
    emit_unsat(out, "P384U", "P384", CURVES[1][1], CURVES[1][3], CURVES[1][4], 28, 14, 0,
               solinas=((128, -1), (96, -1), (32, 1)), sparse=True, extra=bb(1), root_exp=(CURVES[1][1] + 1) // 4)
    emit_unsat(out, "P521U", "P521", CURVES[2][1], CURVES[2][3], CURVES[2][4], 29, 18, 2, extra=bb(2), root_exp=(CURVES[2][1] + 1) // 4)
    emit_unsat(out, "BLS12_381U", "BLS12_381", CURVES[3][1], CURVES[3][3], CURVES[3][4], 28, 14, 1,
               extra=bb(3) + (("BETA", _bls_beta()),), root_exp=(CURVES[3][1] + 1) // 4)
    # scalar split k = k1 + k2 * x^2 (ECCX_ASSUME_SUBGROUP): x^2 and floor(2^256 / x^2) in 32-bit limbs
    x2 = BLS_X_ABS * BLS_X_ABS
    out.append("struct BLS12_381_GLV {")
    out.append("  static constexpr uint64_t SEED_ABS = 0x%016xull;  // |x|, x the curve's seed (negative)" % BLS_X_ABS)
    out.append(arr("X2", limbs(x2, 4)))
    out.append(arr("MU", limbs((1 << 256) // x2, 5)))
    out.append("  static constexpr int K_BITS = %d;  // bits of the halves: k1 < x^2, k2 <= (2^256 - 1) / x^2" % max(x2.bit_length(), (((1 << 256) - 1) // x2).bit_length()))
    out.append("};")
    out.append("")
    L = 8
    out.append("struct ED25519;")
    emit_unsat(out, "ED25519U", "ED25519", P25519, ED_GX, ED_GY, 29, 9, 3, extra=(("D2", 2 * ED_D % P25519), ("D", ED_D), ("SQRT_M1", pow(2, (P25519 - 1) // 4, P25519))),
               root_exp=(P25519 - 5) // 8)
    out.append("struct ED25519 {")
    out.append("  static constexpr int L = 8;")
    out.append("  static constexpr int FB = 32;")
    out.append("  static constexpr int SB = 32;")
    R = emit_field(out, P25519, L, 0, 1)
    out.append(arr("D2", limbs(2 * ED_D * R % P25519, L)))
    out.append(arr("GX", limbs(ED_GX * R % P25519, L)))
    out.append(arr("GY", limbs(ED_GY * R % P25519, L)))
    out.append("};")
    out.append("")
    # secp256k1: a = 0 and cofactor 1 on a 256-bit prime that is neither -1 mod 2^29 (p = 0x1ffffc2f mod 2^29) nor of
    # the Mersenne kinds -- 9 x 29 limbs, general Montgomery reduction (the field of p256k1)
    k1 = P256K1_CURVE
    emit_sat(out, *k1)
    emit_unsat(out, "P256K1U", "P256K1", k1[1], k1[3], k1[4], 29, 9, 1,
               extra=(("CB", k1[2]), ("CB3", 3 * k1[2] % k1[1]), ("BETA", K1_BETA)), root_exp=(k1[1] + 1) // 4)
    n, g1, g2 = _k1_glv()
    out.append("struct P256K1_GLV {")
    out.append("  static constexpr bool LATTICE = true;  // signed split k = k1 + k2 lambda, sigma(P) = (beta x, y) = [lambda] P")
    out.append(arr("N", limbs(n, 8)))
    out.append(arr("G1", limbs(g1, 8)) + "  // round(2^384 b2 / n)")
    out.append(arr("G2", limbs(g2, 8)) + "  // round(-2^384 b1 / n)")
    out.append(arr("A1", limbs(K1_A1, 5)))
    out.append(arr("B1N", limbs(-K1_B1, 5)) + "  // -b1 (b1 < 0)")
    out.append(arr("A2", limbs(K1_A2, 5)))
    out.append(arr("B2", limbs(K1_B2, 5)))
    out.append("  static constexpr int K_BITS = 128;  // |k1|, |k2| < 2^128 for k < n")
    out.append("};")
    # the scalar fields of the ECDSA curves (kernels_ecdsa.hpp): arithmetic modulo the group order n with fe.hpp's general
    # word-by-word Montgomery product and inv_gcd.hpp's division steps.  FB is the scalar size here, so the byte I/O of
    # fe.hpp moves SB-byte scalars.  The P-521 order is a general 521-bit modulus (not Mersenne): 17 limbs, Montgomery.
    for name in ("P256", "P384", "P521", "P256K1"):
        n = ORDERS[name][0]
        sb = next(c[6] for c in CURVES + [P256K1_CURVE] if c[0] == name)
        L = (n.bit_length() + 31) // 32
        out.append("")
        out.append("struct %s_ORD {  // n, the order of the generator of %s" % (name, name))
        out.append("  static constexpr int L = %d;   // 32-bit limbs" % L)
        out.append("  static constexpr int FB = %d;  // bytes of an element (= SB)" % sb)
        out.append("  static constexpr int SB = %d;  // scalar bytes" % sb)
        out.append("  static constexpr int NBITS = %d;  // qlen: bits2int keeps this many leading bits of a digest" % n.bit_length())
        emit_field(out, n, L)
        out.append("};")
    # the order l of edwards25519's base point (kernels_ed25519_verify.hpp): S < l, SHA-512(R || A || M) mod l.  General
    # Montgomery as above; NBITS is l's bit length (no bits2int here: the wide hash is reduced exactly)
    ell = ED25519_L
    out.append("")
    out.append("struct ED25519_ORD {  // l, the order of the base point of edwards25519")
    out.append("  static constexpr int L = 8;   // 32-bit limbs")
    out.append("  static constexpr int FB = 32;  // bytes of an element (= SB)")
    out.append("  static constexpr int SB = 32;  // scalar bytes")
    out.append("  static constexpr int NBITS = %d;  // bit length of l" % ell.bit_length())
    emit_field(out, ell, 8)
    out.append("};")
    emit_bls_h2c(out)
    emit_bls_g2(out)
    emit_bls_g2_h2c(out)
    emit_bls_pairing(out)
    emit_goldilocks(out)
    emit_jubjub(out)
    sys.stdout.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
