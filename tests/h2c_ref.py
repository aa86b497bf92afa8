"""RFC 9380 hash-to-curve for BLS12-381 G1, written from the RFC's definitions: hashlib, big integers, textbook affine
arithmetic.  The checker of the GPU kernels, not the product; it shares no structure with them (Simplified SWU in the
x1 / x2 form of section 6.6.2 with a Legendre test, the isogeny on affine coordinates with one inversion per fraction).

The suites are BLS12381G1_XMD:SHA-256_SSWU_RO_ (hash_to_curve) and ..._NU_ (encode_to_curve), section 8.8.1.  The
constants of the map (A', B', the appendix E.2 coefficients) are data: tests/golden/bls_h2c.json.
"""
import hashlib
import json
import os

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
H_EFF = 0xD201000000010001  # 1 - x for the curve's seed x = -0xd201000000010000
Z = 11
L = 64  # bytes of uniform randomness per field element: ceil((381 + 128) / 8)

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bls_h2c.json")) as _f:
    FIXTURE = json.load(_f)
_C = FIXTURE["constants"]
ISO_A, ISO_B = int(_C["iso_a"], 16), int(_C["iso_b"], 16)
X_NUM, X_DEN, Y_NUM, Y_DEN = ([int(h, 16) for h in _C[k]] for k in ("x_num", "x_den", "y_num", "y_den"))


def effective_dst(dst: bytes) -> bytes:
    """section 5.3.3: a tag over 255 bytes is hashed down"""
    return hashlib.sha256(b"H2C-OVERSIZE-DST-" + dst).digest() if len(dst) > 255 else dst


def expand_message_xmd(msg: bytes, dst: bytes, len_in_bytes: int) -> bytes:
    """section 5.3.1 with SHA-256"""
    dst = effective_dst(dst)
    ell = (len_in_bytes + 31) // 32
    assert ell <= 255 and len_in_bytes <= 65535
    dst_prime = dst + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + msg + len_in_bytes.to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    b = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        b.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(b)[:len_in_bytes]


def hash_to_field(msg: bytes, dst: bytes, count: int):
    """section 5.2 for m = 1"""
    uniform = expand_message_xmd(msg, dst, count * L)
    return [int.from_bytes(uniform[L * i:L * i + L], "big") % P for i in range(count)]


def sgn0(x: int) -> int:
    return x & 1


def _is_square(x: int) -> bool:
    return x == 0 or pow(x, (P - 1) // 2, P) == 1


def _sqrt(x: int) -> int:
    r = pow(x, (P + 1) // 4, P)
    assert r * r % P == x
    return r


def map_to_curve_sswu(u: int):
    """section 6.6.2 onto E': y^2 = x^3 + A'x + B'"""
    g = lambda x: (x * x * x + ISO_A * x + ISO_B) % P
    tv1 = (Z * Z * pow(u, 4, P) + Z * u * u) % P
    if tv1 == 0:
        x1 = ISO_B * pow(Z * ISO_A, -1, P) % P
    else:
        x1 = (-ISO_B * pow(ISO_A, -1, P)) * (1 + pow(tv1, -1, P)) % P
    if _is_square(g(x1)):
        x, y = x1, _sqrt(g(x1))
    else:
        x = Z * u * u * x1 % P
        y = _sqrt(g(x))
    if sgn0(u) != sgn0(y):
        y = P - y
    return x, y


def _poly(coeffs, x, monic):
    acc = 0
    for i, c in enumerate(coeffs):
        acc += c * pow(x, i, P)
    if monic:
        acc += pow(x, len(coeffs), P)
    return acc % P


def iso_map(pt):
    """appendix E.2; None (the identity) where a denominator vanishes (section 6.6.3)"""
    x, y = pt
    xd, yd = _poly(X_DEN, x, True), _poly(Y_DEN, x, True)
    if xd == 0 or yd == 0:
        return None
    return (_poly(X_NUM, x, False) * pow(xd, -1, P) % P, y * _poly(Y_NUM, x, False) * pow(yd, -1, P) % P)


def map_to_curve(u: int):
    return iso_map(map_to_curve_sswu(u))


def add(a, b):
    """textbook affine addition on y^2 = x^3 + 4; None is the identity"""
    if a is None:
        return b
    if b is None:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def mul(k: int, pt):
    acc = None
    for bit in bin(k)[2:]:
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, pt)
    return acc


def clear_cofactor(pt):
    return mul(H_EFF, pt)


def on_curve(pt) -> bool:
    return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - 4) % P == 0


def finish(us):
    """the point for given field elements: one element is encode_to_curve's tail, two are hash_to_curve's"""
    q = None
    for u in us:
        q = add(q, map_to_curve(u))
    return clear_cofactor(q)


def hash_to_curve(msg: bytes, dst: bytes):
    return finish(hash_to_field(msg, dst, 2))


def encode_to_curve(msg: bytes, dst: bytes):
    return finish(hash_to_field(msg, dst, 1))


def record(pt):
    """(96 bytes x || y big-endian, flag) as the C ABI writes them: zeros and flag 1 for the identity"""
    if pt is None:
        return bytes(96), 1
    return pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big"), 0


def hash_records(msgs, dst: bytes, nonuniform: bool = False):
    fn = encode_to_curve if nonuniform else hash_to_curve
    recs = [record(fn(m, dst)) for m in msgs]
    return b"".join(r[0] for r in recs), bytes(r[1] for r in recs)


def exceptional_u():
    """the two u with Z^2 u^4 + Z u^2 = 0, u != 0: +-sqrt(-1/Z)"""
    r = _sqrt((-pow(Z, -1, P)) % P)
    return r, P - r
