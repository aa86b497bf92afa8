"""Python-integer model of BLS12-381 G2: Fp2 = Fp[u] / (u^2 + 1), the twist E'(Fp2): y^2 = x^3 + 4(1 + u) with its
affine group law (every case), integer-scalar multiplication, the complex-method square root, the zcash encodings
(96 / 192 bytes) with every rejection rule, psi, and subgroup membership by [r]Q = O.

An Fp2 element is a pair (c0, c1) of integers below P; a point is None (infinity) or a pair (x, y) of Fp2 elements.
Bytes are c1 || c0, 48 bytes big-endian each.  Pure Python: what the GPU tests, smoke() and the G2 benchmark compare
against; it needs nothing outside this file.
"""

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SEED_ABS = 0xD201000000010000  # |x|; the seed x is negative
# order of E'(Fp2) = R * H2
H2 = 0x5D543A95414E7F1091D50792876A202CD91DE4547085ABAA68A205B2E5A7DDFA628F1CB4D9E82EF21537E293A6691AE1616EC6E786F0C70CF1C38E31C7238E5

ZERO = (0, 0)
ONE = (1, 0)
B = (4, 4)
B3 = (12, 12)
GX = (0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
      0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E)
GY = (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
      0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE)
G = (GX, GY)


# ---- Fp2 ---------------------------------------------------------------------------------------------------------
def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def f2_conj(a):
    return (a[0], -a[1] % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_sqr(a):
    return ((a[0] + a[1]) * (a[0] - a[1]) % P, 2 * a[0] * a[1] % P)


def f2_mul_fp(a, k):
    return (a[0] * k % P, a[1] * k % P)


def f2_inv(a):
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def f2_pow(a, e):
    r = ONE
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_sqr(a)
        e >>= 1
    return r


def f2_sqrt(a):
    """The complex method (Adj--Rodriguez-Henriquez, algorithm 9) for p = 3 mod 4: a root, or None."""
    a1 = f2_pow(a, (P - 3) // 4)
    alpha = f2_mul(f2_sqr(a1), a)
    x0 = f2_mul(a1, a)
    if alpha == (P - 1, 0):
        root = f2_mul(x0, (0, 1))
    else:
        root = f2_mul(f2_pow(f2_add(ONE, alpha), (P - 1) // 2), x0)
    return root if f2_sqr(root) == a else None


def fp_is_largest(c):
    return c > (P - 1) // 2


def f2_is_largest(a):
    """c1 first, then c0 when c1 = 0: the order of the bytes c1 || c0."""
    return fp_is_largest(a[1]) or (a[1] == 0 and fp_is_largest(a[0]))


def f2_to_bytes(a):
    return a[1].to_bytes(48, "big") + a[0].to_bytes(48, "big")


def f2_from_bytes(b):
    """None unless both components are below p."""
    assert len(b) == 96
    c1, c0 = int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big")
    return (c0, c1) if c0 < P and c1 < P else None


# ---- the twist ---------------------------------------------------------------------------------------------------
def rhs(x):
    return f2_add(f2_mul(f2_sqr(x), x), B)


def on_curve(pt):
    return pt is None or f2_sqr(pt[1]) == rhs(pt[0])


def neg(pt):
    return None if pt is None else (pt[0], f2_neg(pt[1]))


def add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if p[1] != q[1] or p[1] == ZERO:
            return None
        lam = f2_mul(f2_mul_fp(f2_sqr(p[0]), 3), f2_inv(f2_mul_fp(p[1], 2)))
    else:
        lam = f2_mul(f2_sub(q[1], p[1]), f2_inv(f2_sub(q[0], p[0])))
    x3 = f2_sub(f2_sub(f2_sqr(lam), p[0]), q[0])
    return (x3, f2_sub(f2_mul(lam, f2_sub(p[0], x3)), p[1]))


# Jacobian arithmetic for the multiplication (one inversion at the end); None is infinity
def _jdbl(p):
    if p is None:
        return None
    x, y, z = p
    if y == ZERO:
        return None
    a, b = f2_sqr(x), f2_sqr(y)
    c = f2_sqr(b)
    d = f2_mul_fp(f2_sub(f2_sub(f2_sqr(f2_add(x, b)), a), c), 2)
    e = f2_mul_fp(a, 3)
    x3 = f2_sub(f2_sqr(e), f2_mul_fp(d, 2))
    return (x3, f2_sub(f2_mul(e, f2_sub(d, x3)), f2_mul_fp(c, 8)), f2_mul_fp(f2_mul(y, z), 2))


def _jadd_affine(p, q):
    if q is None:
        return p
    if p is None:
        return (q[0], q[1], ONE)
    x1, y1, z1 = p
    zz = f2_sqr(z1)
    u2, s2 = f2_mul(q[0], zz), f2_mul(q[1], f2_mul(zz, z1))
    h, r = f2_sub(u2, x1), f2_sub(s2, y1)
    if h == ZERO:
        return _jdbl(p) if r == ZERO else None
    hh = f2_sqr(h)
    hhh, v = f2_mul(hh, h), f2_mul(x1, hh)
    x3 = f2_sub(f2_sub(f2_sqr(r), hhh), f2_mul_fp(v, 2))
    return (x3, f2_sub(f2_mul(r, f2_sub(v, x3)), f2_mul(y1, hhh)), f2_mul(z1, h))


def _to_affine(p):
    if p is None or p[2] == ZERO:
        return None
    zi = f2_inv(p[2])
    zi2 = f2_sqr(zi)
    return (f2_mul(p[0], zi2), f2_mul(p[1], f2_mul(zi2, zi)))


def mul(k, pt):
    """[k]pt for the integer k >= 0 (not reduced modulo r: off the subgroup that matters)."""
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = _jdbl(acc)
        if bit == "1":
            acc = _jadd_affine(acc, pt)
    return _to_affine(acc)


def in_subgroup(pt):
    return mul(R, pt) is None


# psi(x, y) = (conj(x) * xi^-((p-1)/3), conj(y) * xi^-((p-1)/2)), xi = 1 + u
PSI_X = f2_inv(f2_pow((1, 1), (P - 1) // 3))
PSI_Y = f2_inv(f2_pow((1, 1), (P - 1) // 2))


def psi(pt):
    return None if pt is None else (f2_mul(f2_conj(pt[0]), PSI_X), f2_mul(f2_conj(pt[1]), PSI_Y))


def in_subgroup_psi(pt):
    """psi(Q) = [x]Q = -[|x|]Q."""
    return psi(pt) == neg(mul(SEED_ABS, pt))


def point_of_x(x, largest=False):
    """The point of the twist with this x and the y whose is_largest is `largest`; None if there is none."""
    y = f2_sqrt(rhs(x))
    if y is None:
        return None
    return (x, y if f2_is_largest(y) == largest else f2_neg(y))


def torsion_point(order, seed_x=(1, 2)):
    """A point of this prime order (13 and 23 divide the cofactor twice): [r h2 / order^2] Q for Q at x = seed_x."""
    assert (R * H2) % (order * order) == 0
    q = mul(R * H2 // (order * order), point_of_x(seed_x))
    while q is not None and mul(order, q) is not None:
        q = mul(order, q)
    assert q is not None and mul(order, q) is None
    return q


# ---- records of the C ABI: x || y, 192 bytes, zeros for infinity ---------------------------------------------------
def to_record(pt):
    """(192 bytes, flag): flag 1 and zeros for infinity."""
    if pt is None:
        return bytes(192), 1
    return f2_to_bytes(pt[0]) + f2_to_bytes(pt[1]), 0


def from_record(b):
    return (f2_from_bytes(b[:96]), f2_from_bytes(b[96:]))


# ---- zcash encodings --------------------------------------------------------------------------------------------
def compress(pt):
    if pt is None:
        return bytes([0xC0]) + bytes(95)
    b = bytearray(f2_to_bytes(pt[0]))
    b[0] |= 0x80 | (0x20 if f2_is_largest(pt[1]) else 0)
    return bytes(b)


def uncompressed(pt):
    if pt is None:
        return bytes([0x40]) + bytes(191)
    return f2_to_bytes(pt[0]) + f2_to_bytes(pt[1])


REJECT = "reject"


def decompress(b, check_subgroup=False):
    """A point, None for the infinity encoding, or REJECT."""
    assert len(b) == 96
    f = b[0]
    payload = bytes([f & 0x1F]) + b[1:]
    if not f & 0x80:
        return REJECT
    if f & 0x40:
        return None if not f & 0x20 and not any(payload) else REJECT
    x = f2_from_bytes(payload)
    if x is None:
        return REJECT
    pt = point_of_x(x, bool(f & 0x20))
    if pt is None or (check_subgroup and not in_subgroup(pt)):
        return REJECT
    return pt


def from_uncompressed(b, check_subgroup=False):
    assert len(b) == 192
    f = b[0]
    payload = bytes([f & 0x1F]) + b[1:]
    if f & 0xA0:
        return REJECT
    if f & 0x40:
        return None if not any(payload) else REJECT
    x, y = f2_from_bytes(payload[:96]), f2_from_bytes(payload[96:])
    if x is None or y is None or not on_curve((x, y)) or (check_subgroup and not in_subgroup((x, y))):
        return REJECT
    return (x, y)


def decode_result(res):
    """(192-byte record, flag) as eccx_point_decompress writes it."""
    if res == REJECT:
        return bytes(192), 2
    return to_record(res)
