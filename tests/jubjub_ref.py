"""An independent big-integer model of Jubjub for the tests: the twisted Edwards curve -x^2 + y^2 = 1 + d x^2 y^2,
d = -10240/10241, over the BLS12-381 scalar field Fr.  Nothing here is shared with the engine or its generator.

  * the affine law and an extended-coordinate multiplier (one inversion per result, batched: 1 500 units in seconds);
  * the reference's scale_bytes / double / add sequence (src/curve/jubjub/mod.rs:115-176) value for value, for `proj`;
  * the comb table (j + 1) * 16^i * G of src/params/comb/jubjub.rs;
  * the packed wire format (y little-endian, bit 7 of byte 31 = x mod 2) with its three rejections;
  * Tonelli-Shanks in the fixed shape the device uses, and the textbook one to check it against.
"""
import hashlib

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R = 0x0E7DB4EA6533AFA906673B0101343B00A6682093CCC81082D0970E5ED6F72CB7
D = (-10240 * pow(10241, -1, Q)) % Q
GX = 0x5183972AF8EFF38CA624B4DF00384882000C546BF2F39EDE7F4ECF1A74F976C4
GY = 0x3B43F8472CA2FC2C9E8FCC5ABD9DC308096C8707FFA6833B146BAD709349702E
G = (GX, GY)
NEUTRAL = (0, 1)
TS_S = 32
TS_T = (Q - 1) >> TS_S
TS_Z = pow(5, TS_T, Q)  # a root of unity of order 2^32 (5 is a non-residue)


def on_curve(P):
    x, y = P
    return (y * y - x * x - 1 - D * x * x % Q * y * y) % Q == 0


def add(P, S):
    """The affine law; complete on the whole curve (d is a non-square, -1 a square)."""
    (x1, y1), (x2, y2) = P, S
    k = D * x1 * x2 % Q * y1 * y2 % Q
    return ((x1 * y2 + y1 * x2) * pow(1 + k, -1, Q) % Q, (y1 * y2 + x1 * x2) * pow(1 - k, -1, Q) % Q)


def neg(P):
    return (-P[0] % Q, P[1])


# ---- extended coordinates (X : Y : Z : T), the formulas of mod.rs:115-149 on plain residues ----------------------
def ext(P):
    return (P[0], P[1], 1, P[0] * P[1] % Q)


def ext_double(p):
    x, y, z, _ = p
    a, b, c = x * x % Q, y * y % Q, 2 * z * z % Q
    d = -a % Q
    e = ((x + y) * (x + y) - (a + b)) % Q
    g = (d + b) % Q
    f = (g - c) % Q
    h = (d - b) % Q
    return (e * f % Q, g * h % Q, f * g % Q, e * h % Q)


def ext_add(p, s):
    aa = (p[1] - p[0]) * (s[1] - s[0]) % Q
    bb = (p[1] + p[0]) * (s[1] + s[0]) % Q
    cc = 2 * D * p[3] % Q * s[3] % Q
    dd = 2 * p[2] * s[2] % Q
    e, f, g, h = (bb - aa) % Q, (dd - cc) % Q, (dd + cc) % Q, (bb + aa) % Q
    return (e * f % Q, g * h % Q, f * g % Q, e * h % Q)


def scale_bytes_ext(P, k_be):
    """Point::scale_bytes (mod.rs:165-176): per bit, MSB first, double, add, keep the sum where the bit is set.  Returns
    the un-normalised (X, Y, Z, T) -- what ECCX_MIRROR_REFERENCE writes into `proj`."""
    p, q = ext(P), (0, 1, 1, 0)
    for byte in k_be:
        for i in range(7, -1, -1):
            q = ext_double(q)
            if (byte >> i) & 1:
                q = ext_add(q, p)
    return q


def batch_affine(pts):
    """(X, Y, Z, T) -> (x, y) for a list, one inversion (Montgomery's trick).  Z is never zero on this curve."""
    pre, acc = [], 1
    for p in pts:
        acc = acc * p[2] % Q
        pre.append(acc)
    inv = pow(acc, -1, Q)
    out = [None] * len(pts)
    for i in range(len(pts) - 1, -1, -1):
        zi = inv * (pre[i - 1] if i else 1) % Q
        inv = inv * pts[i][2] % Q
        out[i] = (pts[i][0] * zi % Q, pts[i][1] * zi % Q)
    return out


def mul_ext(P, k):
    """k * P in extended coordinates, any integer k >= 0."""
    p, q = ext(P), (0, 1, 1, 0)
    for bit in bin(k)[2:] if k else "":
        q = ext_double(q)
        if bit == "1":
            q = ext_add(q, p)
    return q


def mul(P, k):
    return batch_affine([mul_ext(P, k)])[0]


def mul_many(points, scalars):
    return batch_affine([mul_ext(P, k) for P, k in zip(points, scalars)])


def double_mul_many(u1s, u2s, points, subtract=False):
    """[u1] G + [u2] Q, or [u1] G - [u2] Q."""
    out = []
    for u1, u2, P in zip(u1s, u2s, points):
        b = mul_ext(P, u2)
        if subtract:
            b = (-b[0] % Q, b[1], b[2], -b[3] % Q)
        out.append(ext_add(mul_ext(G, u1), b))
    return batch_affine(out)


def comb_table():
    """The whole table of src/params/comb/jubjub.rs, 64 windows x 15 entries (j + 1) * 16^i * G, as affine pairs."""
    rows, base = [], ext(G)
    for _ in range(64):
        acc = base
        for j in range(15):
            rows.append(acc)
            acc = ext_add(acc, base)
        base = acc  # 16 * base
    return batch_affine(rows)


def comb_table_bytes():
    return b"".join(x.to_bytes(32, "big") + y.to_bytes(32, "big") for x, y in comb_table())


def comb_table_sha256():
    return hashlib.sha256(comb_table_bytes()).hexdigest()


# ---- square roots ----------------------------------------------------------------------------------------------
def sqrt_fixed(a):
    """Tonelli-Shanks in the device's fixed shape: every step runs whatever a is; returns a root candidate (0 for 0)."""
    w = pow(a, (TS_T - 1) // 2, Q)
    x = a * w % Q
    b = x * w % Q
    z = TS_Z
    for i in range(TS_S, 1, -1):
        need = pow(b, 1 << (i - 2), Q) != 1
        xz = x * z % Q
        z = z * z % Q
        bz = b * z % Q
        if need:
            x, b = xz, bz
    return x


def sqrt(a):
    """A square root of a, or None: the fixed-shape candidate, checked."""
    a %= Q
    x = sqrt_fixed(a)
    return x if x * x % Q == a else None


def is_square(a):
    a %= Q
    return a == 0 or pow(a, (Q - 1) // 2, Q) == 1


# ---- wire format -----------------------------------------------------------------------------------------------
def compress(P):
    x, y = P
    b = bytearray(y.to_bytes(32, "little"))
    b[31] |= (x & 1) << 7
    return bytes(b)


def decompress(enc):
    """The point, or None for the three rejections: y >= q, (y^2 - 1) / (d y^2 + 1) not a square, x = 0 with the sign
    bit set."""
    assert len(enc) == 32
    sign = enc[31] >> 7
    y = int.from_bytes(enc, "little") & ((1 << 255) - 1)
    if y >= Q:
        return None
    u, v = (y * y - 1) % Q, (D * y * y + 1) % Q
    assert v != 0  # -1/d is a non-square
    x = sqrt(u * pow(v, -1, Q) % Q)
    if x is None:
        return None
    if x == 0 and sign:
        return None
    if (x & 1) != sign:
        x = Q - x
    return (x, y)


def point_bytes(P):
    return P[0].to_bytes(32, "big") + P[1].to_bytes(32, "big")


def random_point(rng):
    """A uniformly chosen y with a point above it, sign at random: any point of the curve (order dividing 8 r)."""
    while True:
        enc = bytearray(rng.randrange(Q).to_bytes(32, "little"))
        enc[31] |= rng.randrange(2) << 7
        P = decompress(bytes(enc))
        if P is not None:
            return P


def small_order_points(rng):
    """Points of order exactly 2, 4 and 8, made by clearing r from random points: (0, -1), then one of order 4 and one
    of order 8."""
    found = {}
    while len(found) < 3:
        T = mul(random_point(rng), R)
        order, S = 1, T
        while S != NEUTRAL:
            S = add(S, S)
            order *= 2
        if order in (2, 4, 8):
            found.setdefault(order, T)
    assert found[2] == (0, Q - 1)
    return found
