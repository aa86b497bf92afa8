"""Python-integer model of the BLS12-381 optimal-ate pairing on top of tests/g2_ref.py.

Fp12 is held in the basis 1, w, .., w^5 over Fp2 with w^6 = xi = 1 + u: a tuple of six Fp2 elements.  The tower of
the reference, Fp6 = Fp2[v] / (v^3 - xi) and Fp12 = Fp6[w] / (w^2 - v), is the same field with v = w^2: the Fp6 half c0
is the coefficients of w^0, w^2, w^4 and c1 is those of w^1, w^3, w^5.

Two independent computations of e(P, Q):
  pairing / pairing_product   the optimised shape: twist-side projective Miller loop over |x| with sparse lines, the easy
                              part and the hard part m * y1^(p^2 + x^2 - 1), y = m^lambda3, y1 = y^p * y^x
  pairing_definition          G2 untwisted onto E(Fp12), textbook affine double-and-add with the vertical-line
                              denominators, then a plain square-and-multiply by (p^12 - 1) / r, then conjugated
Bytes of an Fp12 value: 576 = the twelve Fp coefficients from the highest tower coefficient down (Fp12 c1 || c0, each
Fp6 c2 || c1 || c0, each Fp2 c1 || c0), 48 bytes big-endian each.
"""
from oracle import ecc_ref as R1
from tests import g2_ref as G2

P = G2.P
R = G2.R
X_ABS = G2.SEED_ABS
XI = (1, 1)
G1C = R1.BLS12_381_G1
G1 = (G1C.gx, G1C.gy)
LAMBDA3 = (X_ABS + 1) ** 2 // 3  # (x - 1)^2 / 3 for the negative seed x = -X_ABS
assert LAMBDA3 * 3 == (X_ABS + 1) ** 2
assert (P ** 4 - P ** 2 + 1) % R == 0
# the factorisation the hard part walks: exactly (p^4 - p^2 + 1) / r, not its cube
assert LAMBDA3 * (P - X_ABS) * (P * P + X_ABS * X_ABS - 1) + 1 == (P ** 4 - P ** 2 + 1) // R

f2_add, f2_sub, f2_mul, f2_sqr, f2_neg, f2_conj, f2_inv = G2.f2_add, G2.f2_sub, G2.f2_mul, G2.f2_sqr, G2.f2_neg, G2.f2_conj, G2.f2_inv
Z2, O2 = G2.ZERO, G2.ONE


def f2_mul_xi(a):
    return ((a[0] - a[1]) % P, (a[0] + a[1]) % P)


# ---- derived constants ----------------------------------------------------------------------------------------------
GAMMA = G2.f2_pow(XI, (P - 1) // 6)                     # w^(p-1)
GAMMA_POW = [O2]
for _ in range(5):
    GAMMA_POW.append(f2_mul(GAMMA_POW[-1], GAMMA))       # gamma^k: the Frobenius coefficient of w^k
FP6_C1 = G2.f2_pow(XI, (P - 1) // 3)                    # v^(p-1)   = gamma^2
FP6_C2 = G2.f2_pow(XI, 2 * (P - 1) // 3)                # v^(2(p-1)) = gamma^4

# ---- polynomials in w (degree < D) modulo w^D = xi^(6/D): D = 6 is Fp12, D = 3 with w standing for v is Fp6 -------
ZERO12 = (Z2,) * 6
ONE12 = (O2,) + (Z2,) * 5


def poly_mul(a, b):
    d = len(a)
    lo, hi = [Z2] * d, [Z2] * d
    for i in range(d):
        if a[i] == Z2:
            continue
        for j in range(d):
            if b[j] == Z2:
                continue
            t = f2_mul(a[i], b[j])
            if i + j < d:
                lo[i + j] = f2_add(lo[i + j], t)
            else:
                hi[i + j - d] = f2_add(hi[i + j - d], t)
    return tuple(f2_add(l, f2_mul_xi(h)) for l, h in zip(lo, hi))


def poly_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def poly_sub(a, b):
    return tuple(f2_sub(x, y) for x, y in zip(a, b))


def poly_neg(a):
    return tuple(f2_neg(x) for x in a)


f12_mul = poly_mul
f6_mul = poly_mul


def f12_sqr(a):
    return poly_mul(a, a)


def f6_sqr(a):
    return poly_mul(a, a)


def f6_mul_by_v(a):
    """multiplication by the non-residue of Fp12 over Fp6"""
    return (f2_mul_xi(a[2]), a[0], a[1])


def f6_mul_by_01(a, c0, c1):
    return poly_mul(a, (c0, c1, Z2))


def f6_mul_by_1(a, c1):
    return poly_mul(a, (Z2, c1, Z2))


def f6_frobenius(a):
    return (f2_conj(a[0]), f2_mul(f2_conj(a[1]), FP6_C1), f2_mul(f2_conj(a[2]), FP6_C2))


def f6_inv(a):
    c0, c1, c2 = a
    t0 = f2_sub(f2_sqr(c0), f2_mul_xi(f2_mul(c1, c2)))
    t1 = f2_sub(f2_mul_xi(f2_sqr(c2)), f2_mul(c0, c1))
    t2 = f2_sub(f2_sqr(c1), f2_mul(c0, c2))
    n = f2_add(f2_mul(c0, t0), f2_mul_xi(f2_add(f2_mul(c2, t1), f2_mul(c1, t2))))
    ni = f2_inv(n)
    return (f2_mul(t0, ni), f2_mul(t1, ni), f2_mul(t2, ni))


def f12_halves(a):
    return (a[0], a[2], a[4]), (a[1], a[3], a[5])


def f12_of_halves(c0, c1):
    return (c0[0], c1[0], c0[1], c1[1], c0[2], c1[2])


def f12_conj(a):
    return tuple(f2_neg(c) if k & 1 else c for k, c in enumerate(a))


def f12_inv(a):
    c0, c1 = f12_halves(a)
    d = f6_inv(poly_sub(f6_sqr(c0), f6_mul_by_v(f6_sqr(c1))))
    return f12_of_halves(f6_mul(c0, d), poly_neg(f6_mul(c1, d)))


def f12_frobenius(a):
    return tuple(f2_mul(f2_conj(c), GAMMA_POW[k]) for k, c in enumerate(a))


def f12_mul_by_014(a, c0, c1, c4):
    """by c0 + c1 v + c4 v w: the coefficients of w^0, w^2 and w^3"""
    return poly_mul(a, (c0, Z2, c1, c4, Z2, Z2))


def f12_pow(a, e):
    r = ONE12
    for bit in bin(e)[2:] if e else "":
        r = f12_sqr(r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def _fp4_sqr(a, b):
    """(a + b s)^2 in Fp4 = Fp2[s] / (s^2 - xi)"""
    t0, t1 = f2_sqr(a), f2_sqr(b)
    return f2_add(f2_mul_xi(t1), t0), f2_sub(f2_sub(f2_sqr(f2_add(a, b)), t0), t1)


def f12_cyclotomic_sqr(a):
    """Granger-Scott squaring, valid where a^(p^6 + 1) = 1.  With s = w^3 (s^2 = xi) the element is
    (a0 + a3 s) + (a4 + a1 s) w^4 ... grouped as three Fp4 values: A = (a0, a3), B = (a1, a4), C = (a2, a5)."""
    a0, a1, a2, a3, a4, a5 = a
    t00, t01 = _fp4_sqr(a0, a3)   # A^2
    t10, t11 = _fp4_sqr(a1, a4)   # B^2
    t20, t21 = _fp4_sqr(a2, a5)   # C^2
    three = lambda t, z: f2_add(f2_add(f2_sub(t, z), f2_sub(t, z)), t)    # 3t - 2z
    threep = lambda t, z: f2_add(f2_add(f2_add(t, z), f2_add(t, z)), t)   # 3t + 2z
    return (three(t00, a0), threep(f2_mul_xi(t21), a1), three(t10, a2),
            threep(t01, a3), three(t20, a4), threep(t11, a5))


def f12_to_bytes(a):
    return b"".join(G2.f2_to_bytes(a[k]) for k in (5, 3, 1, 4, 2, 0))


def f12_from_bytes(b):
    c = [G2.f2_from_bytes(b[96 * i:96 * i + 96]) for i in range(6)]
    return (c[5], c[2], c[4], c[1], c[3], c[0])


ONE_BYTES = f12_to_bytes(ONE12)


# ---- (a) the optimised shape ------------------------------------------------------------------------------------------
def doubling_step(t):
    """t -> 2t on the twist, homogeneous (uniformly scaled by 4), and the tangent's coefficients (c0, c1, c4):
    l = c0 + (c1 xP) v + (c4 yP) v w"""
    x, y, z = t
    yy, zz = f2_sqr(y), f2_sqr(z)
    e = f2_mul(G2.B3, zz)
    f = f2_add(f2_add(e, e), e)
    h = f2_sub(f2_sqr(f2_add(y, z)), f2_add(yy, zz))           # 2YZ
    xy2 = f2_mul(f2_add(x, x), y)
    ee = f2_sqr(e)
    ee12 = G2.f2_mul_fp(ee, 12)
    yy4 = G2.f2_mul_fp(yy, 4)
    xx = f2_sqr(x)
    t3 = (f2_mul(xy2, f2_sub(yy, f)), f2_sub(f2_sqr(f2_add(yy, f)), ee12), f2_mul(yy4, h))
    return t3, (f2_sub(e, yy), G2.f2_mul_fp(xx, 3), f2_neg(h))


def addition_step(t, q):
    """t -> t + q (q affine, != +-t) and the chord's coefficients"""
    x, y, z = t
    qx, qy = q
    th = f2_sub(y, f2_mul(qy, z))
    la = f2_sub(x, f2_mul(qx, z))
    ll = f2_sqr(la)
    lll = f2_mul(la, ll)
    xll = f2_mul(x, ll)
    h = f2_sub(f2_add(lll, f2_mul(z, f2_sqr(th))), f2_add(xll, xll))
    t3 = (f2_mul(la, h), f2_sub(f2_mul(th, f2_sub(xll, h)), f2_mul(lll, y)), f2_mul(z, lll))
    return t3, (f2_sub(f2_mul(th, qx), f2_mul(la, qy)), f2_neg(th), la)


def _ell(f, c, p):
    return f12_mul_by_014(f, c[0], G2.f2_mul_fp(c[1], p[0]), G2.f2_mul_fp(c[2], p[1]))


def miller_product(terms):
    """terms: (P, Q) affine pairs, None for infinity on either side (the term contributes 1)"""
    terms = [(p, q) for p, q in terms if p is not None and q is not None]
    if not terms:
        return ONE12
    f = ONE12
    ts = [(q[0], q[1], O2) for _, q in terms]
    for i in range(62, -1, -1):
        f = f12_sqr(f)
        for j, (p, q) in enumerate(terms):
            ts[j], c = doubling_step(ts[j])
            f = _ell(f, c, p)
            if (X_ABS >> i) & 1:
                ts[j], c = addition_step(ts[j], q)
                f = _ell(f, c, p)
    return f12_conj(f)


def cyclotomic_pow(a, e):
    acc = a
    for bit in bin(e)[3:]:
        acc = f12_cyclotomic_sqr(acc)
        if bit == "1":
            acc = f12_mul(acc, a)
    return acc


def exp_by_x(a):
    return f12_conj(cyclotomic_pow(a, X_ABS))


def easy_part(f):
    t = f12_mul(f12_conj(f), f12_inv(f))
    return f12_mul(f12_frobenius(f12_frobenius(t)), t)


def hard_part(m):
    y = cyclotomic_pow(m, LAMBDA3)
    y1 = f12_mul(f12_frobenius(y), exp_by_x(y))
    y2 = f12_mul(f12_mul(f12_frobenius(f12_frobenius(y1)), exp_by_x(exp_by_x(y1))), f12_conj(y1))
    return f12_mul(m, y2)


def final_exponentiation(f):
    return hard_part(easy_part(f))


def pairing_product(terms):
    return final_exponentiation(miller_product(terms))


def pairing(p, q):
    return pairing_product([(p, q)])


# ---- (b) the definition ---------------------------------------------------------------------------------------------
FINAL_EXP = (P ** 12 - 1) // R
assert FINAL_EXP * R == P ** 12 - 1


def _embed2(a):
    return (a,) + (Z2,) * 5


def pairing_definition(p, q):
    w = (Z2, O2, Z2, Z2, Z2, Z2)
    w2 = f12_sqr(w)
    w3 = f12_mul(w2, w)
    px, py = _embed2((p[0], 0)), _embed2((p[1], 0))
    qx, qy = f12_mul(_embed2(q[0]), f12_inv(w2)), f12_mul(_embed2(q[1]), f12_inv(w3))
    num, den = ONE12, ONE12
    tx, ty = qx, qy

    def step(lam, x2):
        x3 = poly_sub(poly_sub(f12_sqr(lam), tx), x2)
        y3 = poly_sub(f12_mul(lam, poly_sub(tx, x3)), ty)
        line = poly_sub(poly_sub(py, ty), f12_mul(lam, poly_sub(px, tx)))
        return x3, y3, line, poly_sub(px, x3)

    for i in range(62, -1, -1):
        xx = f12_sqr(tx)
        lam = f12_mul(poly_add(poly_add(xx, xx), xx), f12_inv(poly_add(ty, ty)))
        tx, ty, line, vert = step(lam, tx)
        num, den = f12_mul(f12_sqr(num), line), f12_mul(f12_sqr(den), vert)
        if (X_ABS >> i) & 1:
            lam = f12_mul(poly_sub(ty, qy), f12_inv(poly_sub(tx, qx)))
            tx, ty, line, vert = step(lam, qx)
            num, den = f12_mul(num, line), f12_mul(den, vert)
    return f12_conj(f12_pow(f12_mul(num, f12_inv(den)), FINAL_EXP))


# ---- points and records ------------------------------------------------------------------------------------------------
def g1_mul(k):
    return R1.affine_mul(G1C, k % R, G1)


def g1_neg(p):
    return None if p is None else (p[0], -p[1] % P)


def g2_mul(k):
    return G2.mul(k % R, G2.G)


def g1_record(p):
    """(96 bytes x || y, flag) as the G1 entry points write them"""
    if p is None:
        return bytes(96), 1
    return p[0].to_bytes(48, "big") + p[1].to_bytes(48, "big"), 0


def term_records(terms):
    """(g1 bytes, g1 flags, g2 bytes, g2 flags) of a list of (P, Q)"""
    a = [g1_record(p) for p, _ in terms]
    b = [G2.to_record(q) for _, q in terms]
    return b"".join(x[0] for x in a), bytes(x[1] for x in a), b"".join(x[0] for x in b), bytes(x[1] for x in b)
