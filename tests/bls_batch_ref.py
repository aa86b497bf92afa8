"""Python model of BLS batch verification by a random linear combination, on tests/bls_sig_ref.py, tests/g2_ref.py and
tests/pairing_ref.py.  The checker, not the product.

    min-pk:   e(-G1, sum c_i sig_i) * prod e(c_i pk_i, H(m_i)) = 1
    min-sig:  e(sum c_i sig_i, -G2) * prod e(c_i H(m_i), pk_i) = 1          c_i: 64-bit coefficients, nonzero

Three ways to the same verdict, from the most literal to the cheapest:
  equation()          the pairing product of L + 1 terms as written above;
  shortcut()          for keys with known secrets: both groups have prime order r and the pairing is non-degenerate, so the
                      product is 1 iff sum c_i sig_i = sum c_i sk_i H(m_i) in the signatures' group;
  shortcut_honest()   the same identity with sk_i H(m_i) given as a point (the honest signature of member i's key on member
                      i's message): members whose signature IS the honest one cancel, so the sum runs over the others.
Expected verdicts of the GPU tests come from verdict() below, never from which members a test tampered with.
"""
from tests import bls_sig_ref as B
from tests import g2_ref as G2
from tests import pairing_ref as PR

R = B.R
INVALID, VALID, MALFORMED, BAD_KEY = B.INVALID, B.VALID, B.MALFORMED, B.BAD_KEY
REJECT = B.REJECT


def _g1_neg(p):
    return PR.g1_neg(p)


def neg(group, p):
    return G2.neg(p) if group is B._G2 else _g1_neg(p)


def scalarmul_u64(group, c: int, p):
    """[c]P for a 64-bit coefficient on group (B._G1 or B._G2): the integer multiple, whatever the point's order."""
    assert 0 <= c < 1 << 64
    return group.mul(c, p) if c and p is not None else None


def coeff(cb: bytes) -> int:
    assert len(cb) == 8
    return int.from_bytes(cb, "big")


def linear_combination(group, coeffs, points):
    acc = None
    for c, p in zip(coeffs, points):
        acc = group.add(acc, scalarmul_u64(group, c, p))
    return acc


def equation(key_pts, msgs, sig_pts, coeffs, dst, min_sig=False) -> int:
    """The literal product of L + 1 terms; an identity term contributes 1.  The empty batch is VALID."""
    kg, sg = B.groups(min_sig)
    agg = linear_combination(sg, coeffs, sig_pts)
    hs = [sg.hash(m, dst) for m in msgs]
    if min_sig:
        terms = [(agg, G2.neg(G2.G))] + [(scalarmul_u64(sg, c, h), k) for c, h, k in zip(coeffs, hs, key_pts)]
    else:
        terms = [(_g1_neg(B.G1), agg)] + [(scalarmul_u64(kg, c, k), h) for c, h, k in zip(coeffs, hs, key_pts)]
    assert len(terms) == len(msgs) + 1
    terms = [t for t in terms if t[0] is not None and t[1] is not None]
    return VALID if PR.pairing_product(terms) == PR.ONE12 else INVALID


def shortcut(sks, msgs, sig_pts, coeffs, dst, min_sig=False) -> int:
    """sum c_i sig_i = sum c_i sk_i H(m_i), for keys pk_i = sk_i G with known secrets."""
    _, sg = B.groups(min_sig)
    want = linear_combination(sg, coeffs, [sg.mul(sk % R, sg.hash(m, dst)) for sk, m in zip(sks, msgs)])
    return VALID if linear_combination(sg, coeffs, sig_pts) == want else INVALID


def shortcut_honest(sigs, honest, coeffs, min_sig=False) -> int:
    """The same with the compressed honest signatures sk_i H(m_i) given: sum over the members whose bytes differ of
    c_i (sig_i - honest_i) is the identity.  (A compressed encoding names one point, so equal bytes cancel.)"""
    _, sg = B.groups(min_sig)
    acc = None
    for s, h, c in zip(sigs, honest, coeffs):
        if s != h:
            diff = sg.add(sg.decode(s), neg(sg, sg.decode(h)))
            acc = sg.add(acc, scalarmul_u64(sg, c, diff))
    return VALID if acc is None else INVALID


def member_status(pk: bytes, sig: bytes, cb: bytes, min_sig=False, honest=None, bad_offsets=False) -> int:
    """What decoding finds about one member: MALFORMED (the signature, the message offsets, a zero coefficient) before
    BAD_KEY, else VALID, which says nothing of the equation.  A signature equal to the honest one is a point of the subgroup."""
    if bad_offsets or coeff(cb) == 0:
        return MALFORMED
    if sig != honest and B.groups(min_sig)[1].decode(sig) == REJECT:
        return MALFORMED
    return BAD_KEY if B.key_validate(pk, min_sig) is None else VALID


def verdict(pks, sigs, coeff_bytes, honest, min_sig=False, bad_offsets=()) -> int:
    """One batch: MALFORMED before BAD_KEY before the equation (by shortcut_honest).  honest[i] is the compressed signature
    of member i's key on member i's message.  The empty batch is VALID."""
    st = [member_status(pk, s, cb, min_sig, h, i in bad_offsets) for i, (pk, s, cb, h) in enumerate(zip(pks, sigs, coeff_bytes, honest))]
    if MALFORMED in st:
        return MALFORMED
    if BAD_KEY in st:
        return BAD_KEY
    return shortcut_honest(sigs, honest, [coeff(cb) for cb in coeff_bytes], min_sig)


def g1_record(p):
    return PR.g1_record(p)


def record(group, p):
    """(x || y bytes, flag) as the C ABI writes them for group"""
    return G2.to_record(p) if group is B._G2 else PR.g1_record(p)
