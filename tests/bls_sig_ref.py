"""Python model of BLS signatures on BLS12-381 (draft-irtf-cfrg-bls-signature), composed from the models already here:
hashing to G1 and G2 (tests/h2c_ref.py, tests/h2c_g2_ref.py), G2 and its codec (tests/g2_ref.py), the G1 codec and
subgroup test (oracle/ecc_ref.py) and the pairing (tests/pairing_ref.py).  The checker, not the product.

Two variants: min-pk (Ethereum's; the default: 48-byte keys in G1, 96-byte signatures in G2, H(m) = hash_to_g2) and
min-sig (min_sig=True: the groups swapped).  The basic, message-augmentation and proof-of-possession schemes differ only in
the tag and in what the caller puts into the message, so the tag is an argument everywhere.  Verdicts are the library's
ECCX_SIG_* values, with MALFORMED (the signature) before BAD_KEY (the key) before the equation.
"""
import functools

from oracle import ecc_ref as R1
from tests import g2_ref as G2
from tests import h2c_g2_ref as H2
from tests import h2c_ref as H1
from tests import pairing_ref as PR

R = G2.R
G1C = R1.BLS12_381_G1
G1 = (G1C.gx, G1C.gy)
INVALID, VALID, MALFORMED, BAD_KEY = 0, 1, 2, 3

# the standard tags (draft section 4.2); PopProve / PopVerify sign the key's own bytes under the POP tag
DST_NUL = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_"
DST_AUG = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_AUG_"
DST_POP = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
DST_POP_PROOF = b"BLS_POP_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
DST_NUL_MIN_SIG = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_"
DST_AUG_MIN_SIG = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_AUG_"
DST_POP_MIN_SIG = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_POP_"
DST_POP_PROOF_MIN_SIG = b"BLS_POP_BLS12381G1_XMD:SHA-256_SSWU_RO_POP_"

REJECT = G2.REJECT


# ---- the two groups behind one interface: (multiply, add, compress, decode with the subgroup test, hash) --------------
def _g1_decode(b):
    pt, st = R1.ref_point_decompress("bls12_381_g1", b, check_subgroup=True)
    return REJECT if st == R1.CODEC_INVALID else pt  # None for the infinity encoding


class _G1:
    size = 48
    mul = staticmethod(lambda k, p: R1.affine_mul(G1C, k, p))
    add = staticmethod(lambda p, q: R1.affine_add(G1C, p, q))
    compress = staticmethod(lambda p: R1.ref_point_compress("bls12_381_g1", p))
    decode = staticmethod(_g1_decode)
    hash = staticmethod(H1.hash_to_curve)
    gen = G1


class _G2:
    size = 96
    mul = staticmethod(G2.mul)
    add = staticmethod(G2.add)
    compress = staticmethod(G2.compress)
    decode = staticmethod(lambda b: G2.decompress(b, check_subgroup=True))
    hash = staticmethod(H2.hash_to_curve)
    gen = G2.G


def groups(min_sig=False):
    """(the keys' group, the signatures' group)"""
    return (_G2, _G1) if min_sig else (_G1, _G2)


def sk_to_pk(sk: int, min_sig=False):
    """The compressed public key, or None where sk = 0 or sk >= r (ECCX_SIGN_NONE)."""
    if not 0 < sk < R:
        return None
    kg, _ = groups(min_sig)
    return kg.compress(kg.mul(sk, kg.gen))


def sign(sk: int, msg: bytes, dst: bytes, min_sig=False):
    """The compressed signature sk * H(m), or None where sk = 0 or sk >= r."""
    if not 0 < sk < R:
        return None
    _, sg = groups(min_sig)
    return sg.compress(sg.mul(sk, sg.hash(msg, dst)))


@functools.lru_cache(maxsize=None)
def key_validate(pk: bytes, min_sig=False):
    """The key's point, or None where it does not decode, lies outside the subgroup or is the identity."""
    pt = groups(min_sig)[0].decode(pk)
    return None if pt == REJECT or pt is None else pt


def _equation(key_pt, msg, dst, sig_pt, min_sig):
    """e(pk, H(m)) e(-G1, sig) = 1, or for min-sig e(sig, -G2) e(H(m), pk) = 1; an identity term contributes 1"""
    _, sg = groups(min_sig)
    h = sg.hash(msg, dst)
    if min_sig:
        terms = [(sig_pt, G2.neg(G2.G)), (h, key_pt)]
    else:
        terms = [(key_pt, h), (PR.g1_neg(G1), sig_pt)]
    terms = [t for t in terms if t[0] is not None and t[1] is not None]
    return VALID if PR.pairing_product(terms) == PR.ONE12 else INVALID


def verify(pk: bytes, msg: bytes, sig: bytes, dst: bytes, min_sig=False) -> int:
    sig_pt = groups(min_sig)[1].decode(sig)
    if sig_pt == REJECT:
        return MALFORMED
    key_pt = key_validate(pk, min_sig)
    if key_pt is None:
        return BAD_KEY
    return _equation(key_pt, msg, dst, sig_pt, min_sig)  # the identity signature is a legal point: the equation decides


def aggregate(encodings, group):
    """The compressed sum of compressed points of `group` (_G1 or _G2), or None where one does not decode."""
    acc = None
    for e in encodings:
        pt = group.decode(e)
        if pt == REJECT:
            return None
        acc = group.add(acc, pt)
    return group.compress(acc)


def aggregate_signatures(sigs, min_sig=False):
    return aggregate(sigs, groups(min_sig)[1])


def fast_aggregate_verify(pks, msg: bytes, sig: bytes, dst: bytes, min_sig=False) -> int:
    """Every key goes through KeyValidate; the EMPTY group is BAD_KEY (the draft makes n >= 1 a precondition, and the equation
    would accept the identity signature for it); a group whose keys SUM to the identity is not refused: the draft checks
    each key, not the aggregate."""
    kg, sg = groups(min_sig)
    sig_pt = sg.decode(sig)
    if sig_pt == REJECT:
        return MALFORMED
    if not pks:
        return BAD_KEY
    acc = None
    for pk in pks:
        pt = key_validate(pk, min_sig)
        if pt is None:
            return BAD_KEY
        acc = kg.add(acc, pt)
    return _equation(acc, msg, dst, sig_pt, min_sig)


def pop_prove(sk: int, min_sig=False):
    return sign(sk, sk_to_pk(sk, min_sig), DST_POP_PROOF_MIN_SIG if min_sig else DST_POP_PROOF, min_sig)


def pop_verify(pk: bytes, proof: bytes, min_sig=False) -> int:
    return verify(pk, pk, proof, DST_POP_PROOF_MIN_SIG if min_sig else DST_POP_PROOF, min_sig)
