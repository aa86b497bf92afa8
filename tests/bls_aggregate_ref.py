"""Python model of BLS AggregateVerify (draft-irtf-cfrg-bls-signature, CoreAggregateVerify), composed from the model of
the scheme (tests/bls_sig_ref.py) and the pairing (tests/pairing_ref.py).  The checker, not the product.

One aggregate signature against k (key, message) pairs: e(sig, -G) prod_j e(pk_j, H(m_j)) = 1.  Verdicts are the
library's ECCX_SIG_* values: MALFORMED (the signature) before BAD_KEY (any key fails KeyValidate; the EMPTY group, which the
draft makes a precondition) before the equation.  Distinctness of the messages is NOT checked here: that is the basic
scheme's own rule, `distinct` below.
"""
import functools

from tests import bls_sig_ref as B
from tests import g2_ref as G2
from tests import pairing_ref as PR

INVALID, VALID, MALFORMED, BAD_KEY = B.INVALID, B.VALID, B.MALFORMED, B.BAD_KEY


@functools.lru_cache(maxsize=None)
def hash_point(msg: bytes, dst: bytes, min_sig=False):
    """H(m) in the signatures' group"""
    return B.groups(min_sig)[1].hash(msg, dst)


def aggregate_verify(pks, msgs, sig: bytes, dst: bytes, min_sig=False) -> int:
    if len(pks) != len(msgs):
        raise ValueError("one key per message")
    _, sg = B.groups(min_sig)
    sig_pt = sg.decode(sig)
    if sig_pt == B.REJECT:
        return MALFORMED
    if not pks:
        return BAD_KEY
    key_pts = [B.key_validate(bytes(pk), min_sig) for pk in pks]
    if any(pt is None for pt in key_pts):
        return BAD_KEY
    hs = [hash_point(bytes(m), bytes(dst), min_sig) for m in msgs]
    if min_sig:
        terms = [(sig_pt, G2.neg(G2.G))] + [(h, k) for k, h in zip(key_pts, hs)]
    else:
        terms = [(k, h) for k, h in zip(key_pts, hs)] + [(PR.g1_neg(B.G1), sig_pt)]
    terms = [t for t in terms if t[0] is not None and t[1] is not None]  # an identity term contributes 1
    return VALID if PR.pairing_product(terms) == PR.ONE12 else INVALID


def distinct(msgs) -> bool:
    """the basic scheme's precondition: the messages of one unit are pairwise distinct"""
    return len({bytes(m) for m in msgs}) == len(msgs)


def aggregate_signature(sks, msgs, dst: bytes, min_sig=False) -> bytes:
    """The compressed sum of sk_j * H(m_j), without a decoder in between"""
    _, sg = B.groups(min_sig)
    acc = None
    for sk, m in zip(sks, msgs):
        acc = sg.add(acc, sg.mul(sk, hash_point(bytes(m), bytes(dst), min_sig)))
    return sg.compress(acc)
