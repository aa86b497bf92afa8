"""The model of BLS AggregateVerify (tests/bls_aggregate_ref.py) against the three Ethereum `sign` vectors of
tests/golden/bls_sig.json and against the models of verify and FastAggregateVerify, and the library's side of
eccx_bls_aggregate_verify / eccx_pairing_groups that needs no device: symbols, constants, argument checks.  CPU only.

The three vectors are signed by ONE key, so swapping two of their messages permutes equal factors and changes nothing: the
swap that must fail is between a vector's pair and a fourth pair under a second key, made by the model."""
import json
import os

import numpy as np

from tests import bls_aggregate_ref as A
from tests import bls_sig_ref as B
from tests.oracle_lib import ROOT

with open(os.path.join(ROOT, "tests", "golden", "bls_sig.json")) as _f:
    GOLDEN = json.load(_f)

SK = int(GOLDEN["sk"], 16)
PK = bytes.fromhex(GOLDEN["pk"])
DST = GOLDEN["dst"].encode()
MSGS = [bytes.fromhex(v["message"]) for v in GOLDEN["sign"]]
SIGS = [bytes.fromhex(v["signature"]) for v in GOLDEN["sign"]]
SK2 = 0x5B1C << 200 | 12345
ERR_ARG = -2


def test_aggregate_of_the_ethereum_vectors():
    agg = B.aggregate_signatures(SIGS)
    assert agg == A.aggregate_signature([SK] * 3, MSGS, DST)
    assert A.aggregate_verify([PK] * 3, MSGS, agg, DST) == A.VALID
    assert A.aggregate_verify([PK] * 3, [MSGS[1], MSGS[0], MSGS[2]], agg, DST) == A.VALID   # one key: the same factors
    assert A.aggregate_verify([PK] * 2, MSGS[:2], agg, DST) == A.INVALID
    assert A.aggregate_verify([PK] * 3, MSGS, agg, B.DST_NUL) == A.INVALID
    # a fourth pair under a second key: two messages swapped across the keys
    pk2, m3 = B.sk_to_pk(SK2), b"a fourth message"
    agg4 = B.aggregate_signatures(SIGS + [B.sign(SK2, m3, DST)])
    pks, msgs = [PK] * 3 + [pk2], MSGS + [m3]
    assert A.aggregate_verify(pks, msgs, agg4, DST) == A.VALID
    assert A.aggregate_verify(pks, [msgs[0], msgs[1], msgs[3], msgs[2]], agg4, DST) == A.INVALID
    # refusals and their order
    inf_key, inf_sig = B.groups()[0].compress(None), B.groups()[1].compress(None)
    assert A.aggregate_verify([PK, inf_key, PK], MSGS, agg, DST) == A.BAD_KEY
    assert A.aggregate_verify([], [], agg, DST) == A.BAD_KEY
    assert A.aggregate_verify([], [], inf_sig, DST) == A.BAD_KEY          # the equation alone would accept it
    broken = bytes([agg[0] & 0x7F]) + agg[1:]
    assert A.aggregate_verify([PK] * 3, MSGS, broken, DST) == A.MALFORMED
    assert A.aggregate_verify([PK, inf_key, PK], MSGS, broken, DST) == A.MALFORMED   # MALFORMED before BAD_KEY
    assert A.distinct(MSGS) and not A.distinct(MSGS + MSGS[:1])


def test_agreement_with_verify_and_fast_aggregate_verify():
    for min_sig in (False, True):
        dst = B.DST_NUL_MIN_SIG if min_sig else B.DST_NUL
        sks = [SK, SK2, 3 * SK % B.R]
        pks = [B.sk_to_pk(s, min_sig) for s in sks]
        msg, other = b"one message", b"another"
        # groups of one are verify
        sig = B.sign(sks[0], msg, dst, min_sig)
        for pk, m in ((pks[0], msg), (pks[0], other), (pks[1], msg)):
            assert A.aggregate_verify([pk], [m], sig, dst, min_sig) == B.verify(pk, m, sig, dst, min_sig)
        # a group with one repeated message is FastAggregateVerify
        agg = B.aggregate_signatures([B.sign(s, msg, dst, min_sig) for s in sks], min_sig)
        for keys in (pks, pks[:2], []):
            assert A.aggregate_verify(keys, [msg] * len(keys), agg, dst, min_sig) == B.fast_aggregate_verify(keys, msg, agg, dst, min_sig)
        assert A.aggregate_verify(pks, [msg] * 3, agg, dst, min_sig) == A.VALID


# ---- the library's side that needs no GPU ------------------------------------------------------------------------------
def test_symbols_and_constants():
    import eccoxide_amd as E
    from eccoxide_amd import _lib
    from eccoxide_amd import engine as EN

    lib = _lib.load()
    for base in ("eccx_bls_aggregate_verify", "eccx_pairing_groups", "eccx_pairing_check_groups"):
        for name in (base, base + "_dev"):
            assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert len(_lib.SYMBOLS[base + "_dev"][1]) == len(_lib.SYMBOLS[base][1]) + 1  # the _dev form takes the stream on top
    k, r = lib.eccx_pairing_group_chunk(), lib.eccx_pairing_group_fanin()
    assert 2 <= k <= 64 and 2 <= r <= 16
    assert EN.PREP_PAIRING_GROUPS == 1 << 16 and EN.PREP_BLS_AGGREGATE == 1 << 17
    for name in ("bls_aggregate_verify", "pairing_groups", "pairing_check_groups"):
        assert callable(getattr(E.Engine, name)) and callable(getattr(E.Engine, name + "_t")), name
    for name in ("pairing_group_chunk", "pairing_group_fanin"):
        assert callable(getattr(E.Engine, name)), name


def test_argument_checks_that_need_no_device():
    from eccoxide_amd import _lib
    from eccoxide_amd import engine as EN

    lib = _lib.load()
    offs = np.array([0, 1], dtype=np.uint64)
    o = offs.ctypes.data
    for opts in (0, EN.BLS_MIN_SIG, EN.VALIDATE_POINTS, 1 << 20):
        assert lib.eccx_bls_aggregate_verify(None, 1, b"m", o, None, 0, bytes(96), bytes(48), o, 1, None, opts) == ERR_ARG
        assert lib.eccx_bls_aggregate_verify_dev(None, 0, None, None, None, 0, None, None, None, 0, None, opts, None) == ERR_ARG
        assert lib.eccx_pairing_groups(None, 1, 1, bytes(96), None, bytes(192), None, o, None, None, opts) == ERR_ARG
        assert lib.eccx_pairing_check_groups_dev(None, 0, 0, None, None, None, None, None, None, opts, None) == ERR_ARG
