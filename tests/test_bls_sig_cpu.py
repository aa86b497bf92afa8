"""The model of BLS signatures (tests/bls_sig_ref.py) against three Ethereum consensus-spec `sign` vectors
(tests/golden/bls_sig.json) and against itself, both variants: keys, signatures, verification's verdict order,
aggregation, FastAggregateVerify on the empty group and on a group that sums to zero, proof of possession.  CPU only.
A model signature costs about 25 ms and a two-term pairing product about 50 ms: the distinct cases are computed once."""
import json
import os

import pytest

from tests import bls_sig_ref as B
from tests import g2_ref as G2
from tests import msm_ref as M
from tests.oracle_lib import ROOT

with open(os.path.join(ROOT, "tests", "golden", "bls_sig.json")) as _f:
    GOLDEN = json.load(_f)

SK = int(GOLDEN["sk"], 16)
DST = GOLDEN["dst"].encode()


def test_ethereum_sign_vectors():
    assert DST == B.DST_POP
    pk = B.sk_to_pk(SK)
    assert pk.hex() == GOLDEN["pk"]
    for v in GOLDEN["sign"]:
        msg = bytes.fromhex(v["message"])
        assert len(msg) == 32
        sig = B.sign(SK, msg, DST)
        assert sig.hex() == v["signature"] and len(sig) == 96
    # the first vector verifies, and under another message, key or tag it does not
    msg, sig = bytes.fromhex(GOLDEN["sign"][0]["message"]), bytes.fromhex(GOLDEN["sign"][0]["signature"])
    assert B.verify(pk, msg, sig, DST) == B.VALID
    assert B.verify(pk, msg[:-1] + b"\x57", sig, DST) == B.INVALID
    assert B.verify(B.sk_to_pk(SK + 1), msg, sig, DST) == B.INVALID
    assert B.verify(pk, msg, sig, B.DST_NUL) == B.INVALID


@pytest.fixture(scope="module", params=[False, True], ids=["min_pk", "min_sig"])
def signed(request):
    """(min_sig, tag, sk, pk, message, signature) of one honest unit"""
    min_sig = request.param
    dst = B.DST_NUL_MIN_SIG if min_sig else B.DST_NUL
    sk, msg = 0x1234567890ABCDEF << 100 | 77, b"the model against itself"
    return min_sig, dst, sk, B.sk_to_pk(sk, min_sig), msg, B.sign(sk, msg, dst, min_sig)


def test_sizes_and_secret_range(signed):
    min_sig, dst, sk, pk, msg, sig = signed
    assert (len(pk), len(sig)) == ((96, 48) if min_sig else (48, 96))
    for bad in (0, B.R, B.R + 5, (1 << 256) - 1):
        assert B.sk_to_pk(bad, min_sig) is None and B.sign(bad, msg, dst, min_sig) is None
    assert B.sk_to_pk(B.R - 1, min_sig) is not None


def test_verdicts_and_their_order(signed):
    min_sig, dst, sk, pk, msg, sig = signed
    kg, sg = B.groups(min_sig)
    assert B.verify(pk, msg, sig, dst, min_sig) == B.VALID
    assert B.verify(pk, msg + b"!", sig, dst, min_sig) == B.INVALID
    bad_sig = bytes([sig[0] & 0x7F]) + sig[1:]            # the compression bit cleared
    inf_key, inf_sig = kg.compress(None), sg.compress(None)
    assert B.verify(pk, msg, bad_sig, dst, min_sig) == B.MALFORMED
    assert B.verify(inf_key, msg, sig, dst, min_sig) == B.BAD_KEY          # KeyValidate: the identity is no key
    assert B.verify(inf_key, msg, bad_sig, dst, min_sig) == B.MALFORMED    # MALFORMED before BAD_KEY
    assert B.verify(pk, msg, inf_sig, dst, min_sig) == B.INVALID           # the identity signature is a legal point
    # a point of the curve outside the subgroup, as a key and as a signature
    off1 = B.R1.ref_point_compress("bls12_381_g1", M.point_off_subgroup())
    off2 = G2.compress(G2.torsion_point(13))
    off_key, off_sig = (off2, off1) if min_sig else (off1, off2)
    assert B.verify(off_key, msg, sig, dst, min_sig) == B.BAD_KEY
    assert B.verify(pk, msg, off_sig, dst, min_sig) == B.MALFORMED


def test_aggregation_and_fast_aggregate_verify(signed):
    min_sig, dst, sk, pk, msg, sig = signed
    kg, sg = B.groups(min_sig)
    sks = [sk, sk + 1, 3 * sk % B.R]
    pks = [B.sk_to_pk(s, min_sig) for s in sks]
    sigs = [B.sign(s, msg, dst, min_sig) for s in sks]
    agg = B.aggregate_signatures(sigs, min_sig)
    assert agg == B.sign(sum(sks) % B.R, msg, dst, min_sig)            # the sum of signatures is the sum of keys' signature
    assert B.fast_aggregate_verify(pks, msg, agg, dst, min_sig) == B.VALID
    assert B.fast_aggregate_verify(pks[:2], msg, agg, dst, min_sig) == B.INVALID
    assert B.fast_aggregate_verify(pks[:1] + [kg.compress(None)] + pks[1:], msg, agg, dst, min_sig) == B.BAD_KEY
    assert B.aggregate_signatures([sigs[0], bytes(len(sig))], min_sig) is None
    # the empty group: BAD_KEY even with the identity signature, which the equation alone would accept
    inf_sig = sg.compress(None)
    assert B.fast_aggregate_verify([], msg, inf_sig, dst, min_sig) == B.BAD_KEY
    # keys sk and r - sk sum to the identity; each passes KeyValidate, so with the identity signature the unit is VALID
    pair = [B.sk_to_pk(sk, min_sig), B.sk_to_pk(B.R - sk, min_sig)]
    assert B.aggregate(pair, kg) == kg.compress(None)
    assert B.fast_aggregate_verify(pair, msg, inf_sig, dst, min_sig) == B.VALID
    assert B.fast_aggregate_verify(pair, msg, sig, dst, min_sig) == B.INVALID


def test_proof_of_possession(signed):
    min_sig, _, sk, pk, _, _ = signed
    proof = B.pop_prove(sk, min_sig)
    assert B.pop_verify(pk, proof, min_sig) == B.VALID
    assert B.pop_verify(B.sk_to_pk(sk + 1, min_sig), proof, min_sig) == B.INVALID


# ---- the library's side that needs no GPU ------------------------------------------------------------------------------
BLS_SYMBOLS = ("eccx_bls_public_key", "eccx_bls_sign", "eccx_bls_verify", "eccx_bls_fast_aggregate_verify")


def test_symbols_are_exported_and_bound():
    from eccoxide_amd import _lib

    lib = _lib.load()
    for base in BLS_SYMBOLS:
        for name in (base, base + "_dev"):
            assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert len(_lib.SYMBOLS[base + "_dev"][1]) == len(_lib.SYMBOLS[base][1]) + 1  # the _dev form takes the stream on top


def test_null_context_is_refused_before_anything_else():
    from eccoxide_amd import _lib
    from eccoxide_amd import engine as EN

    lib = _lib.load()
    for opts in (0, EN.BLS_MIN_SIG, 1 << 20):
        assert lib.eccx_bls_public_key(None, 1, bytes(32), None, None, opts) == -2
        assert lib.eccx_bls_sign(None, 0, None, None, None, 0, None, None, None, opts) == -2
        assert lib.eccx_bls_verify_dev(None, 1, None, None, None, 0, None, None, None, opts, None) == -2
        assert lib.eccx_bls_fast_aggregate_verify(None, 1, None, None, None, 0, None, None, None, 0, None, opts) == -2


def test_engine_names_the_scheme_and_its_tags():
    import eccoxide_amd as E
    from eccoxide_amd import engine as EN

    for name in ("bls_public_key", "bls_sign", "bls_verify", "bls_fast_aggregate_verify", "bls_pop_prove", "bls_pop_verify", "bls_aggregate"):
        assert callable(getattr(E.Engine, name)), name
        if name.startswith("bls_") and not name.startswith(("bls_pop", "bls_agg")):
            assert callable(getattr(E.Engine, name + "_t")), name
    assert (EN.BLS_DST_NUL, EN.BLS_DST_AUG, EN.BLS_DST_POP, EN.BLS_DST_POP_PROOF) == (B.DST_NUL, B.DST_AUG, B.DST_POP, B.DST_POP_PROOF)
    assert (EN.BLS_DST_NUL_MIN_SIG, EN.BLS_DST_AUG_MIN_SIG, EN.BLS_DST_POP_MIN_SIG, EN.BLS_DST_POP_PROOF_MIN_SIG) == \
        (B.DST_NUL_MIN_SIG, B.DST_AUG_MIN_SIG, B.DST_POP_MIN_SIG, B.DST_POP_PROOF_MIN_SIG)
    assert EN.BLS_MIN_SIG == 1 << 14 and EN.PREP_BLS == 1 << 15


def test_rust_wrappers_check_sizes_before_they_hand_out_pointers():
    """Every safe wrapper of rust/eccoxide-gpu/src/bls.rs that calls the library refuses sizes that do not fit first: the
    library reads n x width bytes through each pointer."""
    import os
    import re

    from tests.oracle_lib import ROOT

    src = open(os.path.join(ROOT, "rust", "eccoxide-gpu", "src", "bls.rs")).read()
    calls = {}
    for m in re.finditer(r"pub fn (\w+)\((.*?)\n}\n", src, flags=re.S):
        calls[m.group(1)] = m.group(2)
    unsafe = {name: body for name, body in calls.items() if "unsafe" in body}
    assert set(unsafe) == {"point_sum", "public_key", "sign", "verify", "fast_aggregate_verify"}
    for name, body in unsafe.items():
        assert "size_err(" in body and body.index("size_err(") < body.index("unsafe"), name
