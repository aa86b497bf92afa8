"""eccx_bls_aggregate_verify through the engine layer and libeccx.so, both variants: a dozen units against the model
(tests/bls_aggregate_ref.py, at most 40 pairs in all: the Python hash is the cost), every refusal in a non-first position
of a group of K + 1, about 300 units whose keys, signatures and aggregates the library itself makes, agreement with
bls_verify on groups of one and with bls_fast_aggregate_verify on single-message groups, require_distinct, what
eccx_reserve promises and the ABI's argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest

import eccoxide_amd as E
from eccoxide_amd import engine as EN
from tests import bls_aggregate_ref as A
from tests import bls_sig_ref as B
from tests import g2_ref as G2
from tests import msm_ref as M
from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

R = B.R
ERR_ARG = -2
VALID, INVALID, MALFORMED, BAD_KEY = EN.SIG_VALID, EN.SIG_INVALID, EN.SIG_MALFORMED, EN.SIG_BAD_KEY

with open(os.path.join(ROOT, "tests", "golden", "bls_sig.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def eng():
    with E.Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    return torch


class Variant:
    def __init__(self, min_sig):
        self.min_sig = min_sig
        self.kb, self.sb = (96, 48) if min_sig else (48, 96)
        self.dst = B.DST_NUL_MIN_SIG if min_sig else B.DST_NUL
        self.kg, self.sg = B.groups(min_sig)
        self.key_curve, self.sig_curve = ("bls12_381_g2", "bls12_381_g1") if min_sig else ("bls12_381_g1", "bls12_381_g2")
        outsider1 = B.R1.ref_point_compress("bls12_381_g1", M.point_off_subgroup())
        outsider2 = G2.compress(G2.torsion_point(13))
        self.off_key = outsider2 if min_sig else outsider1
        self.inf_key, self.inf_sig = self.kg.compress(None), self.sg.compress(None)


@pytest.fixture(scope="module", params=[False, True], ids=["min_pk", "min_sig"])
def v(request):
    return Variant(request.param)


def sk_bytes(sks):
    return b"".join(int(s).to_bytes(32, "big") for s in sks)


def _split(b, w):
    return [b[w * i:w * i + w] for i in range(len(b) // w)]


def test_ethereum_vectors(eng):
    """the aggregate of the three pinned signatures against the three (pk, message) pairs; a swap across two keys fails"""
    dst = GOLDEN["dst"].encode()
    pk = bytes.fromhex(GOLDEN["pk"])
    msgs = [bytes.fromhex(x["message"]) for x in GOLDEN["sign"]]
    sigs = b"".join(bytes.fromhex(x["signature"]) for x in GOLDEN["sign"])
    agg, fl = eng.bls_aggregate(sigs, [3])
    assert fl == b"\0" and agg == B.aggregate_signatures(_split(sigs, 96))
    assert eng.bls_aggregate_verify(msgs, agg, pk * 3, [3], dst) == bytes([VALID])
    assert eng.bls_aggregate_verify(msgs[:2], agg, pk * 2, [2], dst) == bytes([INVALID])
    sk2 = (7).to_bytes(32, "big")
    pk2, _ = eng.bls_public_key(sk2)
    s4, _ = eng.bls_sign([b"a fourth message"], sk2, dst)
    agg4, _ = eng.bls_aggregate(sigs + s4, [4])
    m4 = msgs + [b"a fourth message"]
    assert eng.bls_aggregate_verify(m4, agg4, pk * 3 + pk2, [4], dst) == bytes([VALID])
    assert eng.bls_aggregate_verify([m4[0], m4[1], m4[3], m4[2]], agg4, pk * 3 + pk2, [4], dst) == bytes([INVALID])


def test_against_the_model(eng, v):
    rng = np.random.default_rng(2381 + v.min_sig)
    sks = [int.from_bytes(rng.bytes(32), "big") % R for _ in range(6)]
    pks = [B.sk_to_pk(s, v.min_sig) for s in sks]
    ms = [b"", b"m1", b"message two", bytes(range(150)), b"m4", b"m5"]
    sign = lambda js, ks: A.aggregate_signature([sks[j] for j in js], [ms[k] for k in ks], v.dst, v.min_sig)
    keys = lambda js: [pks[j] for j in js]
    msgs = lambda ks: [ms[k] for k in ks]
    broken = lambda s: bytes([s[0] & 0x7F]) + s[1:]
    units = [
        (keys([0]), msgs([1]), sign([0], [1])),
        (keys([1, 2]), msgs([1, 2]), sign([1, 2], [1, 2])),
        (keys([0, 1, 2]), msgs([3, 3, 0]), sign([0, 1, 2], [3, 3, 0])),              # a repeated message, the empty message
        (keys([0, 1, 2, 3, 4]), msgs([0, 1, 2, 3, 4]), sign([0, 1, 2, 3, 4], [0, 1, 2, 3, 4])),
        (keys([0, 1, 2]), msgs([2, 1, 4]), sign([0, 1, 2], [1, 2, 4])),              # two messages swapped
        (keys([0]) + [v.inf_key], msgs([1, 2]), sign([0], [1])),                     # the identity key
        ([], [], v.inf_sig),                                                         # the empty group
        (keys([1, 2]), msgs([1, 2]), broken(sign([1, 2], [1, 2]))),                  # MALFORMED
        ([pks[3], B.sk_to_pk(R - sks[3], v.min_sig)], msgs([5, 5]), v.inf_sig),      # the identity signature: VALID
        (keys([0, 1, 2, 3]), msgs([0, 1, 2, 3]), sign([0, 1, 2], [0, 1, 2])),        # a signature missing from the aggregate
        ([v.off_key], msgs([1]), sign([0], [1])),                                    # a key outside the subgroup
        (keys([5, 4, 3]), msgs([5, 4, 3]), sign([3, 4, 5], [3, 4, 5])),
    ]
    assert sum(len(u[0]) for u in units) <= 40
    want = [A.aggregate_verify(k, m, s, v.dst, v.min_sig) for k, m, s in units]
    assert want == [VALID, VALID, VALID, VALID, INVALID, BAD_KEY, BAD_KEY, MALFORMED, VALID, INVALID, BAD_KEY, VALID]
    flat_m = [m for u in units for m in u[1]]
    flat_k = b"".join(k for u in units for k in u[0])
    sigs = b"".join(u[2] for u in units)
    groups = [len(u[0]) for u in units]
    assert eng.bls_aggregate_verify(flat_m, sigs, flat_k, groups, v.dst, min_sig=v.min_sig) == bytes(want)
    # require_distinct: unit 2 repeats a message and becomes INVALID on the host; unit 8 does and is VALID no more either
    got = eng.bls_aggregate_verify(flat_m, sigs, flat_k, groups, v.dst, min_sig=v.min_sig, require_distinct=True)
    exp = list(want)
    exp[2] = exp[8] = INVALID
    assert got == bytes(exp)
    assert [A.distinct(u[1]) for u in units] == [i not in (2, 8) for i in range(len(units))]


class Made:
    """keys, messages and signatures made by the library itself: pair t has secret t + 11, message b"pair %d" % t"""

    def __init__(self, eng, v, lengths):
        self.lengths = lengths
        self.offs = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
        self.terms = int(self.offs[-1])
        self.msgs = [b"pair %d" % t for t in range(self.terms)]
        secrets = sk_bytes(range(11, 11 + self.terms))
        self.keys, st = eng.bls_public_key(secrets, min_sig=v.min_sig)
        assert st == bytes([EN.SIGN_OK]) * self.terms
        self.pair_sigs, st = eng.bls_sign(self.msgs, secrets, v.dst, min_sig=v.min_sig)
        assert st == bytes([EN.SIGN_OK]) * self.terms
        self.sigs, fl = eng.bls_aggregate(self.pair_sigs, lengths, curve=v.sig_curve)
        assert fl == bytes(1 if length == 0 else 0 for length in lengths)   # the empty group's aggregate is the identity


def test_refusals_in_a_group_of_k_plus_one(eng, torch_mod, v):
    """each refusal in a non-first position of a group of K + 1 pairs, honest groups between them"""
    torch = torch_mod
    K = eng.pairing_group_chunk()
    L = K + 1
    names = ["honest", "wrong message", "wrong key", "key outside the subgroup", "identity key", "undecodable signature and a bad key",
             "honest too"]
    made = Made(eng, v, [L] * len(names))
    msgs, keys, sigs = list(made.msgs), bytearray(made.keys), bytearray(made.sigs)
    at = lambda unit, pos: unit * L + pos
    msgs[at(1, K)] = b"not what was signed"
    t = at(2, 3)
    keys[v.kb * t:v.kb * t + v.kb] = made.keys[:v.kb]                   # another unit's key
    t = at(3, K - 1)
    keys[v.kb * t:v.kb * t + v.kb] = v.off_key
    t = at(4, 1)
    keys[v.kb * t:v.kb * t + v.kb] = v.inf_key
    t = at(5, K)
    keys[v.kb * t:v.kb * t + v.kb] = v.inf_key
    sigs[v.sb * 5] &= 0x7F                                              # the compression bit cleared
    # ... and the empty group with the identity signature behind them
    groups = [L] * len(names) + [0]
    sigs = bytes(sigs) + v.inf_sig
    want = bytes([VALID, INVALID, INVALID, BAD_KEY, BAD_KEY, MALFORMED, VALID, BAD_KEY])
    assert eng.bls_aggregate_verify(msgs, sigs, bytes(keys), groups, v.dst, min_sig=v.min_sig) == want
    # the _dev form: message offsets that decrease inside unit 6 (at a non-first pair), a group range that decreases by one
    # at unit 2 (units 1 and 3 then share a pair with it: their verdicts are not specified), the last range leaving the pairs
    flat, moffs = eng._ragged(msgs)
    moffs = moffs.astype(np.int64) + 3
    t = at(6, 4)
    moffs[t] = moffs[t + 1] + 2
    go = np.concatenate(([0], np.cumsum(groups))).astype(np.int64) + 5
    go[3] = go[2] - 1
    go[len(groups)] += 1
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    side = torch.cuda.Stream()
    args = (d(bytes(3) + flat)[3:], torch.from_numpy(moffs).cuda(), d(sigs), d(bytes(keys)), torch.from_numpy(go).cuda())
    torch.cuda.synchronize()
    got = eng.bls_aggregate_verify_t(*args, v.dst, min_sig=v.min_sig, stream=side.cuda_stream)
    side.synchronize()
    got = got.cpu().numpy().tobytes()
    assert got[2] == MALFORMED and got[6] == MALFORMED and got[7] == MALFORMED
    assert (got[0], got[4], got[5]) == (VALID, BAD_KEY, MALFORMED)


def test_library_made_groups(eng, v):
    """about 300 units with the lengths of the ragged pairing test: every non-empty unit VALID (the empty ones BAD_KEY), then
    one flipped message bit per wave INVALID alone; groups of one against bls_verify, single-message groups against
    bls_fast_aggregate_verify"""
    K = eng.pairing_group_chunk()
    cyc = [0, 1, 2, K - 1, K, K + 1, 2 * K, 2 * K + 1]
    n = 300
    lengths = [cyc[i % len(cyc)] for i in range(n)]
    made = Made(eng, v, lengths)
    want = bytes(BAD_KEY if length == 0 else VALID for length in lengths)
    assert eng.bls_aggregate_verify(made.msgs, made.sigs, made.keys, lengths, v.dst, min_sig=v.min_sig) == want
    msgs, exp = list(made.msgs), bytearray(want)
    for unit in range(5, n, 64):                       # lengths[5 + 64 k] = K + 1: one unit in every wave of units
        t = int(made.offs[unit]) + unit % (K + 1)
        msgs[t] = bytes([msgs[t][0] ^ 1]) + msgs[t][1:]
        exp[unit] = INVALID
    assert eng.bls_aggregate_verify(msgs, made.sigs, made.keys, lengths, v.dst, min_sig=v.min_sig) == bytes(exp)
    # groups of one are bls_verify, the tampered and the refused among them
    ones = [int(made.offs[i]) for i in range(n) if lengths[i] == 1]
    m1 = [made.msgs[t] for t in ones]
    k1 = bytearray(b"".join(made.keys[v.kb * t:v.kb * t + v.kb] for t in ones))
    s1 = bytearray(b"".join(made.pair_sigs[v.sb * t:v.sb * t + v.sb] for t in ones))
    m1[1] = b"tampered"
    k1[v.kb * 2:v.kb * 3] = v.inf_key
    s1[v.sb * 3] &= 0x7F
    k1[v.kb * 4:v.kb * 5] = k1[:v.kb]
    got = eng.bls_aggregate_verify(m1, bytes(s1), bytes(k1), [1] * len(ones), v.dst, min_sig=v.min_sig)
    assert got == eng.bls_verify(m1, bytes(s1), bytes(k1), v.dst, min_sig=v.min_sig)
    assert got[:5] == bytes([VALID, INVALID, BAD_KEY, MALFORMED, INVALID]) and got[5:] == bytes([VALID]) * (len(ones) - 5)
    # single-message groups are bls_fast_aggregate_verify
    sizes = [1, 2, K + 1, 0, 3, 2 * K + 1]
    total = sum(sizes)
    secrets = sk_bytes(range(1000, 1000 + total))
    keys, _ = eng.bls_public_key(secrets, min_sig=v.min_sig)
    unit_msgs = [b"committee %d" % i for i in range(len(sizes))]
    flat = [unit_msgs[i] for i, size in enumerate(sizes) for _ in range(size)]
    pair_sigs, _ = eng.bls_sign(flat, secrets, v.dst, min_sig=v.min_sig)
    aggs, _ = eng.bls_aggregate(pair_sigs, sizes, curve=v.sig_curve)
    keys = bytearray(keys)
    keys[v.kb * 4:v.kb * 5] = keys[:v.kb]              # unit 2: a wrong key
    got = eng.bls_aggregate_verify(flat, aggs, bytes(keys), sizes, v.dst, min_sig=v.min_sig)
    assert got == eng.bls_fast_aggregate_verify(unit_msgs, aggs, bytes(keys), sizes, v.dst, min_sig=v.min_sig)
    assert got == bytes([VALID, VALID, INVALID, BAD_KEY, VALID, VALID])


def test_reserve_covers_the_dev_call(torch_mod, eng, v):
    torch = torch_mod
    K = eng.pairing_group_chunk()
    lengths = [1, K + 1, 0, 2, 2 * K + 1] * 6
    made = Made(eng, v, lengths)
    n = len(lengths)
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    flat, moffs = eng._ragged(made.msgs)
    args = (d(flat), torch.from_numpy(moffs.astype(np.int64)).cuda(), d(made.sigs), d(made.keys), torch.from_numpy(made.offs).cuda())
    with E.Engine(0) as fresh:
        fresh.reserve("bls12_381_g2", n + made.terms, var=False, bls_aggregate=True)
        before = fresh.device_bytes()
        assert before > 0
        got = fresh.bls_aggregate_verify_t(*args, v.dst, min_sig=v.min_sig)
        few = fresh.bls_aggregate_verify_t(args[0], args[1][:3], args[2][:2 * v.sb], args[3][:2 * v.kb],
                                           torch.tensor([0, 1, 2], dtype=torch.int64).cuda(), v.dst, min_sig=v.min_sig)
        torch.cuda.synchronize()
        assert fresh.device_bytes() == before
        assert got.cpu().numpy().tobytes() == bytes(BAD_KEY if length == 0 else VALID for length in lengths)
        assert few.cpu().numpy().tobytes() == bytes([VALID, INVALID])   # unit 1 of `few` has unit 1's aggregate over K + 1 pairs


def test_argument_checks_and_empty_batches(eng, v):
    lib, ctx = eng._lib, eng._ctx
    ms = EN.BLS_MIN_SIG if v.min_sig else 0
    offs = np.array([0, 3], dtype=np.uint64)
    o = offs.ctypes.data
    st = ctypes.create_string_buffer(b"\x5a", 1)
    err = lambda: lib.eccx_last_error(ctx).decode()
    msg, dst = b"abc", v.dst
    sk = sk_bytes([5])
    key, _ = eng.bls_public_key(sk, min_sig=v.min_sig)
    sig, _ = eng.bls_sign([msg], sk, dst, min_sig=v.min_sig)
    one = np.array([0, 1], dtype=np.uint64)
    g = one.ctypes.data
    call = lambda *a: lib.eccx_bls_aggregate_verify(ctx, *a)
    assert call(1, msg, o, dst, len(dst), sig, key, g, 1, st, ms) == 0 and st.raw == bytes([VALID])
    st.raw = b"\x5a"
    for bad in (EN.VALIDATE_POINTS, EN.CT_SCAN, EN.CT_GATHER, EN.CHECK_SUBGROUP, 1 << 15, 1 << 31):
        assert call(1, msg, o, dst, len(dst), sig, key, g, 1, st, ms | bad) == ERR_ARG and "opts" in err()
        assert lib.eccx_bls_aggregate_verify_dev(ctx, 0, None, None, None, 0, None, None, None, 0, None, ms | bad, None) == ERR_ARG
    assert call(1, msg, o, dst, len(dst), None, key, g, 1, st, ms) == ERR_ARG and "null buffer" in err()
    assert call(1, msg, o, dst, len(dst), sig, None, g, 1, st, ms) == ERR_ARG and "null buffer" in err()
    assert call(1, msg, o, dst, len(dst), sig, key, None, 1, st, ms) == ERR_ARG and "null buffer" in err()
    assert call(1, msg, o, dst, len(dst), sig, key, g, 1, None, ms) == ERR_ARG and "null buffer" in err()
    assert call(1, msg, None, dst, len(dst), sig, key, g, 1, st, ms) == ERR_ARG and "null buffer" in err()
    assert call(1, None, o, dst, len(dst), sig, key, g, 1, st, ms) == ERR_ARG and "null buffer" in err()
    assert call(1, msg, o, None, 3, sig, key, g, 1, st, ms) == ERR_ARG and "null buffer" in err()
    down = np.array([3, 0], dtype=np.uint64)
    assert call(1, msg, down.ctypes.data, dst, len(dst), sig, key, g, 1, st, ms) == ERR_ARG and "decrease" in err()
    assert call(1, msg, o, dst, len(dst), sig, key, np.array([1, 0], dtype=np.uint64).ctypes.data, 1, st, ms) == ERR_ARG and "decrease" in err()
    assert call(1, msg, o, dst, len(dst), sig, key, np.array([0, 2], dtype=np.uint64).ctypes.data, 1, st, ms) == ERR_ARG and "beyond" in err()
    assert lib.eccx_bls_aggregate_verify_dev(ctx, 1, None, None, None, 0, None, None, None, 1, None, ms, None) == ERR_ARG and "null buffer" in err()
    assert st.raw == b"\x5a"
    assert call(0, None, None, None, 0, None, None, None, 0, None, ms) == 0
    assert lib.eccx_bls_aggregate_verify_dev(ctx, 0, None, None, None, 0, None, None, None, 0, None, ms, None) == 0
    # no pairs at all: every unit is the empty group
    zero = np.zeros(3, dtype=np.uint64)
    two = ctypes.create_string_buffer(2)
    assert call(2, None, None, dst, len(dst), v.inf_sig * 2, None, zero.ctypes.data, 0, two, ms) == 0 and two.raw == bytes([BAD_KEY]) * 2
