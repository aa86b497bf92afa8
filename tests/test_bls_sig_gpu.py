"""eccx_bls_public_key / _sign / _verify / _fast_aggregate_verify through the engine layer and libeccx.so against the model
(tests/bls_sig_ref.py, itself pinned to the Ethereum vectors of tests/golden/bls_sig.json), both variants.  Every expected
value is the model's.  The distinct cases are computed once per module and repeated with a short period, so that every
wavefront of a batch holds VALID and non-VALID units side by side."""
import ctypes
import json
import os

import numpy as np
import pytest

import eccoxide_amd as E
from eccoxide_amd import engine as EN
from tests import bls_sig_ref as B
from tests import g2_ref as G2
from tests import msm_ref as M
from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

R = B.R
P = G2.P
ERR_ARG = -2
PERIOD = 13

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
    """One variant's honest units (13 secrets, keys, messages, signatures) from the model, made once."""

    def __init__(self, min_sig):
        self.min_sig = min_sig
        self.kb, self.sb = (96, 48) if min_sig else (48, 96)
        self.dst = B.DST_NUL_MIN_SIG if min_sig else B.DST_NUL
        self.kg, self.sg = B.groups(min_sig)
        rng = np.random.default_rng(1381 + min_sig)
        raw = rng.bytes(32 * PERIOD)
        self.sks = [int.from_bytes(raw[32 * j:32 * j + 32], "big") % R for j in range(PERIOD)]
        self.sks[1] = R - 1
        self.msgs = [b"unit %d " % j * (j % 4) for j in range(PERIOD)]
        self.msgs[0], self.msgs[5] = b"", bytes(range(200))
        self.pks = [B.sk_to_pk(s, min_sig) for s in self.sks]
        self.sigs = [B.sign(s, m, self.dst, min_sig) for s, m in zip(self.sks, self.msgs)]
        outsider1 = B.R1.ref_point_compress("bls12_381_g1", M.point_off_subgroup())
        outsider2 = G2.compress(G2.torsion_point(13))
        self.off_key, self.off_sig = (outsider2, outsider1) if min_sig else (outsider1, outsider2)

    def no_point(self, group):
        """a compressed encoding whose x has no point on the curve"""
        x = 1
        while True:
            x += 1
            enc = bytes([0x80]) + bytes(group.size - 2) + bytes([x])
            if group.decode(enc) == B.REJECT and self._x_free(group, enc):
                return enc

    @staticmethod
    def _x_free(group, enc):  # neither sign bit gives a point: the x itself is the reason
        return group.decode(bytes([enc[0] | 0x20]) + enc[1:]) == B.REJECT

    def x_not_below_p(self, group):
        """x = p in the leading coordinate (c1 on G2): flag bits over the bytes of p"""
        pb = P.to_bytes(48, "big")
        return bytes([0x80 | pb[0]]) + pb[1:] + bytes(group.size - 48)


@pytest.fixture(scope="module", params=[False, True], ids=["min_pk", "min_sig"])
def v(request):
    return Variant(request.param)


def sk_bytes(sks):
    return b"".join(s.to_bytes(32, "big") for s in sks)


def test_golden_vectors(eng):
    sk = bytes.fromhex(GOLDEN["sk"])
    dst = GOLDEN["dst"].encode()
    assert dst == EN.BLS_DST_POP == B.DST_POP
    msgs = [bytes.fromhex(x["message"]) for x in GOLDEN["sign"]]
    keys, kst = eng.bls_public_key(sk * 3)
    assert keys == bytes.fromhex(GOLDEN["pk"]) * 3 and kst == bytes([EN.SIGN_OK]) * 3
    sigs, sst = eng.bls_sign(msgs, sk * 3, dst)
    assert sigs.hex() == "".join(x["signature"] for x in GOLDEN["sign"]) and sst == bytes([EN.SIGN_OK]) * 3
    assert eng.bls_verify(msgs, sigs, keys, dst) == bytes([EN.SIG_VALID]) * 3
    assert eng.bls_verify(msgs[1:] + msgs[:1], sigs, keys, dst) == bytes([EN.SIG_INVALID]) * 3
    assert eng.bls_public_key(sk * 3, ct_gather=True) == (keys, kst)
    assert eng.bls_sign(msgs, sk * 3, dst, ct_gather=True) == (sigs, sst)  # accepted for min-pk; the ladder has no gather form


def test_sign_and_keys_against_the_model(eng, v):
    n = 300
    tag = b"a tag of three hundred bytes " * 11
    tag = tag[:300]
    specials = {3: 0, 4: R, 6: (1 << 256) - 1}  # status NONE and zero bytes; sks[1] = r - 1 is OK
    sks = [specials.get(j, v.sks[j]) for j in range(PERIOD)]
    want_sig = [B.sign(s, m, tag, v.min_sig) for s, m in zip(sks, v.msgs)]
    want_key = [B.sk_to_pk(s, v.min_sig) for s in sks]
    assert want_sig[1] is not None and [j for j in range(PERIOD) if want_sig[j] is None] == [3, 4, 6]
    idx = [i % PERIOD for i in range(n)]
    secrets = sk_bytes(sks[j] for j in idx)
    sigs, st = eng.bls_sign([v.msgs[j] for j in idx], secrets, tag, min_sig=v.min_sig)
    assert st == bytes(0 if want_sig[j] is None else 1 for j in idx)
    assert sigs == b"".join(want_sig[j] or bytes(v.sb) for j in idx)
    keys, kst = eng.bls_public_key(secrets, min_sig=v.min_sig)
    assert kst == st and keys == b"".join(want_key[j] or bytes(v.kb) for j in idx)


def verify_cases(v):
    """(key, message, signature) triples: the honest units, then the crafted ones"""
    k, m, s = v.pks, v.msgs, v.sigs
    bad_flags = bytes([s[2][0] & 0x7F]) + s[2][1:]
    inf_key, inf_sig = v.kg.compress(None), v.sg.compress(None)
    cases = [(k[j], m[j], s[j]) for j in range(PERIOD)]
    cases += [
        (k[2], m[3], s[2]),                          # a wrong message
        (k[3], m[2], s[2]),                          # a wrong key
        (k[2], m[2], s[3]),                          # a wrong signature
        (k[2], m[2], bad_flags),                     # the compression bit cleared
        (k[2], m[2], bytes([s[2][0] | 0x40]) + s[2][1:]),  # the infinity bit over a payload
        (k[2], m[2], v.x_not_below_p(v.sg)),         # x >= p
        (k[2], m[2], v.no_point(v.sg)),              # no point with this x
        (k[2], m[2], v.off_sig),                     # a point outside the subgroup
        (k[2], m[2], inf_sig),                       # the identity signature: legal, the equation decides
        (inf_key, m[2], s[2]),                       # the identity key (KeyValidate)
        (inf_key, m[2], inf_sig),                    # ... which the equation alone would accept
        (v.no_point(v.kg), m[2], s[2]),              # a key that is no curve point
        (v.x_not_below_p(v.kg), m[2], s[2]),
        (v.off_key, m[2], s[2]),                     # a key outside the subgroup
        (inf_key, m[2], bad_flags),                  # MALFORMED and BAD_KEY: MALFORMED
        (v.off_key, m[2], v.off_sig),
    ]
    return cases


def test_verify_against_the_model(eng, torch_mod, v):
    torch = torch_mod
    cases = verify_cases(v)
    want = [B.verify(k, m, s, v.dst, v.min_sig) for k, m, s in cases]
    assert want[:PERIOD] == [B.VALID] * PERIOD and set(want) == {B.VALID, B.INVALID, B.MALFORMED, B.BAD_KEY}
    assert want[-2:] == [B.MALFORMED, B.MALFORMED] and want[PERIOD + 8] == B.INVALID and want[PERIOD + 10] == B.BAD_KEY
    n = 549  # two workgroups and a part of one
    idx = [i % len(cases) for i in range(n)]
    msgs = [cases[j][1] for j in idx]
    keys, sigs = b"".join(cases[j][0] for j in idx), b"".join(cases[j][2] for j in idx)
    assert eng.bls_verify(msgs, sigs, keys, v.dst, min_sig=v.min_sig) == bytes(want[j] for j in idx)
    # the _dev form on a side stream, with two lanes whose offsets decrease: MALFORMED, alone
    flat, offs = eng._ragged(msgs[:40])
    offs = offs.astype(np.int64) + 5
    offs[7], offs[20] = offs[8] + 3, offs[21] + 1
    side = torch.cuda.Stream()
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    d_m, d_o, d_s, d_k = d(bytes(5) + flat)[5:], torch.from_numpy(offs).cuda(), d(sigs[:40 * v.sb]), d(keys[:40 * v.kb])
    torch.cuda.synchronize()
    got = eng.bls_verify_t(d_m, d_o, d_s, d_k, v.dst, min_sig=v.min_sig, stream=side.cuda_stream)
    side.synchronize()
    exp = [want[j] for j in idx[:40]]
    for lane in (6, 7, 19, 20):  # a decreasing pair spoils the lane that ends low and the one that starts high
        if offs[lane + 1] < offs[lane]:
            exp[lane] = B.MALFORMED
    exp[6] = B.verify(cases[idx[6]][0], flat[offs[6] - 5:offs[7] - 5], cases[idx[6]][2], v.dst, v.min_sig)
    exp[19] = B.verify(cases[idx[19]][0], flat[offs[19] - 5:offs[20] - 5], cases[idx[19]][2], v.dst, v.min_sig)
    assert got.cpu().numpy().tobytes() == bytes(exp)


def test_fast_aggregate_verify_against_the_model(eng, torch_mod, v):
    torch = torch_mod
    msg = b"one message for the whole committee"
    inf_sig = v.sg.compress(None)

    def committee(size, shift):
        js = [(shift + i) % PERIOD for i in range(size)]
        return [v.pks[j] for j in js], B.sign(sum(v.sks[j] for j in js) % R, msg, v.dst, v.min_sig)

    units = [committee(size, size) for size in (1, 2, 64, 65, 130)]
    keys65, sig65 = units[3]
    units += [
        (keys65[:30] + [v.kg.compress(None)] + keys65[31:], sig65),          # one bad key in the middle: the identity
        (keys65[:40] + [v.off_key] + keys65[41:], sig65),                    # ... and one outside the subgroup
        (keys65[:-1], sig65),                                                # a key missing: the equation fails
        ([], inf_sig),                                                       # the empty group: BAD_KEY
        ([B.sk_to_pk(v.sks[2], v.min_sig), B.sk_to_pk(R - v.sks[2], v.min_sig)], inf_sig),  # sums to the identity: VALID
        ([B.sk_to_pk(v.sks[2], v.min_sig), B.sk_to_pk(R - v.sks[2], v.min_sig)], units[0][1]),
        (keys65, bytes([sig65[0] & 0x7F]) + sig65[1:]),                      # MALFORMED
    ]
    want = [B.fast_aggregate_verify(ks, msg, sg, v.dst, v.min_sig) for ks, sg in units]
    assert want == [B.VALID] * 5 + [B.BAD_KEY, B.BAD_KEY, B.INVALID, B.BAD_KEY, B.VALID, B.INVALID, B.MALFORMED]
    groups = [len(ks) for ks, _ in units]
    flat_keys, sigs = b"".join(b"".join(ks) for ks, _ in units), b"".join(sg for _, sg in units)
    n = len(units)
    assert eng.bls_fast_aggregate_verify([msg] * n, sigs, flat_keys, groups, v.dst, min_sig=v.min_sig) == bytes(want)
    # the _dev form: a key range that decreases and one that leaves the keys are MALFORMED, alone
    ko = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(groups, out=ko[1:])
    ko += 9
    ko[2] = ko[1] - 1          # unit 1's range decreases; unit 2 then spans keys it was not signed for
    ko[n] = ko[n] + 1          # the last unit's range leaves the keys
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    offs = torch.arange(n + 1, dtype=torch.int64).cuda() * len(msg)
    got = eng.bls_fast_aggregate_verify_t(d(msg * n), offs, d(sigs), d(flat_keys), torch.from_numpy(ko).cuda(), v.dst, min_sig=v.min_sig)
    torch.cuda.synchronize()
    exp = list(want)
    exp[1], exp[2], exp[n - 1] = B.MALFORMED, B.INVALID, B.MALFORMED
    assert got.cpu().numpy().tobytes() == bytes(exp)
    # aggregation of the model's signatures against the model's sum
    sig_sets = [[v.sigs[(3 * g + i) % PERIOD] for i in range(size)] for g, size in enumerate((1, 2, 64, 65, 130))]
    enc = b"".join(b"".join(x) for x in sig_sets)
    agg, fl = eng.bls_aggregate(enc, [len(x) for x in sig_sets], curve="bls12_381_g1" if v.min_sig else "bls12_381_g2")
    assert fl == bytes(5) and agg == b"".join(B.aggregate_signatures(x, v.min_sig) for x in sig_sets)


def test_proof_of_possession(eng, v):
    secrets = sk_bytes(v.sks[:3])
    proofs, st = eng.bls_pop_prove(secrets, min_sig=v.min_sig)
    assert st == bytes([EN.SIGN_OK]) * 3 and proofs[:v.sb] == B.pop_prove(v.sks[0], v.min_sig)
    keys = b"".join(v.pks[:3])
    assert eng.bls_pop_verify(keys, proofs, min_sig=v.min_sig) == bytes([B.pop_verify(v.pks[j], proofs[v.sb * j:v.sb * j + v.sb], v.min_sig)
                                                                         for j in range(3)]) == bytes([EN.SIG_VALID]) * 3
    swapped = b"".join(v.pks[j] for j in (1, 0, 2))
    assert eng.bls_pop_verify(swapped, proofs, min_sig=v.min_sig) == bytes([EN.SIG_INVALID, EN.SIG_INVALID, EN.SIG_VALID])


def test_argument_checks_and_empty_batches(eng, v):
    lib, ctx = eng._lib, eng._ctx
    ms = EN.BLS_MIN_SIG if v.min_sig else 0
    offs = np.array([0, 3], dtype=np.uint64)
    out, st = ctypes.create_string_buffer(b"\x5a" * 96, 96), ctypes.create_string_buffer(b"\x5a", 1)
    untouched = lambda: (out.raw, st.raw) == (b"\x5a" * 96, b"\x5a")
    err = lambda: lib.eccx_last_error(ctx).decode()
    sk, msg, dst = sk_bytes(v.sks[:1]), b"abc", v.dst
    refused = [EN.VALIDATE_POINTS, EN.MIRROR_REFERENCE, EN.CT_SCAN, EN.CHECK_SUBGROUP, EN.H2C_NU, EN.ASSUME_SUBGROUP, 1 << 15, 1 << 31]
    for bad in refused + [EN.CT_GATHER]:
        assert lib.eccx_bls_verify(ctx, 1, msg, offs.ctypes.data, dst, len(dst), v.sigs[0], v.pks[0], st, ms | bad) == ERR_ARG and "opts" in err()
        assert lib.eccx_bls_verify_dev(ctx, 1, None, None, None, 0, None, None, None, ms | bad, None) == ERR_ARG
        assert lib.eccx_bls_fast_aggregate_verify(ctx, 1, msg, offs.ctypes.data, dst, len(dst), v.sigs[0], v.pks[0], offs.ctypes.data, 1, st,
                                                  ms | bad) == ERR_ARG
        assert lib.eccx_bls_fast_aggregate_verify_dev(ctx, 0, None, None, None, 0, None, None, None, 0, None, ms | bad, None) == ERR_ARG
        assert untouched(), bad
    for bad in refused + ([EN.CT_GATHER] if v.min_sig else []):  # the gather comb exists on G1: min-pk keys only
        assert lib.eccx_bls_sign(ctx, 1, msg, offs.ctypes.data, dst, len(dst), sk, out, st, ms | bad) == ERR_ARG and "opts" in err()
        assert lib.eccx_bls_public_key(ctx, 1, sk, out, st, ms | bad) == ERR_ARG and "opts" in err()
        assert lib.eccx_bls_sign_dev(ctx, 1, None, None, None, 0, None, None, None, ms | bad, None) == ERR_ARG
        assert lib.eccx_bls_public_key_dev(ctx, 0, None, None, None, ms | bad, None) == ERR_ARG
        assert untouched(), bad
    # null buffers, decreasing offsets in the host forms
    down = np.array([3, 0], dtype=np.uint64)
    assert lib.eccx_bls_verify(ctx, 1, msg, down.ctypes.data, dst, len(dst), v.sigs[0], v.pks[0], st, ms) == ERR_ARG and "decrease" in err()
    assert lib.eccx_bls_sign(ctx, 1, msg, down.ctypes.data, dst, len(dst), sk, out, st, ms) == ERR_ARG and "decrease" in err()
    assert lib.eccx_bls_verify(ctx, 1, None, offs.ctypes.data, dst, len(dst), v.sigs[0], v.pks[0], st, ms) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_bls_verify(ctx, 1, msg, offs.ctypes.data, None, 3, v.sigs[0], v.pks[0], st, ms) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_bls_verify(ctx, 1, msg, offs.ctypes.data, dst, len(dst), None, v.pks[0], st, ms) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_bls_verify(ctx, 1, msg, offs.ctypes.data, dst, len(dst), v.sigs[0], v.pks[0], None, ms) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_bls_sign(ctx, 1, msg, offs.ctypes.data, dst, len(dst), None, out, st, ms) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_bls_public_key(ctx, 1, None, out, st, ms) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_bls_fast_aggregate_verify(ctx, 1, msg, offs.ctypes.data, dst, len(dst), v.sigs[0], v.pks[0], None, 1, st, ms) == ERR_ARG
    assert lib.eccx_bls_verify_dev(ctx, 1, None, None, None, 0, None, None, None, ms, None) == ERR_ARG and "null buffer" in err()
    assert untouched()
    # n == 0
    assert lib.eccx_bls_public_key(ctx, 0, None, None, None, ms) == 0 and lib.eccx_bls_sign(ctx, 0, None, None, None, 0, None, None, None, ms) == 0
    assert lib.eccx_bls_verify(ctx, 0, None, None, None, 0, None, None, None, ms) == 0
    assert lib.eccx_bls_fast_aggregate_verify_dev(ctx, 0, None, None, None, 0, None, None, None, 0, None, ms, None) == 0
    assert untouched()
    # an empty tag is a tag
    sig0, st0 = eng.bls_sign([msg], sk, b"", min_sig=v.min_sig)
    assert (sig0, st0) == (B.sign(v.sks[0], msg, b"", v.min_sig), b"\1")


def test_reserve_covers_the_dev_calls(torch_mod, v):
    torch = torch_mod
    n = 70
    idx = [i % PERIOD for i in range(n)]
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    flat = b"".join(v.msgs[j] for j in idx)
    lens = np.cumsum([0] + [len(v.msgs[j]) for j in idx]).astype(np.int64)
    d_m, d_o = d(flat), torch.from_numpy(lens).cuda()
    d_sk = d(sk_bytes(v.sks[j] for j in idx))
    d_keys = d(b"".join(v.pks[j] for j in idx))
    ko = torch.arange(n + 1, dtype=torch.int64).cuda()
    with E.Engine(0) as fresh:
        fresh.prepare("bls12_381_g2" if v.min_sig else "bls12_381_g1", base=False, ct=True)
        fresh.reserve("bls12_381_g2", n, var=False, bls=True)
        before = fresh.device_bytes()
        assert before > 0
        keys, kst = fresh.bls_public_key_t(d_sk, min_sig=v.min_sig)
        sigs, sst = fresh.bls_sign_t(d_m, d_o, d_sk, v.dst, min_sig=v.min_sig)
        ver = fresh.bls_verify_t(d_m, d_o, sigs.reshape(-1), d_keys, v.dst, min_sig=v.min_sig)
        fav = fresh.bls_fast_aggregate_verify_t(d_m, d_o, sigs.reshape(-1), d_keys, ko, v.dst, min_sig=v.min_sig)
        torch.cuda.synchronize()
        assert fresh.device_bytes() == before
        assert keys.cpu().numpy().tobytes() == b"".join(v.pks[j] for j in idx) and kst.cpu().numpy().tobytes() == b"\1" * n
        assert sigs.cpu().numpy().tobytes() == b"".join(v.sigs[j] for j in idx) and sst.cpu().numpy().tobytes() == b"\1" * n
        assert ver.cpu().numpy().tobytes() == fav.cpu().numpy().tobytes() == bytes([EN.SIG_VALID]) * n
