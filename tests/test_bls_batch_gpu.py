"""eccx_bls_batch_verify through the engine layer and libeccx.so, both variants.  Keys and honest signatures come from
Engine.bls_public_key / Engine.bls_sign (pinned to the model by tests/test_bls_sig_gpu.py); every expected verdict comes
from the model (tests/bls_batch_ref.py: verdict(), over the honest signatures), never from which members a test tampered
with and never from the library.  Coefficients are fixed per test, so every run checks the same equations."""
import ctypes
import json
import os

import numpy as np
import pytest

import eccoxide_amd as E
from eccoxide_amd import engine as EN
from tests import bls_batch_ref as BR
from tests import bls_sig_ref as B
from tests import g2_ref as G2
from tests import msm_ref as M
from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

R = B.R
ERR_ARG = -2
VALID, INVALID, MALFORMED, BAD_KEY = EN.SIG_VALID, EN.SIG_INVALID, EN.SIG_MALFORMED, EN.SIG_BAD_KEY
NKEYS = 7   # distinct secrets: the model validates each key once

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
        self.sig_curve = "bls12_381_g1" if min_sig else "bls12_381_g2"
        outsider1 = B.R1.ref_point_compress("bls12_381_g1", M.point_off_subgroup())
        outsider2 = G2.compress(G2.torsion_point(13))
        self.off_key, self.off_sig = (outsider2, outsider1) if min_sig else (outsider1, outsider2)
        self.inf_key, self.inf_sig = self.kg.compress(None), self.sg.compress(None)
        pb = G2.P.to_bytes(48, "big")
        self.big_x_sig = bytes([0x80 | pb[0]]) + pb[1:] + bytes(self.sb - 48)   # x = p in the leading coordinate
        x = 1
        while True:   # an x with no point on the curve, under either sign bit
            x += 1
            enc = bytes([0x80]) + bytes(self.sb - 2) + bytes([x])
            if self.sg.decode(enc) == B.REJECT and self.sg.decode(bytes([0xA0]) + enc[1:]) == B.REJECT:
                self.no_point_sig = enc
                break


@pytest.fixture(scope="module", params=[False, True], ids=["min_pk", "min_sig"])
def v(request):
    return Variant(request.param)


def sk_bytes(sks):
    return b"".join(int(s).to_bytes(32, "big") for s in sks)


def split(b, w):
    return [b[w * i:w * i + w] for i in range(len(b) // w)]


def fixed_coeffs(n, seed):
    """n nonzero 8-byte coefficients, the same at every run"""
    raw = np.random.default_rng(seed).bytes(8 * n)
    return [raw[8 * i:8 * i + 8] if any(raw[8 * i:8 * i + 8]) else b"\0" * 7 + b"\1" for i in range(n)]


class Made:
    """n triples made by the library: member t has secret 11 + t % NKEYS and message b"member %d" % t (msgs overrides)"""

    def __init__(self, eng, v, n, msgs=None, dst=None):
        self.n = n
        self.dst = v.dst if dst is None else dst
        self.sks = [11 + t % NKEYS for t in range(n)]
        self.msgs = [b"member %d" % t for t in range(n)] if msgs is None else list(msgs)
        secrets = sk_bytes(self.sks)
        keys, st = eng.bls_public_key(secrets, min_sig=v.min_sig)
        assert st == bytes([EN.SIGN_OK]) * n
        sigs, st = eng.bls_sign(self.msgs, secrets, self.dst, min_sig=v.min_sig)
        assert st == bytes([EN.SIGN_OK]) * n
        self.keys, self.sigs = split(keys, v.kb), split(sigs, v.sb)


def honest_for(eng, v, sks, msgs, dst):
    """the honest signature of each (secret, message) pair; None where the member has no valid key (sk is None)"""
    idx = [i for i, s in enumerate(sks) if s is not None]
    out = [None] * len(sks)
    if idx:
        sigs, st = eng.bls_sign([msgs[i] for i in idx], sk_bytes(sks[i] for i in idx), dst, min_sig=v.min_sig)
        assert st == bytes([EN.SIGN_OK]) * len(idx)
        for i, s in zip(idx, split(sigs, v.sb)):
            out[i] = s
    return out


def model(v, keys, sigs, coeffs, honest, lengths):
    """(batch verdicts, member statuses) from the model"""
    offs = np.concatenate(([0], np.cumsum(lengths))).astype(int)
    verdicts = [BR.verdict(keys[a:b], sigs[a:b], coeffs[a:b], honest[a:b], v.min_sig) for a, b in zip(offs, offs[1:])]
    status = [BR.member_status(k, s, c, v.min_sig, h) for k, s, c, h in zip(keys, sigs, coeffs, honest)]
    return bytes(verdicts), bytes(status)


def run(eng, v, msgs, sigs, keys, coeffs, lengths, dst=None):
    return eng.bls_batch_verify(msgs, b"".join(sigs), b"".join(keys), v.dst if dst is None else dst, batches=lengths,
                                coeffs=b"".join(coeffs), min_sig=v.min_sig)


def test_ethereum_vectors_as_one_batch(eng):
    dst = GOLDEN["dst"].encode()
    pk = bytes.fromhex(GOLDEN["pk"])
    msgs = [bytes.fromhex(x["message"]) for x in GOLDEN["sign"]]
    sigs = b"".join(bytes.fromhex(x["signature"]) for x in GOLDEN["sign"])
    coeffs = b"".join(fixed_coeffs(3, 1))
    assert eng.bls_batch_verify(msgs, sigs, pk * 3, dst, coeffs=coeffs) == (bytes([VALID]), bytes([VALID]) * 3)
    assert eng.bls_batch_verify(msgs, sigs, pk * 3, dst, batches=[1, 1, 1], coeffs=coeffs)[0] == bytes([VALID]) * 3
    swapped = sigs[96:192] + sigs[:96] + sigs[192:]
    want = BR.verdict([pk] * 3, split(swapped, 96), split(coeffs, 8), split(sigs, 96))
    assert want == INVALID and eng.bls_batch_verify(msgs, swapped, pk * 3, dst, coeffs=coeffs)[0] == bytes([want])


LENGTHS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 130]


def test_valid_batches_and_isolation(eng, v):
    """the lengths around the chunk of K = 8 terms, the short-sum boundary and the wave, all valid in one call; then one
    tampered signature in the middle of the batch of 65 and one in the batch of 9: those two INVALID, the others as before"""
    n = sum(LENGTHS)
    made = Made(eng, v, n)
    coeffs = fixed_coeffs(n, 2)
    want = model(v, made.keys, made.sigs, coeffs, made.sigs, LENGTHS)
    assert want == (bytes([VALID]) * len(LENGTHS), bytes([VALID]) * n)
    assert run(eng, v, made.msgs, made.sigs, made.keys, coeffs, LENGTHS) == want
    offs = np.concatenate(([0], np.cumsum(LENGTHS))).astype(int)
    sigs = list(made.sigs)
    for batch, pos in ((8, 32), (5, 4)):
        t = int(offs[batch]) + pos
        sigs[t] = made.sigs[t + 1]   # another member's signature: a point of the subgroup, the wrong one
    want2 = model(v, made.keys, sigs, coeffs, made.sigs, LENGTHS)
    assert [i for i in range(len(LENGTHS)) if want2[0][i] != want[0][i]] == [5, 8] and want2[0][5] == want2[0][8] == INVALID
    assert run(eng, v, made.msgs, sigs, made.keys, coeffs, LENGTHS) == want2


def test_cancelling_forgery(eng, v):
    """sig_1 + D and sig_2 - D: VALID under the plain sum check (all coefficients 1), INVALID as soon as the two
    coefficients differ, in the bottom byte or in the top byte alone -- what a kernel that ignores, truncates or byte-swaps
    the coefficients gets wrong.  The model says the same in every case."""
    made = Made(eng, v, 4)
    d = v.sg.mul(0xD1FF, v.sg.gen)
    pts = [v.sg.decode(s) for s in made.sigs]
    sigs = list(made.sigs)
    sigs[1] = v.sg.compress(v.sg.add(pts[1], d))
    sigs[2] = v.sg.compress(v.sg.add(pts[2], BR.neg(v.sg, d)))
    c = lambda *vals: [int(x).to_bytes(8, "big") for x in vals]
    top = 1 << 56
    cases = [(c(1, 1, 1, 1), VALID), (c(9, 1, 2, 9), INVALID), (c(9, 5, 5, 9), VALID),
             (c(3, top | 1, 1, 3), INVALID), (c(3, top | 1, 2 * top | 1, 3), INVALID), (c(3, top | 1, top | 1, 3), VALID),
             (c(3, top | 1, top | 2, 3), INVALID), (c(1, (1 << 64) - 1, (1 << 64) - 1, 1), VALID), (c(1, 1 << 63, 1 << 62, 1), INVALID)]
    for coeffs, expect in cases:
        want = model(v, made.keys, sigs, coeffs, made.sigs, [4])
        assert want[0] == bytes([expect]), coeffs
        assert run(eng, v, made.msgs, sigs, made.keys, coeffs, [4]) == want, coeffs


def test_equal_and_opposite_operands(eng, v):
    made = Made(eng, v, 3)
    # the same triple twice in a batch, with equal and with different coefficients: the sums have equal members
    msgs, keys, sigs = [made.msgs[0]] * 2 + made.msgs[1:], [made.keys[0]] * 2 + made.keys[1:], [made.sigs[0]] * 2 + made.sigs[1:]
    for coeffs in (fixed_coeffs(1, 3) * 2 + fixed_coeffs(2, 4), fixed_coeffs(4, 5)):
        want = model(v, keys, sigs, coeffs, sigs, [2, 2])
        assert want[0] == bytes([VALID, VALID]) and run(eng, v, msgs, sigs, keys, coeffs, [2, 2]) == want
    # keys sk and r - sk on one message with equal coefficients: sum c_i sig_i is the identity, the signature term is
    # flagged infinite, and so is the sum of the scaled keys' pairings: VALID
    sks = [1234567, R - 1234567]
    pk, st = eng.bls_public_key(sk_bytes(sks), min_sig=v.min_sig)
    sg, st2 = eng.bls_sign([b"both"] * 2, sk_bytes(sks), v.dst, min_sig=v.min_sig)
    assert st + st2 == bytes([EN.SIGN_OK]) * 4
    keys, sigs = split(pk, v.kb), split(sg, v.sb)
    assert v.sg.add(v.sg.decode(sigs[0]), v.sg.decode(sigs[1])) is None
    coeffs = fixed_coeffs(1, 6) * 2
    want = model(v, keys, sigs, coeffs, sigs, [2])
    assert want[0] == bytes([VALID]) and run(eng, v, [b"both"] * 2, sigs, keys, coeffs, [2]) == want


PERIOD = 13


@pytest.fixture(scope="module")
def crowd(eng, v):
    """about 550 members in batches of lengths 0 .. 12 repeating, decode failures of every kind at distinct positions of a
    wave, wrong signatures among them; the model's verdicts and eccx_bls_verify's per member"""
    lengths = [i % PERIOD for i in range(7 * PERIOD)]
    n = sum(lengths) + 4   # four members belong to no batch
    made = Made(eng, v, n)
    msgs, keys, sigs, sks = list(made.msgs), list(made.keys), list(made.sigs), list(made.sks)
    s0 = made.sigs[0]
    plan = {5: ("sig", bytes([s0[0] & 0x7F]) + s0[1:]),          # flag bits
            70: ("sig", v.big_x_sig),                            # x >= p
            135: ("sig", v.no_point_sig),                        # no point with this x
            200: ("sig", v.off_sig),                             # outside the subgroup
            265: ("key", v.inf_key),                             # the identity key
            330: ("sig", v.inf_sig),                             # the identity signature: legal, the equation decides
            395: ("both", (v.inf_key, bytes([s0[0] & 0x7F]) + s0[1:])),   # MALFORMED together with BAD_KEY
            460: ("key", v.off_key),                             # a key outside the subgroup
            20: ("sig", made.sigs[21]),                          # another member's signature
            300: ("msg", b"not what was signed"),
            530: ("sig", made.sigs[0]),
            n - 2: ("sig", v.off_sig)}                           # outside every batch
    assert len({t % 64 for t in plan}) == len(plan)
    for t, (what, val) in plan.items():
        if what == "sig":
            sigs[t] = val
        elif what == "key":
            keys[t], sks[t] = val, None
        elif what == "both":
            keys[t], sks[t], sigs[t] = val[0], None, val[1]
        else:
            msgs[t] = val
    honest = honest_for(eng, v, sks, msgs, v.dst)
    coeffs = fixed_coeffs(n, 7)
    want = model(v, keys, sigs, coeffs, honest, lengths)
    single = eng.bls_verify(msgs, b"".join(sigs), b"".join(keys), v.dst, min_sig=v.min_sig)
    return dict(n=n, lengths=lengths, msgs=msgs, keys=keys, sigs=sigs, coeffs=coeffs, want=want, single=single)


def test_agreement_with_the_model_and_with_bls_verify(eng, v, crowd):
    c = crowd
    got = run(eng, v, c["msgs"], c["sigs"], c["keys"], c["coeffs"], c["lengths"])
    assert got == c["want"]
    single = c["single"]
    assert set(single) == {VALID, INVALID, MALFORMED, BAD_KEY}
    # member_status is the fold of eccx_bls_verify's MALFORMED / BAD_KEY verdicts on the same triples
    assert got[1] == bytes(s if s in (MALFORMED, BAD_KEY) else VALID for s in single)
    # a batch is VALID exactly where every member is VALID under eccx_bls_verify (true of these coefficients: the model
    # above has checked them)
    offs = np.concatenate(([0], np.cumsum(c["lengths"]))).astype(int)
    for b, (lo, hi) in enumerate(zip(offs, offs[1:])):
        assert (got[0][b] == VALID) == all(s == VALID for s in single[lo:hi]), b
    assert {MALFORMED, BAD_KEY, INVALID, VALID} == set(got[0])


def test_dev_form(eng, torch_mod, v, crowd):
    """a decreasing batch offset is MALFORMED alone and the batches before it stand; a range leaving n; a side stream; calls of
    549, 65 and 549 members back to back; repeatability"""
    torch = torch_mod
    c = crowd
    n, nb = c["n"], len(c["lengths"])
    flat, moffs = eng._ragged(c["msgs"])
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    bo = np.concatenate(([0], np.cumsum(c["lengths"]))).astype(np.int64) + 9   # relative to batch_offsets[0]
    args = lambda m, k: (d(flat), torch.from_numpy(moffs[:m + 1].astype(np.int64)).cuda(), d(b"".join(c["sigs"][:m])),
                         d(b"".join(c["keys"][:m])), d(b"".join(c["coeffs"][:m])), torch.from_numpy(bo[:k + 1].copy()).cuda())
    side = torch.cuda.Stream()
    n549 = n - 1
    k549 = nb       # every batch lies within the first 549 members (the last four belong to none)
    k65 = max(k for k in range(nb + 1) if bo[k] - 9 <= 65)
    a549, a65 = args(n549, k549), args(65, k65)
    torch.cuda.synchronize()
    outs = [eng.bls_batch_verify_t(*a, v.dst, min_sig=v.min_sig, stream=side.cuda_stream) for a in (a549, a65, a549)]
    side.synchronize()
    outs = [(x.cpu().numpy().tobytes(), y.cpu().numpy().tobytes()) for x, y in outs]
    assert outs[0] == (c["want"][0], c["want"][1][:n549]) and outs[2] == outs[0]
    assert outs[1] == (c["want"][0][:k65], c["want"][1][:65])
    # a decreasing offset at the end: the last batch is MALFORMED alone and every batch before it stands
    bad = bo.copy()
    bad[nb] = bad[nb - 1] - 1
    got = eng.bls_batch_verify_t(*args(n549, nb)[:5], torch.from_numpy(bad).cuda(), v.dst, min_sig=v.min_sig)
    torch.cuda.synchronize()
    got = got[0].cpu().numpy().tobytes()
    assert got[nb - 1] == MALFORMED and got[:nb - 1] == c["want"][0][:nb - 1]
    # ... and in the middle: batch k is MALFORMED; batch k + 1 now starts one member early and shares it with the last
    # non-empty batch before k, so those two are not specified; every other batch stands
    bad = bo.copy()
    k = 40
    assert c["lengths"][k - 1] == 0 and c["lengths"][k - 2] > 0
    bad[k + 1] = bad[k] - 1
    got = eng.bls_batch_verify_t(*args(n549, nb)[:5], torch.from_numpy(bad).cuda(), v.dst, min_sig=v.min_sig)
    torch.cuda.synchronize()
    got = got[0].cpu().numpy().tobytes()
    assert got[k] == MALFORMED and got[:k - 2] == c["want"][0][:k - 2] and got[k + 2:] == c["want"][0][k + 2:]
    # the last range leaves the n members: MALFORMED alone
    far = bo.copy()
    far[nb] = 9 + n549 + 1
    got = eng.bls_batch_verify_t(*args(n549, nb)[:5], torch.from_numpy(far).cuda(), v.dst, min_sig=v.min_sig)
    torch.cuda.synchronize()
    got = got[0].cpu().numpy().tobytes()
    assert got[nb - 1] == MALFORMED and got[:nb - 1] == c["want"][0][:nb - 1]
    # message offsets that decrease at one member: that member and its batch are MALFORMED
    mo = moffs.astype(np.int64).copy()
    t = 100
    mo[t] = mo[t + 1] + 2
    a = args(n549, nb)
    got = eng.bls_batch_verify_t(a[0], torch.from_numpy(mo[:n549 + 1]).cuda(), *a[2:], v.dst, min_sig=v.min_sig)
    torch.cuda.synchronize()
    b_of_t = int(np.searchsorted(bo - 9, t, side="right")) - 1
    assert got[1].cpu().numpy().tobytes()[t] == MALFORMED and got[0].cpu().numpy().tobytes()[b_of_t] == MALFORMED


@pytest.mark.parametrize("lengths", [[5], [1, 2, 3, 4, 5], [64], [63], [70, 0, 3]], ids=lambda x: "+".join(map(str, x)))
def test_dev_form_few_batches_before_a_decreasing_offset(eng, torch_mod, v, lengths):
    """a few valid batches and then an offset that decreases by one: the last batch is MALFORMED alone and the batch right
    before it keeps EVERY member in its sum (an honest one is VALID, one with a wrong signature INVALID), whatever the number
    of batches.  Expected verdicts of the valid batches are the model's."""
    torch = torch_mod
    n = sum(lengths)
    made = Made(eng, v, n)
    coeffs = fixed_coeffs(n, 10 + n)
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    flat, moffs = eng._ragged(made.msgs)
    bo = np.concatenate(([0], np.cumsum(lengths), [n - 1])).astype(np.int64) + 3
    for tamper in (None, n - 1, 0):   # nothing; the last member of the batch before the bad offset; the first member
        sigs = list(made.sigs)
        if tamper is not None:
            sigs[tamper] = made.sigs[(tamper + 1) % n] if n > 1 else v.inf_sig
        want = model(v, made.keys, sigs, coeffs, made.sigs, lengths)
        if tamper is None:
            assert want[0] == bytes([VALID]) * len(lengths)
        else:
            assert INVALID in want[0]
        got = eng.bls_batch_verify_t(d(flat), torch.from_numpy(moffs.astype(np.int64)).cuda(), d(b"".join(sigs)), d(b"".join(made.keys)),
                                     d(b"".join(coeffs)), torch.from_numpy(bo).cuda(), v.dst, min_sig=v.min_sig)
        torch.cuda.synchronize()
        assert got[0].cpu().numpy().tobytes() == want[0] + bytes([MALFORMED]), (lengths, tamper)
        assert got[1].cpu().numpy().tobytes() == want[1]


def test_other_inputs(eng, v):
    """a zero coefficient, a member outside every batch, empty and 200-byte messages, a 300-byte tag"""
    tag = bytes(range(256)) + b"x" * 44
    msgs = [b"", bytes(range(200)), b"m2", b"", b"m4", b"m5"]
    made = Made(eng, v, 6, msgs=msgs, dst=tag)
    coeffs = fixed_coeffs(6, 8)
    want = model(v, made.keys, made.sigs, coeffs, made.sigs, [2, 2, 1])
    assert want == (bytes([VALID]) * 3, bytes([VALID]) * 6)
    assert run(eng, v, msgs, made.sigs, made.keys, coeffs, [2, 2, 1], dst=tag) == want
    assert run(eng, v, msgs, made.sigs, made.keys, coeffs, [2, 2, 1])[0] == bytes([INVALID]) * 3   # the standard tag: another hash
    # a zero coefficient: MALFORMED for its batch alone
    zc = list(coeffs)
    zc[2] = bytes(8)
    want = model(v, made.keys, made.sigs, zc, made.sigs, [2, 2, 1])
    assert want == (bytes([VALID, MALFORMED, VALID]), bytes([VALID, VALID, MALFORMED, VALID, VALID, VALID]))
    assert run(eng, v, msgs, made.sigs, made.keys, zc, [2, 2, 1], dst=tag) == want
    # the member outside every batch (the last) has a status and touches no verdict
    sigs = list(made.sigs)
    sigs[5] = v.off_sig
    want = model(v, made.keys, sigs, coeffs, made.sigs, [2, 2, 1])
    assert want == (bytes([VALID]) * 3, bytes([VALID]) * 5 + bytes([MALFORMED]))
    assert run(eng, v, msgs, sigs, made.keys, coeffs, [2, 2, 1], dst=tag) == want
    # batches=None is one batch of everything; no batches at all leaves the statuses
    assert run(eng, v, msgs, sigs, made.keys, coeffs, None, dst=tag) == (bytes([MALFORMED]), want[1])
    assert run(eng, v, msgs, sigs, made.keys, coeffs, [], dst=tag) == (b"", want[1])
    # no members: every batch is empty and VALID
    assert eng.bls_batch_verify([], b"", b"", tag, batches=[0, 0], coeffs=b"", min_sig=v.min_sig) == (bytes([VALID]) * 2, b"")


def test_reserve_covers_the_dev_call(torch_mod, eng, v):
    torch = torch_mod
    lengths = [1, 9, 0, 2, 17] * 4
    n = sum(lengths)
    made = Made(eng, v, n)
    d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    flat, moffs = eng._ragged(made.msgs)
    bo = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    coeffs = fixed_coeffs(n, 9)
    args = (d(flat), torch.from_numpy(moffs.astype(np.int64)).cuda(), d(b"".join(made.sigs)), d(b"".join(made.keys)), d(b"".join(coeffs)),
            torch.from_numpy(bo).cuda())
    with E.Engine(0) as fresh:
        fresh.reserve("bls12_381_g2", n + len(lengths), var=False, bls_batch=True)
        before = fresh.device_bytes()
        assert before > 0
        got = fresh.bls_batch_verify_t(*args, v.dst, min_sig=v.min_sig)
        few = fresh.bls_batch_verify_t(args[0], args[1][:4], args[2][:3 * v.sb], args[3][:3 * v.kb], args[4][:24],
                                       torch.tensor([0, 1, 3], dtype=torch.int64).cuda(), v.dst, min_sig=v.min_sig)
        torch.cuda.synchronize()
        assert fresh.device_bytes() == before
        assert got[0].cpu().numpy().tobytes() == bytes([VALID]) * len(lengths) and got[1].cpu().numpy().tobytes() == bytes([VALID]) * n
        assert few[0].cpu().numpy().tobytes() == bytes([VALID, VALID])
    # ECCX_PREP_BLS and ECCX_PREP_BLS_AGGREGATE reserve exactly what they did before: the batch slab is a slab of its own
    with E.Engine(0) as a, E.Engine(0) as b:
        a.reserve("bls12_381_g2", 64, var=False, bls=True, bls_aggregate=True)
        b.reserve("bls12_381_g2", 64, var=False, bls=True, bls_aggregate=True, bls_batch=True)
        assert b.device_bytes() > a.device_bytes()


def test_argument_checks_write_nothing(eng, v):
    lib, ctx = eng._lib, eng._ctx
    ms = EN.BLS_MIN_SIG if v.min_sig else 0
    err = lambda: lib.eccx_last_error(ctx).decode()
    made = Made(eng, v, 1, msgs=[b"abc"])
    msg, dst, sig, key, co = b"abc", v.dst, made.sigs[0], made.keys[0], (5).to_bytes(8, "big")
    offs = np.array([0, 3], dtype=np.uint64)
    one = np.array([0, 1], dtype=np.uint64)
    o, g = offs.ctypes.data, one.ctypes.data
    st, mst = ctypes.create_string_buffer(b"\x5a", 1), ctypes.create_string_buffer(b"\x5a", 1)
    call = lambda *a: lib.eccx_bls_batch_verify(ctx, *a)
    assert call(1, msg, o, dst, len(dst), sig, key, co, 1, g, st, mst, ms) == 0 and st.raw + mst.raw == bytes([VALID, VALID])
    assert call(1, msg, o, dst, len(dst), sig, key, co, 1, g, st, None, ms) == 0 and st.raw == bytes([VALID])   # member_status is optional
    st.raw = mst.raw = b"\x5a"
    for bad in (EN.VALIDATE_POINTS, EN.CT_SCAN, EN.CT_GATHER, EN.CHECK_SUBGROUP, 1 << 18, 1 << 31):
        assert call(1, msg, o, dst, len(dst), sig, key, co, 1, g, st, mst, ms | bad) == ERR_ARG and "opts" in err()
        assert lib.eccx_bls_batch_verify_dev(ctx, 0, None, None, None, 0, None, None, None, 0, None, None, None, ms | bad, None) == ERR_ARG
    for hole in (5, 6, 7, 9, 10, 2):   # sigs, pubkeys, coeffs, batch offsets, verdicts, message offsets
        a = [1, msg, o, dst, len(dst), sig, key, co, 1, g, st, mst, ms]
        a[hole] = None
        assert call(*a) == ERR_ARG and "null buffer" in err(), hole
    assert call(1, None, o, dst, len(dst), sig, key, co, 1, g, st, mst, ms) == ERR_ARG and "null buffer" in err()
    assert call(1, msg, o, None, 3, sig, key, co, 1, g, st, mst, ms) == ERR_ARG and "null buffer" in err()
    down = np.array([3, 0], dtype=np.uint64)
    assert call(1, msg, down.ctypes.data, dst, len(dst), sig, key, co, 1, g, st, mst, ms) == ERR_ARG and "decrease" in err()
    assert call(1, msg, o, dst, len(dst), sig, key, co, 1, np.array([1, 0], dtype=np.uint64).ctypes.data, st, mst, ms) == ERR_ARG and "decrease" in err()
    assert call(1, msg, o, dst, len(dst), sig, key, co, 1, np.array([0, 2], dtype=np.uint64).ctypes.data, st, mst, ms) == ERR_ARG and "beyond" in err()
    assert call(1 << 30, msg, o, dst, len(dst), sig, key, co, 1, g, st, mst, ms) == ERR_ARG and "2^30" in err()
    assert lib.eccx_bls_batch_verify_dev(ctx, 1, None, None, None, 0, None, None, None, 1, None, None, None, ms, None) == ERR_ARG and "null buffer" in err()
    assert st.raw + mst.raw == b"\x5a\x5a"
    assert call(0, None, None, None, 0, None, None, None, 0, None, None, None, ms) == 0
    assert lib.eccx_bls_batch_verify_dev(ctx, 0, None, None, None, 0, None, None, None, 0, None, None, None, ms, None) == 0


def test_engine_draws_the_coefficients(eng, v):
    """coeffs=None: the engine draws them; only VALID / INVALID is asserted (the coefficients differ from run to run)"""
    made = Made(eng, v, 9)
    assert eng.bls_batch_verify(made.msgs, b"".join(made.sigs), b"".join(made.keys), v.dst, min_sig=v.min_sig) == \
        (bytes([VALID]), bytes([VALID]) * 9)
    sigs = list(made.sigs)
    sigs[4] = made.sigs[5]
    assert eng.bls_batch_verify(made.msgs, b"".join(sigs), b"".join(made.keys), v.dst, batches=[3, 3, 3], min_sig=v.min_sig)[0] == \
        bytes([VALID, INVALID, VALID])
