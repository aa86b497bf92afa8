"""eccx_reserve against the calls it promises to cover: on a fresh context, with every table of the curve prepared and one
reserve(max_n) with every flag the curve supports, no device-resident or host-buffer call of max_n units grows a buffer
(eccx_device_bytes stays where the reserve left it) and each returns the reference's bytes.  The sizes eccx_reserve
computes and the sizes the launch paths ask for must agree for this to hold; n = 300 is more than one workgroup of 256,
and ragged.

Not covered by ECCX_PREP_HOST, and not run here (the device-resident forms of the same calls are):
  - the un-normalised X:Y:Z of the reference-mirroring kernels (`want_proj`): their device-side copy, 3 or 4 FB bytes per
    unit in slot IO_J, is wider than the SB bytes the flag sizes there for the second scalar of the verify shape;
  - the host-buffer eccx_ed25519_public_key, and eccx_ed25519_sign with supplied keys: both keep 32 bytes per unit in slot
    IO_A, which the flag sizes at one byte per unit (the infinity flags of the group law), so their first call grows it."""
import random

import pytest

from eccoxide_amd import workload as W
from oracle import ecc_ref as R
from tests import ecdsa_ref as EC, ecdsa_sign_ref as ES, ed25519_ref as ED, p256k1_ref as K

pytestmark = pytest.mark.gpu

N = 300
CURVES = ["p256r1", "p384r1", "p521r1", "bls12_381_g1", "ed25519", "p256k1"]
ECDSA_CURVES = ("p256r1", "p384r1", "p521r1", "p256k1")


def _params(curve):
    return R.ED25519 if curve == "ed25519" else K.K1 if curve == "p256k1" else R.CURVES[curve]


PERIOD = 56


def _split(b, w):
    return [b[i: i + w] for i in range(0, len(b), w)]


def _rep(block, lanes=PERIOD):
    """The records of `lanes` lanes repeated to N lanes."""
    return (block * (N // lanes + 1))[: len(block) // lanes * N]


def _ref_mul(oracle, curve, ks, pts=None):
    """(x || y, flags) of ks[i] * pts[i] (pts None: the generator): the C oracle, or for p256k1, which it does not have,
    the Python model's windowed multiplication (a cached table per base point: the callers use few distinct bases)."""
    if curve != "p256k1":
        return (oracle.base(curve, ks, threads=8) if pts is None else oracle.var(curve, ks, pts, threads=8))[:2]
    bases = [None] * (len(ks) // 32) if pts is None else [(int.from_bytes(p[:32], "big"), int.from_bytes(p[32:], "big"))
                                                          for p in _split(pts, 64)]
    recs = [K.affine_bytes(EC.mul(K.K1, int.from_bytes(k, "big"), P)) for k, P in zip(_split(ks, 32), bases)]
    return b"".join(r[0] for r in recs), bytes(r[1] for r in recs)


def _ref_add(curve, a, b):
    """(x || y, flags) of a[i] + b[i] for affine records without the point at infinity among them."""
    c = _params(curve)
    ed = curve == "ed25519"
    order = "little" if ed else "big"
    out, flags = [], []
    for ra, rb in zip(_split(a, 2 * c.fb), _split(b, 2 * c.fb)):
        P, Q = (tuple(int.from_bytes(r[i * c.fb:(i + 1) * c.fb], order) for i in (0, 1)) for r in (ra, rb))
        S = R.ed_affine_add(c, P, Q) if ed else R.affine_add(c, P, Q)
        flags.append(1 if S is None else 0)
        out.append(bytes(2 * c.fb) if S is None else S[0].to_bytes(c.fb, order) + S[1].to_bytes(c.fb, order))
    return b"".join(out), bytes(flags)


@pytest.mark.parametrize("curve", CURVES)
def test_reserve_covers_every_call(oracle, curve):
    import torch

    import eccoxide_amd as E

    c = _params(curve)
    sb, pb = c.sb, 2 * c.fb
    ed, ecdsa = curve == "ed25519", curve in ECDSA_CURVES
    ks = W.random_scalars(curve, N, seed=701).tobytes()
    ks2 = W.random_scalars(curve, N, seed=702).tobytes()
    few = _split(W.random_scalars(curve, 8, seed=703).tobytes(), sb)   # eight distinct bases, keys and secrets
    pts = _ref_mul(oracle, curve, b"".join(few))[0]
    pts = b"".join(_split(pts, pb)[i % 8] for i in range(N))
    want_b, want_v = _ref_mul(oracle, curve, ks), _ref_mul(oracle, curve, ks2, pts)
    want_add = _ref_add(curve, pts, want_b[0])
    want_dbl = _ref_add(curve, want_b[0], want_v[0])                   # ks * G + ks2 * pts
    want_enc = b"".join(K.compress((int.from_bytes(p[:32], "big"), int.from_bytes(p[32:], "big"))) for p in _split(pts, pb)) \
        if curve == "p256k1" else R.point_compress_bytes(curve, pts, None)
    zeros = bytes(N)

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()

    with E.Engine(0) as eng:
        eng.prepare(curve, base=True, base_lds=ed, ct=True, ct_gather=True)
        eng.reserve(curve, N, var=True, mirror=True, ct=True, host=True, ecdsa=ecdsa, ecdsa_sign=ecdsa, ed25519=ed,
                    ed25519_sign=ed)
        last = [eng.device_bytes()]
        grew, wrong = [], []

        def run(label, call, want):
            got = call()
            got = got if isinstance(got, tuple) else (got,)
            got = tuple(bytes(g.cpu().numpy().reshape(-1)) if hasattr(g, "cpu") else g for g in got)
            now = eng.device_bytes()
            print(f"{curve} {label}: device_bytes {now} ({now - last[0]:+d}), bytes {'ok' if got == want else 'DIFFER'}")
            if now != last[0]:
                grew.append((label, now - last[0]))
                last[0] = now
            if got != want:
                wrong.append(label)

        d_ks, d_ks2, d_pts, d_b = t(ks), t(ks2), t(pts), t(want_b[0])
        # variable base: default, endomorphism / subgroup form, secret scalars (both forms), reference-mirroring kernels
        for label, kw in (("default", {}), ("assume_subgroup", {"assume_subgroup": True}), ("ct", {"ct_scan": True}),
                          ("ct+assume_subgroup", {"ct_scan": True, "assume_subgroup": True}), ("mirror", {"mirror": True})):
            run(f"var {label}", lambda: eng.scalarmul_var(curve, ks2, pts, **kw), want_v)
            run(f"var_t {label}", lambda: eng.scalarmul_var_t(curve, d_ks2, d_pts, **kw), want_v)
        # fixed base: public (wide table, reference layout) and secret (scan, lane gather)
        for label, kw in (("default", {}), ("mirror", {"mirror": True}), ("ct", {"ct_scan": True}), ("ct_gather", {"ct_gather": True})):
            run(f"base {label}", lambda: eng.scalarmul_base(curve, ks, **kw), want_b)
            run(f"base_t {label}", lambda: eng.scalarmul_base_t(curve, d_ks, **kw), want_b)
        if ed:
            run("base_t table_in_lds", lambda: eng.scalarmul_base_t(curve, d_ks, table_in_lds=True), want_b)
        run("double", lambda: eng.double_scalarmul(curve, ks, ks2, pts), want_dbl)
        run("double_t", lambda: eng.double_scalarmul_t(curve, d_ks, d_ks2, d_pts), want_dbl)
        for mirror in (False, True):
            run(f"add mirror={mirror}", lambda: eng.point_add(curve, pts, want_b[0], mirror=mirror), want_add)
            run(f"add_t mirror={mirror}", lambda: eng.point_add_t(curve, d_pts, d_b, mirror=mirror), want_add)
        inf = None if ed else zeros
        run("compress", lambda: eng.point_compress(curve, pts, inf), (want_enc,))
        run("compress_t", lambda: eng.point_compress_t(curve, d_pts, None if ed else t(zeros)), (want_enc,))
        run("decompress", lambda: eng.point_decompress(curve, want_enc), (pts, zeros))
        run("decompress_t", lambda: eng.point_decompress_t(curve, t(want_enc)), (pts, zeros))

        if ecdsa:
            # the models are Python: PERIOD lanes of reference work (a multiple of the 8 keys and of the 7-lane pattern of
            # bad signatures), repeated over the batch
            rng = random.Random("reserve " + curve)
            b_secrets = b"".join(few[i % 8] for i in range(PERIOD))
            b_digests, b_nonces = rng.randbytes(32 * PERIOD), ks[:PERIOD * sb]
            keys = [ES.public_key_record(c, d) for d in _split(b_secrets, sb)]
            keys1 = [ES.public_key_record(c, d, sec1=True) for d in _split(b_secrets, sb)]
            recs = [ES.sign_record(c, dg, d, k) for dg, d, k in zip(_split(b_digests, 32), _split(b_secrets, sb), _split(b_nonces, sb))]
            b_sigs = bytearray(b"".join(r[0] for r in recs))
            for i in range(3, PERIOD, 7):                             # some signatures that do not verify
                b_sigs[(i + 1) * 2 * sb - 1] ^= 1
            b_ver = bytes(EC.verdict(c, dg, sg, ky[0]) for dg, sg, ky in zip(_split(b_digests, 32), _split(bytes(b_sigs), 2 * sb), keys))
            assert set(b_ver) >= {EC.SIG_VALID, EC.SIG_INVALID}
            secrets, digests, nonces, sigs = _rep(b_secrets), _rep(b_digests), _rep(b_nonces), _rep(bytes(b_sigs))
            want_keys = (_rep(b"".join(k[0] for k in keys)), _rep(bytes(k[1] for k in keys)))
            want_keys1 = (_rep(b"".join(k[0] for k in keys1)), _rep(bytes(k[1] for k in keys1)))
            want_sigs = (_rep(b"".join(r[0] for r in recs)), _rep(bytes(r[1] for r in recs)))
            want_ver = (_rep(b_ver),)
            d_sec, d_dig, d_sig, d_non = t(secrets), t(digests), t(sigs), t(nonces)
            run("ecdsa_public_key", lambda: eng.ecdsa_public_key(curve, secrets), want_keys)
            run("ecdsa_public_key sec1", lambda: eng.ecdsa_public_key(curve, secrets, sec1=True), want_keys1)
            run("ecdsa_public_key_t", lambda: eng.ecdsa_public_key_t(curve, d_sec), want_keys)
            run("ecdsa_public_key_t sec1", lambda: eng.ecdsa_public_key_t(curve, d_sec, sec1=True, ct_gather=True), want_keys1)
            run("ecdsa_sign", lambda: eng.ecdsa_sign(curve, digests, secrets, nonces, digest_bytes=32), want_sigs)
            run("ecdsa_sign ct_gather", lambda: eng.ecdsa_sign(curve, digests, secrets, nonces, digest_bytes=32, ct_gather=True), want_sigs)
            run("ecdsa_sign_t", lambda: eng.ecdsa_sign_t(curve, d_dig, d_sec, d_non, digest_bytes=32), want_sigs)
            run("ecdsa_verify", lambda: eng.ecdsa_verify(curve, digests, sigs, want_keys[0], digest_bytes=32), want_ver)
            run("ecdsa_verify sec1", lambda: eng.ecdsa_verify(curve, digests, sigs, want_keys1[0], digest_bytes=32, sec1=True), want_ver)
            run("ecdsa_verify_t", lambda: eng.ecdsa_verify_t(curve, d_dig, d_sig, t(want_keys[0]), digest_bytes=32), want_ver)
            run("ecdsa_verify_t sec1", lambda: eng.ecdsa_verify_t(curve, d_dig, d_sig, t(want_keys1[0]), digest_bytes=32, sec1=True), want_ver)

        if ed:
            seeds = [bytes((j * 37 + b * 11 + 5) & 0xFF for b in range(32)) for j in range(5)]
            model = [ED.expand_secret(s) for s in seeds]
            pub5 = [ED.encode(ED.mul(a)) for a, _ in model]
            # the model is Python: 35 lanes of reference work (5 seeds, the 7-lane pattern of bad signatures), repeated
            b_msgs = [b"reserve %d" % i for i in range(35)]
            b_msgs[1] = b""
            b_sig = bytearray(b"".join(ED.sign_with(*model[i % 5], pub5[i % 5], m) for i, m in enumerate(b_msgs)))
            want_sig = (_rep(bytes(b_sig), 35),)
            for i in range(3, 35, 7):                                 # some signatures that do not verify
                b_sig[64 * i + 40] ^= 1
            b_ver = bytes(ED.verdict(m, sg, pub5[i % 5]) for i, (m, sg) in enumerate(zip(b_msgs, _split(bytes(b_sig), 64))))
            assert set(b_ver) >= {ED.SIG_VALID, ED.SIG_INVALID}
            msgs = [b_msgs[i % 35] for i in range(N)]
            seedb, pubs = b"".join(seeds[i % 5] for i in range(N)), b"".join(pub5[i % 5] for i in range(N))
            sigs, want_ver = _rep(bytes(b_sig), 35), (_rep(b_ver, 35),)
            offs = [0]
            for m in msgs:
                offs.append(offs[-1] + len(m))
            d_msgs, d_offs, d_seeds, d_pubs = t(b"".join(msgs)), torch.tensor(offs, dtype=torch.int64).cuda(), t(seedb), t(pubs)
            run("ed25519_public_key_t", lambda: eng.ed25519_public_key_t(d_seeds), (pubs,))
            run("ed25519_public_key_t ct_gather", lambda: eng.ed25519_public_key_t(d_seeds, ct_gather=True), (pubs,))
            run("ed25519_sign", lambda: eng.ed25519_sign(msgs, seedb), want_sig)
            run("ed25519_sign_t", lambda: eng.ed25519_sign_t(d_msgs, d_offs, d_seeds), want_sig)
            run("ed25519_sign_t keys", lambda: eng.ed25519_sign_t(d_msgs, d_offs, d_seeds, d_pubs, ct_gather=True), want_sig)
            run("ed25519_verify", lambda: eng.ed25519_verify(msgs, sigs, pubs), want_ver)
            run("ed25519_verify_t", lambda: eng.ed25519_verify_t(d_msgs, d_offs, t(sigs), d_pubs), want_ver)
            u = oracle.x25519(ks2)[0]                                 # valid u-coordinates: multiples of the base point
            run("x25519 base", lambda: eng.x25519(ks), oracle.x25519(ks))
            run("x25519", lambda: eng.x25519(ks, u), oracle.x25519(ks, u))
            run("x25519_t", lambda: eng.x25519_t(d_ks, t(u)), oracle.x25519(ks, u))

        assert not wrong, f"{curve}: bytes differ from the reference in {wrong}"
        assert not grew, f"{curve}: a buffer grew after eccx_reserve in {grew}"
