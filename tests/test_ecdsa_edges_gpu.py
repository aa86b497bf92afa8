"""The crafted signatures of tests/ecdsa_cases.py through eccx_ecdsa_verify[_dev]: forced (u1, u2) that make the fused
ladder's two halves collide (doubling branch, identity), leave one half at infinity, or keep the accumulator at infinity
through the leading windows; forced s at the inverse's edges; digests at and above n.  Verdicts against the model
(tests/ecdsa_ref.py), lane for lane, with ordinary signatures in between, through affine and SEC1 keys and the
device-tensor form, and with each case filling a whole wavefront."""
import collections

import pytest

from tests import ecdsa_cases as X
from tests import ecdsa_ref as E

pytestmark = pytest.mark.gpu

CURVES = list(E.CURVES)


def _batches(curve):
    """{digest_bytes: records}, crafted and ordinary lanes alternating (so they share wavefronts)."""
    keys, recs = X.cases(curve)
    by = collections.defaultdict(list)
    for r in recs:
        by[r.digest_bytes].append(r)
    out = {}
    for db, special in by.items():
        plain = X.ordinary(curve, len(special) + 3, 1, db)
        mixed = [plain[-1], plain[-2], plain[-3]]
        for s, o in zip(special, plain):
            mixed += [s, o]
        out[db] = mixed
    return keys, out


def _pack(c, keys, recs):
    D = b"".join(r.digest for r in recs)
    S = b"".join(r.sig for r in recs)
    K = b"".join(E.key_bytes(c, keys[r.key][1]) for r in recs)
    K1 = b"".join(E.key_sec1(c, keys[r.key][1]) for r in recs)
    return D, S, K, K1


def _mismatches(recs, want, got):
    return [(i, recs[i].group, recs[i].label, recs[i].key, recs[i].digest_bytes, want[i], got[i])
            for i in range(len(recs)) if want[i] != got[i]][:12]


@pytest.mark.parametrize("curve", CURVES)
def test_crafted_signatures_among_ordinary_ones(engine, curve):
    import torch

    c = E.CURVES[curve]
    keys, batches = _batches(curve)
    stream = torch.cuda.Stream()
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    groups = collections.Counter()
    for db, recs in batches.items():
        # the model's verdict for every lane, and the constructor's promise
        want = [E.verdict(c, r.digest, r.sig, E.key_bytes(c, keys[r.key][1]), hashed=db == 0) for r in recs]
        assert want == [r.want for r in recs]
        groups.update((r.group, w) for r, w in zip(recs, want))
        D, S, K, K1 = _pack(c, keys, recs)
        got = list(engine.ecdsa_verify(curve, D, S, K, digest_bytes=db))
        assert got == want, (curve, db, _mismatches(recs, want, got))
        got = list(engine.ecdsa_verify(curve, D, S, K1, digest_bytes=db, sec1=True))
        assert got == want, (curve, db, "sec1", _mismatches(recs, want, got))
        with torch.cuda.stream(stream):
            td, ts, tk, tk1 = t(D), t(S), t(K), t(K1)
            va = engine.ecdsa_verify_t(curve, td, ts, tk, digest_bytes=db, stream=stream.cuda_stream)
            vs = engine.ecdsa_verify_t(curve, td, ts, tk1, digest_bytes=db, sec1=True, stream=stream.cuda_stream)
        stream.synchronize()
        va, vs = va.cpu().tolist(), vs.cpu().tolist()
        assert va == want, (curve, db, "dev", _mismatches(recs, want, va))
        assert vs == want, (curve, db, "dev sec1", _mismatches(recs, want, vs))
    assert groups[("collision", E.SIG_VALID)] and groups[("collision", E.SIG_INVALID)] and groups[("digest", E.SIG_INVALID)]
    assert all(groups[(g, E.SIG_VALID)] for g in X.GROUPS) and groups[("ordinary", E.SIG_VALID)]


@pytest.mark.parametrize("curve", CURVES)
def test_each_crafted_signature_fills_a_wavefront(engine, curve):
    """64 copies of one case per wavefront: the wave-uniform branches (the doubling in ucomb_accumulate) are taken by every
    lane at once, and by none in the ordinary wavefronts in between."""
    c = E.CURVES[curve]
    keys, recs = X.cases(curve)
    by = collections.defaultdict(list)
    for r in recs:
        by[r.digest_bytes].append(r)
    for db, special in by.items():
        plain = X.ordinary(curve, 64, 2, db)
        lanes = []
        for i, s in enumerate(special):
            lanes += [s] * 64
            if i % 8 == 7:
                lanes += plain
        lanes += plain[:5]                               # the batch does not end on a wavefront
        want = [r.want for r in lanes]                   # (equal to the model's: tests/test_ecdsa_cases_cpu.py)
        D, S, K, K1 = _pack(c, keys, lanes)
        got = list(engine.ecdsa_verify(curve, D, S, K, digest_bytes=db))
        assert got == want, (curve, db, _mismatches(lanes, want, got))
        got = list(engine.ecdsa_verify(curve, D, S, K1, digest_bytes=db, sec1=True))
        assert got == want, (curve, db, "sec1", _mismatches(lanes, want, got))
