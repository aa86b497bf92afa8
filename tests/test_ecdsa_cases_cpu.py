"""The crafted ECDSA signatures of tests/ecdsa_cases.py against the Python model (tests/ecdsa_ref.py): every record's
model verdict is the one its constructor promises, the forced (u1, u2) are what the verifier computes, and no group is
short of what tests/test_ecdsa_edges_gpu.py relies on."""
import collections

import pytest

from tests import ecdsa_cases as X
from tests import ecdsa_ref as E

CURVES = list(E.CURVES)


def _z(c, rec):
    return int.from_bytes(rec.digest, "big") if rec.digest_bytes == 0 else E.digest_to_scalar(c, rec.digest)


@pytest.mark.parametrize("curve", CURVES)
def test_model_agrees_with_every_constructor(curve):
    c = E.CURVES[curve]
    keys, recs = X.cases(curve)
    assert [E.mul(c, d) for d, _ in keys] == [Q for _, Q in keys]
    assert [d for d, _ in keys][:3] == [1, c.n - 1, 2] and keys[1][1] == (c.gx, c.p - c.gy)
    for rec in recs:
        assert len(rec.digest) == (rec.digest_bytes or c.sb) and rec.digest_bytes <= 2 * c.sb
        Q = keys[rec.key][1]
        hashed = rec.digest_bytes == 0
        assert E.verdict(c, rec.digest, rec.sig, E.key_bytes(c, Q), hashed=hashed) == rec.want, rec
        assert E.verdict(c, rec.digest, rec.sig, E.key_sec1(c, Q), sec1=True, hashed=hashed) == rec.want, rec
        r, s = int.from_bytes(rec.sig[: c.sb], "big"), int.from_bytes(rec.sig[c.sb:], "big")
        if rec.pair is not None:
            assert E.u1u2(c, _z(c, rec), r, s) == rec.pair, rec
            t = (rec.pair[0] + rec.pair[1] * keys[rec.key][0]) % c.n
            assert rec.want == (E.SIG_VALID if t else E.SIG_INVALID)


@pytest.mark.parametrize("curve", CURVES)
def test_every_listed_case_is_there(curve):
    c = E.CURVES[curve]
    n, qlen = c.n, c.n.bit_length()
    keys, recs = X.cases(curve)
    assert {r.group for r in recs} == set(X.GROUPS)
    by = collections.defaultdict(list)
    for r in recs:
        by[(r.group, r.key)].append(r)
    forced = {(r.key, r.pair) for r in recs if r.pair is not None}
    assert len(forced) >= 100
    n_small = len(X.small_u2(c))
    assert n_small == 23 and len(X.forced_s_values(c)) == 11
    for ki, (d, _) in enumerate(keys):
        col = by[("collision", ki)]
        assert {r.want for r in col} == {E.SIG_VALID, E.SIG_INVALID}
        assert len({r.label for r in col}) == 27 and len({r.pair for r in col}) == 27
        for r in col:                                   # u2 Q is m G for the m the label names
            u1, u2 = r.pair
            m = u2 * d % n
            assert u1 in (m, n - m, 0)
        assert sum(1 for r in col if r.pair[0] == 0) >= 9
        # one comb entry: a single non-zero 16-bit (and 8-bit) digit, for the six listed multiples
        singles = {u2 * d % n for _, u2 in {r.pair for r in col} if bin(u2 * d % n).count("1") <= 16}
        assert {1, 200, 7 << 8, 65535 << 16, 255 << 40, 3 << (8 * (c.sb - 2))} <= singles
        assert {r.pair for r in by[("pairs", ki)]} == {(0, 1), (0, n - 1), (1, 1), (n - 1, n - 1), (1, n - 1), (n - 1, 1)}
        # (1, n - 1) and (n - 1, 1) under Q = G, (1, 1) and (n - 1, n - 1) under Q = -G sum to the identity
        want_inv = {1: {(1, n - 1), (n - 1, 1)}, n - 1: {(1, 1), (n - 1, n - 1)}}.get(d, set())
        assert {r.pair for r in by[("pairs", ki)] if r.want == E.SIG_INVALID} == want_inv
        small = by[("small_u2", ki)]
        assert {r.pair[1] for r in small} == set(X.small_u2(c)) and all(r.want == E.SIG_VALID for r in small)
        fs = by[("forced_s", ki)]
        assert {int.from_bytes(r.sig[c.sb:], "big") for r in fs} == set(X.forced_s_values(c))
        assert all(r.want == E.SIG_VALID for r in fs)
        dg = by[("digest", ki)]
        assert len(dg) == 4 * 5 and sum(1 for r in dg if r.want == E.SIG_INVALID) == 4
        assert all((r.want == E.SIG_INVALID) == r.label.endswith("wrong prefix") for r in dg)
        sh = 8 * c.sb - qlen
        prefixes = [int.from_bytes(r.digest[: c.sb], "big") >> sh for r in dg]
        assert sum(1 for v in prefixes if v >= n) >= 8 + 4 and max(prefixes) == (1 << qlen) - 1
        assert {r.digest_bytes for r in dg} == {c.sb, 2 * c.sb}
        for r in dg:                                    # every bit bits2int drops is set
            assert int.from_bytes(r.digest[: c.sb], "big") & ((1 << sh) - 1) == (1 << sh) - 1
            assert r.digest[c.sb:] == b"\xff" * (r.digest_bytes - c.sb)
    # every forced pair comes as a scalar and as at least one digest
    for r in recs:
        if r.pair is not None and r.digest_bytes == 0:
            assert any(o.pair == r.pair and o.key == r.key and o.digest_bytes != 0 for o in by[(r.group, r.key)])
    if curve == "p521r1":
        assert {r.digest_bytes for r in recs} == {0, 65, 66, 132}
    else:
        assert {r.digest_bytes for r in recs} == {0, c.sb, 2 * c.sb}


def test_constructors_refuse_what_they_cannot_build():
    c = E.CURVES["p256r1"]
    with pytest.raises(ValueError):
        X.force_pair(c, 5, 1, 0)
    with pytest.raises(ValueError):
        X.force_s(c, 5, 7, 0)
    with pytest.raises(ValueError):
        X.digest_with_prefix(c, 1 << 256)
    z, r, s, want = X.force_pair(c, 5, 0, 9)
    assert z == 0 and want == E.SIG_VALID and E.verify_hashed(c, E.mul(c, 5), z, r, s)
    z, r, s, want = X.force_s(c, 5, 11, c.n - 1)
    assert s == c.n - 1 and E.verify_hashed(c, E.mul(c, 5), z, r, s)
