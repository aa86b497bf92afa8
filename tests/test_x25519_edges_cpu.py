"""The crafted X25519 units of tests/x25519_cases.py on the CPU: what the builders promise about them holds in the
Python model (oracle/ecc_ref.py), the C oracle agrees with the model on every distinct unit in both modes and through
the base-point path, the model reproduces the RFC 7748 section 5.2 iteration, and the ladder agrees with the Edwards
group law on points with an 8-torsion component."""
import collections

from oracle import ecc_ref as R
from tests import ed25519_ref as ED
from tests import x25519_cases as X


def _by_label(raw, group):
    return {c.label: X.expected(c) for c in X.cases(raw) if c.group == group}


def test_case_sets_are_complete():
    for raw in (False, True):
        groups = collections.Counter(c.group for c in X.cases(raw))
        assert groups["bit"] == 512 and groups["clamp"] == 64 and groups["twist"] == 4
        assert groups["low_order"] == (30 if raw else 20)
        assert groups["non_canonical"] == (63 if raw else 38)
        assert groups["extreme"] == (20 if raw else 4)
        for with_u in (False, True):
            assert X.select(raw, with_u)
            per = X.periodic(raw, with_u)
            assert len(per) == 97 and {f for _, f in map(X.expected, per)} == ({0, 1} if raw or with_u else {0})
        assert all(X.on_twist(int.from_bytes(c.u, "little")) for c in X.cases(raw) if c.group == "twist")


def test_low_order_inputs():
    """raw mode: all ten give zero under a clamped scalar; RFC mode: the seven below 2^255 give zero under any scalar,
    the three above lose bit 255 and are ordinary points"""
    for raw in (False, True):
        for c in X.cases(raw):
            if c.group != "low_order":
                continue
            u = int.from_bytes(c.u, "little")
            out, flag = X.expected(c)
            if raw:
                k = int.from_bytes(c.scalar, "big")
                assert R.ref_ladder(u, (8 * k).to_bytes(33, "big")) == 0
                if k == X.clamp(k):
                    assert (out, flag) == (X.ZERO, 1)
            elif u < 2**255:
                assert (out, flag) == (X.ZERO, 1)
            else:
                assert flag == 0 and out == R.ref_x25519(c.scalar, X.le(u - 2**255))
    for raw in (False, True):
        units = X.low_order_units(raw, 300)
        assert X.want(units) == (bytes(32 * 300), b"\1" * 300)
        assert {c.u for c in units} == {X.le(u) for u in X.low_order_values(raw)}


def test_non_canonical_u():
    rfc = [X.expected(c)[0] for c in X.cases(False) if c.group == "non_canonical"]
    assert rfc[:19] == rfc[19:]                                    # bit 255 is masked
    k = next(c.scalar for c in X.cases(False) if c.group == "non_canonical")
    assert rfc[:19] == [R.ref_x25519(k, X.le(j)) for j in range(19)]   # p + j is j
    assert rfc[0] == X.ZERO and rfc[1] == X.ZERO and X.ZERO not in rfc[2:19]
    raw = [(c, X.expected(c)[0]) for c in X.cases(True) if c.group == "non_canonical"]
    for c, out in raw:                                             # any 256-bit string, modulo p
        u = int.from_bytes(c.u, "little")
        assert out == X.le(R.ref_ladder(u % X.P, c.scalar))
    assert {int.from_bytes(c.u, "little") for c, _ in raw} >= {2**255, 2 * X.P + 37, 2**256 - 1}


def test_scalar_bits_and_clamping():
    for raw in (False, True):
        bits, ext = _by_label(raw, "bit"), _by_label(raw, "extreme")
        assert len({bits[f"2^{t} u"] for t in range(256)}) == (252 if not raw else 256)
        if not raw:
            for t in (0, 1, 2, 255):                               # the clamp clears them: the zero scalar's output
                assert bits[f"2^{t} u"] == ext["k=0x0 u"] and bits[f"2^{t} base"] == ext["k=0x0 base"]
            assert bits["2^254 u"] == ext["k=0x0 u"]                # ... and sets this one
        clamp = _by_label(raw, "clamp")
        for s in range(2):
            outs = {clamp[f"s{s} m{m}"] for m in range(32)}
            assert len(outs) == (32 if raw else 1)


def test_raw_scalar_extremes():
    ext = _by_label(True, "extreme")
    nine = (X.BASE_U, 0)
    assert ext["k=0x0 base"] == (X.ZERO, 1) and ext[f"k={X.L:#x} base"] == (X.ZERO, 1)
    assert ext["k=0x1 base"] == nine and ext[f"k={X.L - 1:#x} base"] == nine and ext[f"k={X.L + 1:#x} base"] == nine
    assert ext[f"k={8 * X.L:#x} base"] == (X.ZERO, 1)


def test_c_oracle_matches_model_on_every_case(oracle):
    total = 0
    for raw in (False, True):
        for with_u in (False, True):
            units = X.interleaved(raw, with_u) + X.periodic(raw, with_u) + (X.low_order_units(raw, 30) if with_u else [])
            k, u = X.pack(units)
            got = oracle.x25519(k, u, rfc=not raw, threads=4)
            want = X.want(units)
            bad = [(i, units[i].group, units[i].label) for i in range(len(units))
                   if got[0][32 * i:32 * i + 32] != want[0][32 * i:32 * i + 32] or got[1][i] != want[1][i]]
            assert not bad, (raw, with_u, bad[:8])
            assert set(want[1]) == ({0, 1} if raw or with_u else {0})
            total += len(units)
    assert total > 2500 and X.evaluations() < 2000   # the model's budget: about 1500 distinct evaluations


def test_rfc7748_iteration_on_the_model():
    """RFC 7748 section 5.2: k = u = 9, then k, u = X25519(k, u), k"""
    k = u = X.BASE_U
    for i in range(1000):
        k, u = R.ref_x25519(k, u), k
        if i == 0:
            assert k.hex() == X.RFC_ITER_1
    assert k.hex() == X.RFC_ITER_1000


def test_ladder_matches_edwards_with_torsion():
    """curve25519.rs:1654-1665 extended to points outside the prime-order subgroup: the ladder's u([k]P) is the
    Montgomery u of the Edwards [k]P for P = [a]B + T and for T alone, T of order 1, 2, 4 and 8"""
    tors = ED.torsion()
    for i, T in enumerate(tors):
        for base in (T, ED.add(ED.mul(3 + i), T)):
            for k in (0, 1, 2, 3, 4, 7, 8, X.L, X.L + 1, 0xDEADBEEF1234567):
                want = X.montgomery_u(ED.mul(k, base))
                assert R.ref_ladder(X.montgomery_u(base), k.to_bytes(32, "big")) == want, (i, k)
