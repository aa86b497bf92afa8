"""X448 without a GPU: the Python model (tests/x448_ref.py) reproduces the RFC 7748 vectors of tests/golden/x448.json
and the section 5.2 iteration, holds the facts the crafted units of tests/x448_cases.py rely on, and agrees with an
independent affine double-and-add; the two entry points are declared, bound and mirrored alike in include/eccx.h,
eccoxide_amd/_lib.py and the Rust crate; a null context is refused before a device is touched."""
import collections
import ctypes
import json
import os
import random
import re

from tests import x448_cases as X
from tests import x448_ref as R
from tests.oracle_lib import ROOT


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "x448.json")) as f:
        return json.load(f)


def test_model_reproduces_rfc7748_vectors():
    g = _golden()
    assert len(g["rfc7748"]) == 2
    for v in g["rfc7748"]:
        assert R.x448(bytes.fromhex(v["k"]), bytes.fromhex(v["u"])).hex() == v["r"]
    dh = {k: bytes.fromhex(v) for k, v in g["diffie_hellman"].items()}
    assert R.x448_base(dh["a"]) == dh["a_pub"] and R.x448_base(dh["b"]) == dh["b_pub"]
    assert R.x448(dh["a"], dh["b_pub"]) == dh["shared"] == R.x448(dh["b"], dh["a_pub"])


def test_model_reproduces_rfc7748_iteration():
    """RFC 7748 section 5.2: k = u = 5, then k, u = X448(k, u), k"""
    k = u = X.BASE_U
    for i in range(1000):
        k, u = R.x448(k, u), k
        if i == 0:
            assert k.hex() == X.RFC_ITER_1
    assert k.hex() == X.RFC_ITER_1000


def test_facts_the_cases_rely_on():
    X.check_facts()
    assert R.P == 2**448 - 2**224 - 1 and R.P % 4 == 3 and 4 * R.A24 == R.A + 2
    # non-canonical u: p .. 2^448 - 1 (2^224 + 1 values) are taken modulo p
    assert 2**448 - R.P == 2**224 + 1
    k = bytes(range(56))
    for j in (0, 5, 2**224):
        assert R.x448(k, R.le(R.P + j)) == R.x448(k, R.le(j))
    assert R.ladder(R.P + 7, b"\x01") == 7


def test_case_sets_are_complete():
    for raw in (False, True):
        groups = collections.Counter(c.group for c in X.cases(raw))
        assert groups["twist"] == 4 and groups["clamp"] == 16 and groups["non_canonical"] == 26
        assert groups["low_order"] == (25 if raw else 15)
        assert groups["extreme"] == (20 if raw else 4)
        if raw:
            assert sum(1 for c in X.cases(raw) if c.group == "bit" and c.u is not None) == 448
        else:
            assert groups["bit"] == 2 * len(X.RFC_BITS)
        for with_u in (False, True):
            assert X.select(raw, with_u)
            per = X.periodic(raw, with_u)
            assert len(per) == 97 and {f for _, f in map(X.expected, per)} == ({0, 1} if raw or with_u else {0})
        assert all(X.on_twist(int.from_bytes(c.u, "little")) for c in X.cases(raw) if c.group == "twist")
    # clamp: the eight settings of bits 0, 1 and 447 give one output per scalar under RFC clamping
    by = {c.label: X.expected(c) for c in X.cases(False) if c.group == "clamp"}
    assert all(len({by[f"s{s} m{m}"] for m in range(8)}) == 1 for s in range(2))
    raw_by = {c.label: X.expected(c) for c in X.cases(True) if c.group == "clamp"}
    assert len(set(raw_by.values())) == 16
    # 2^t for a clamped t is the scalar 0 after clamping
    rfc = {(c.group, c.label): X.expected(c) for c in X.cases(False)}
    for tag in ("u", "base"):
        assert all(rfc[("bit", f"2^{t} {tag}")] == rfc[("extreme", f"k=0x0 {tag}")] for t in X.CLAMPED_BITS)
    assert X.evaluations() <= 1500


def test_low_order_and_extremes():
    for raw in (False, True):
        for c in X.cases(raw):
            if c.group == "low_order":
                k = int.from_bytes(c.scalar, "big" if raw else "little")
                out, flag = X.expected(c)
                if not raw or k % 4 == 0:
                    assert (out, flag) == (X.ZERO, 1)
                elif k % 2:
                    assert out == R.le(int.from_bytes(c.u, "little") % R.P) and flag == (1 if out == X.ZERO else 0)
        units = X.low_order_units(raw, 300)
        assert X.want(units) == (bytes(56 * 300), b"\1" * 300)
    ext = {c.label: X.expected(c) for c in X.cases(True) if c.group == "extreme"}
    u = X.shared_u(True)
    assert ext["k=0x0 base"] == ext[f"k={R.L:#x} base"] == ext[f"k={4 * R.L:#x} base"] == (X.ZERO, 1)
    assert ext["k=0x1 base"] == ext[f"k={R.L + 1:#x} base"] == ext[f"k={R.L - 1:#x} base"] == (X.BASE_U, 0)
    assert ext["k=0x1 u"] == (u, 0) and ext["k=0x0 u"] == (X.ZERO, 1) and ext[f"k={4 * R.L:#x} u"][1] in (0, 1)


def test_model_against_affine_double_and_add():
    """recover v by a square root on the curve, multiply (u, v) by double-and-add, compare u"""
    rng = random.Random(448)
    done = 0
    while done < 16:
        u = rng.randrange(2, R.P - 1)
        v = R.sqrt(R.rhs(u))
        if v is None:
            continue
        k = rng.getrandbits(448)
        pt = R.affine_mul(k, (u, v))
        assert R.ladder(u, k.to_bytes(56, "big")) == (0 if pt is None else pt[0])
        done += 1


def _params(txt, name):
    m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*(?:;|->)" % name, txt, re.S)
    assert m, name
    return [p for p in m.group(1).split(",") if p.strip()]


def test_symbols_in_header_ffi_and_ctypes():
    from eccoxide_amd import _lib
    from eccoxide_amd import engine as EN

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eccx.h")).read(), flags=re.S)
    ffi = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust", "eccoxide-gpu", "src", "ffi.rs")).read())
    for name, count in (("eccx_x448", 7), ("eccx_x448_dev", 8)):
        assert len(_params(hdr, name)) == count and len(_params(ffi, name)) == count
        assert len(_lib.SYMBOLS[name][1]) == count
    assert re.search(r"ECCX_X448_RAW_LADDER\s*=\s*1u\s*<<\s*4\b", hdr) and re.search(r"ECCX_PREP_X448\s*=\s*1u\s*<<\s*13\b", hdr)
    assert re.search(r"ECCX_X448_RAW_LADDER: u32 = 1 << 4;", ffi) and re.search(r"ECCX_PREP_X448: u32 = 1 << 13;", ffi)
    assert EN.X448_RAW_LADDER == 1 << 4 and EN.PREP_X448 == 1 << 13
    rs = open(os.path.join(ROOT, "rust", "eccoxide-gpu", "src", "x448.rs")).read()
    assert re.search(r"pub fn x448_batch\(ctx: &GpuContext, scalars: &\[\[u8; 56\]\], us: Option<&\[\[u8; 56\]\]>\)", rs)
    assert "pub mod x448;" in open(os.path.join(ROOT, "rust", "eccoxide-gpu", "src", "lib.rs")).read()


def test_null_context_is_refused_without_a_device():
    from eccoxide_amd import _lib

    lib = _lib.load()
    k, out, fl = bytes(56), ctypes.create_string_buffer(56), ctypes.create_string_buffer(1)
    assert lib.eccx_x448(None, 1, k, k, out, fl, 0) == -2
    assert lib.eccx_x448(None, 0, None, None, None, None, 0) == -2
    assert lib.eccx_x448_dev(None, 1, None, None, None, None, 0, None) == -2
    assert lib.eccx_x448_dev(None, 0, None, None, None, None, 0, None) == -2
