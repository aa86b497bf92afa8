"""The model of BLS batch verification (tests/bls_batch_ref.py): its shortcuts against the literal pairing product on
batches of 0, 1 and 2 members in both variants, its short multiplication against repeated addition, and the library's side
of eccx_scalarmul_u64 / eccx_bls_batch_verify that needs no device: declarations in the header, the ctypes table and the
Rust bindings, constants, and the refusal of a null context with nothing written.  CPU only."""
import os
import re

import numpy as np

from tests import bls_batch_ref as BR
from tests import bls_sig_ref as B
from tests import g2_ref as G2
from tests import msm_ref as M
from tests.oracle_lib import ROOT

ERR_ARG = -2
SKS = [0x2B7E1516 << 190 | 77, 0x5B1C << 200 | 12345]
MSGS = [b"first", b""]


def _batch(min_sig, count):
    dst = B.DST_NUL_MIN_SIG if min_sig else B.DST_NUL
    kg, sg = B.groups(min_sig)
    sks, msgs = SKS[:count], MSGS[:count]
    keys = [kg.mul(s, kg.gen) for s in sks]
    sigs = [sg.mul(s, sg.hash(m, dst)) for s, m in zip(sks, msgs)]
    return dst, sg, sks, msgs, keys, sigs


def test_shortcuts_equal_the_literal_product():
    for min_sig in (False, True):
        for count in (0, 1, 2):
            dst, sg, sks, msgs, keys, sigs = _batch(min_sig, count)
            coeffs = [0xF00DFACE12345678, 3][:count]
            enc = [sg.compress(s) for s in sigs]
            assert BR.equation(keys, msgs, sigs, coeffs, dst, min_sig) == BR.VALID
            assert BR.shortcut(sks, msgs, sigs, coeffs, dst, min_sig) == BR.VALID
            assert BR.shortcut_honest(enc, enc, coeffs, min_sig) == BR.VALID
            if count == 0:
                continue
            # one signature replaced by another point of the group: all three say INVALID
            bad = list(sigs)
            bad[-1] = sg.add(bad[-1], sg.gen)
            assert BR.equation(keys, msgs, bad, coeffs, dst, min_sig) == BR.INVALID
            assert BR.shortcut(sks, msgs, bad, coeffs, dst, min_sig) == BR.INVALID
            assert BR.shortcut_honest([sg.compress(s) for s in bad], enc, coeffs, min_sig) == BR.INVALID
            # the identity signature is a legal point and refutes the batch
            gone = list(sigs)
            gone[0] = None
            assert BR.equation(keys, msgs, gone, coeffs, dst, min_sig) == BR.shortcut(sks, msgs, gone, coeffs, dst, min_sig) == BR.INVALID


def test_the_cancelling_forgery_in_the_model():
    """sig_1 + D and sig_2 - D pass the plain sum check (all coefficients 1) and fail with coefficients 1 and 2"""
    for min_sig in (False, True):
        dst, sg, sks, msgs, keys, sigs = _batch(min_sig, 2)
        d = sg.mul(0xD1FF, sg.gen)
        forged = [sg.add(sigs[0], d), sg.add(sigs[1], BR.neg(sg, d))]
        for coeffs, want in (([1, 1], BR.VALID), ([1, 2], BR.INVALID), ([1 << 56, 1 << 56], BR.VALID), ([1 | 1 << 56, 1], BR.INVALID)):
            assert BR.equation(keys, msgs, forged, coeffs, dst, min_sig) == want, coeffs
            assert BR.shortcut(sks, msgs, forged, coeffs, dst, min_sig) == want, coeffs
            assert BR.shortcut_honest([sg.compress(s) for s in forged], [sg.compress(s) for s in sigs], coeffs, min_sig) == want


def test_verdict_order_and_zero_coefficient():
    dst, sg, sks, msgs, keys, sigs = _batch(False, 2)
    pks = [B.sk_to_pk(s) for s in sks]
    enc = [sg.compress(s) for s in sigs]
    one = [(1).to_bytes(8, "big"), (2).to_bytes(8, "big")]
    assert BR.verdict(pks, enc, one, enc) == BR.VALID
    assert BR.verdict([], [], [], []) == BR.VALID
    assert BR.verdict(pks, enc, [one[0], bytes(8)], enc) == BR.MALFORMED
    inf_key = B.groups()[0].compress(None)
    assert BR.verdict([pks[0], inf_key], enc, one, [enc[0], None]) == BR.BAD_KEY
    broken = bytes([enc[0][0] & 0x7F]) + enc[0][1:]
    assert BR.verdict([pks[0], inf_key], [broken, enc[1]], one, [enc[0], None]) == BR.MALFORMED   # MALFORMED before BAD_KEY
    assert BR.verdict(pks, [enc[1], enc[0]], one, enc) == BR.INVALID
    assert BR.verdict(pks, enc, one, enc, bad_offsets=(1,)) == BR.MALFORMED


def test_scalarmul_u64_is_repeated_addition():
    off1, off2 = M.point_off_subgroup(), G2.point_of_x((1, 2))
    for group, pts in ((B._G1, [B._G1.gen, off1]), (B._G2, [B._G2.gen, off2])):
        for p in pts:
            acc = None
            for k in range(0, 20):
                assert BR.scalarmul_u64(group, k, p) == acc, k
                acc = group.add(acc, p)
        # in the subgroup the integer multiple is the multiple modulo r; 2^64 - 1 by doubling and subtracting
        g = group.gen
        for k in (1, 0xAAAAAAAAAAAAAAAA, (1 << 64) - 1):
            assert BR.scalarmul_u64(group, k, g) == group.mul((k + B.R) % B.R, g) == group.mul(k + B.R, g)
        top = g
        for _ in range(64):
            top = group.add(top, top)
        assert BR.scalarmul_u64(group, (1 << 64) - 1, g) == group.add(top, BR.neg(group, g))
        assert BR.scalarmul_u64(group, 5, None) is None and BR.scalarmul_u64(group, 0, g) is None


# ---- the library's side that needs no GPU ------------------------------------------------------------------------------
NEW = ("eccx_scalarmul_u64", "eccx_bls_batch_verify")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_declarations_in_header_ctypes_and_rust():
    import eccoxide_amd as E
    from eccoxide_amd import _lib
    from eccoxide_amd import engine as EN

    header, ffi = _read("include", "eccx.h"), _read("rust", "eccoxide-gpu", "src", "ffi.rs")
    lib = _lib.load()
    for base in NEW:
        for name in (base, base + "_dev"):
            assert re.search(r"\bint %s\(" % name, header), name
            assert re.search(r"\bpub fn %s\(" % name, ffi), name
            assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert len(_lib.SYMBOLS[base + "_dev"][1]) == len(_lib.SYMBOLS[base][1]) + 1  # the _dev form takes the stream on top
    assert re.search(r"ECCX_PREP_BLS_BATCH\s*=\s*1u\s*<<\s*18", header)
    assert re.search(r"ECCX_PREP_BLS_BATCH:\s*u32\s*=\s*1\s*<<\s*18", ffi)
    assert EN.PREP_BLS_BATCH == 1 << 18
    # the header says what the coefficients are and are not
    assert "COEFFICIENTS ARE PUBLIC" in header and "DETERMINISTIC FUNCTION OF THE INPUTS" in header
    for name in ("scalarmul_u64", "bls_batch_verify"):
        assert callable(getattr(E.Engine, name)) and callable(getattr(E.Engine, name + "_t")), name
    assert "secrets" in E.Engine.bls_batch_verify.__doc__


def test_drawn_coefficients_are_nonzero_and_fresh():
    import eccoxide_amd as E

    a, b = E.Engine.draw_batch_coeffs(64), E.Engine.draw_batch_coeffs(64)
    assert len(a) == len(b) == 512 and a != b
    assert all(any(a[8 * i:8 * i + 8]) for i in range(64))
    assert E.Engine.draw_batch_coeffs(0) == b""


def test_null_context_is_refused_and_nothing_is_written():
    """Without a device there is no context, so this pins only that: a null context is ECCX_ERR_ARG through all four entry
    points whatever the other arguments are, and no output byte is touched.  The rules for `opts` and for the curve id need
    a context and are checked in tests/test_bls_batch_gpu.py and tests/test_scalarmul_u64_gpu.py."""
    from eccoxide_amd import _lib
    from eccoxide_amd import engine as EN

    lib = _lib.load()
    offs = np.array([0, 1], dtype=np.uint64)
    o = offs.ctypes.data
    out = bytearray(b"\x5a" * 193)
    buf = (np.frombuffer(out, dtype=np.uint8)).ctypes.data
    for opts in (0, EN.BLS_MIN_SIG, EN.VALIDATE_POINTS, EN.CT_SCAN, 1 << 20):
        assert lib.eccx_bls_batch_verify(None, 1, b"m", o, None, 0, bytes(96), bytes(48), bytes(8), 1, o, buf, buf, opts) == ERR_ARG
        assert lib.eccx_bls_batch_verify_dev(None, 0, None, None, None, 0, None, None, None, 0, None, None, None, opts, None) == ERR_ARG
        for curve in (EN.BLS12_381_G1, EN.BLS12_381_G2, EN.P256R1, 99):
            assert lib.eccx_scalarmul_u64(None, curve, 1, bytes(8), bytes(192), None, buf, buf, opts) == ERR_ARG
            assert lib.eccx_scalarmul_u64_dev(None, curve, 0, None, None, None, None, None, opts, None) == ERR_ARG
    assert bytes(out) == b"\x5a" * 193
