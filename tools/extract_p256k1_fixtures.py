#!/usr/bin/env python3
"""Extract the secp256k1 (eccoxide's `p256k1`) golden data from the reference tree (read AS
TEXT, nothing is compiled or executed) into tests/golden/p256k1.json.

    python tools/extract_p256k1_fixtures.py [/root/reference]

What is extracted:
  * curve constants        src/params/sec2.rs, `mod p256k1`
  * the 100 k*G vectors    src/tests/sage.rs, `mod p256k1` KATS (k, x, y)
  * the comb table         src/params/comb/p256k1.rs: a SHA-256 over the whole table plus a
                           few sampled windows (the engine regenerates the table itself)

The fixture is DATA (inputs and expected outputs); no reference source text is stored.  The
other fixtures (tools/extract_fixtures.py) are left as they are.
"""
import hashlib
import json
import os
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "p256k1.json")

HEXBYTE = re.compile(r"0x([0-9a-fA-F]{2})\b")


def read(rel):
    with open(os.path.join(REF, rel), "r") as f:
        return f.read()


def bytes_of(txt):
    return bytes(int(h, 16) for h in HEXBYTE.findall(txt))


def const_bytes(txt, name):
    m = re.search(r"const %s: \[u8; \d+\] = \[(.*?)\];" % name, txt, re.S)
    assert m, name
    return bytes_of(m.group(1)).hex()


def params():
    sec2 = read("src/params/sec2.rs")
    m = re.search(r"pub mod p256k1 \{(.*?)\n\}", sec2, re.S)
    body = m.group(1)
    return {k.lower(): const_bytes(body, k + "_BYTES") for k in ("P", "ORDER", "A", "B", "B3", "GX", "GY")}


def sage_kats():
    txt = read("src/tests/sage.rs")
    start = txt.index("mod p256k1")
    body = txt[start: txt.index("\n    ];", start)]
    kats = re.findall(r"KAT\s*\{\s*n:\s*(\d+),\s*x:\s*\[([^\]]*)\],\s*y:\s*\[([^\]]*)\],?\s*\}", body)
    out = []
    for n, xs, ys in kats:
        x, y = bytes_of(xs), bytes_of(ys)
        assert len(x) == 32 and len(y) == 32, n
        out.append({"k": int(n), "x": x.hex(), "y": y.hex()})
    assert len(out) == 100
    return out


def comb():
    txt = read("src/params/comb/p256k1.rs")
    nw = int(re.search(r"COMB_WINDOWS: usize = (\d+);", txt).group(1))
    start = txt.index("pub static COMB_TABLE")
    start = txt.index("= [", start)
    end = txt.index("\n];", start)
    entries = re.findall(r"\(\[([^\]]*)\],\s*\[([^\]]*)\]\)", txt[start:end])
    assert len(entries) == nw * 15, (len(entries), nw)
    h = hashlib.sha256()
    pts = []
    for xs, ys in entries:
        x, y = bytes_of(xs), bytes_of(ys)
        assert len(x) == 32 and len(y) == 32
        h.update(x)
        h.update(y)
        pts.append((x.hex(), y.hex()))
    sample_windows = sorted({0, 1, nw // 2, nw - 1})
    return {
        "windows": nw,
        "field_bytes": 32,
        "byte_order": "big",
        "sha256_xy_concat": h.hexdigest(),
        "samples": {str(w): [list(pts[w * 15 + j]) for j in range(15)] for w in sample_windows},
    }


def main():
    data = {"params": params(), "sage_kg": sage_kats(), "comb": comb()}
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.normpath(OUT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
