#!/usr/bin/env python3
"""Extract the BLS12-381 G2 golden data from the reference tree (read AS TEXT, nothing is
compiled or executed) into tests/golden/bls_g2.json.

    python tools/extract_g2_fixtures.py <reference-root>      (or ECCX_REFERENCE=<reference-root>)

What is extracted:
  * the parameters          src/params/bls12_381.rs, `mod g2`: b, 3b, generator, the two coefficients of psi
  * the serialization KATs  src/curve/bls12_381/g2.rs, `serialization_kat`: k with k*G compressed (and, where
                            the reference has it, uncompressed)
  * the off-subgroup pairs  src/curve/bls12_381/g2.rs, `OFF_SUBGROUP`: (compressed, uncompressed) of three points
                            of the twist outside G2
  * the comb table          src/params/comb/bls12_381_g2.rs: a SHA-256 over the whole table in its on-disk order
                            plus all 15 entries of the windows 0, 1, 31 and 63 (layout as comb_samples.json)

The fixture is DATA (inputs and expected outputs); no reference source text is stored.
"""
import hashlib
import json
import os
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ECCX_REFERENCE", "reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "bls_g2.json")

HEXBYTE = re.compile(r"0x([0-9a-fA-F]{2})\b")


def read(rel):
    with open(os.path.join(REF, rel), "r") as f:
        return f.read()


def bytes_of(txt):
    return bytes(int(h, 16) for h in HEXBYTE.findall(txt))


def const_bytes(txt, name):
    m = re.search(r"const %s: \[u8; \d+\] = \[(.*?)\];" % name, txt, re.S)
    assert m, name
    b = bytes_of(m.group(1))
    assert len(b) == 96, name
    return b.hex()


def params():
    txt = read("src/params/bls12_381.rs")
    body = txt[txt.index("pub mod g2 {"):]
    names = {"b": "B_BYTES", "b3": "B3_BYTES", "gx": "GX_BYTES", "gy": "GY_BYTES", "psi_x_coeff": "PSI_X_COEFF_BYTES",
             "psi_y_coeff": "PSI_Y_COEFF_BYTES"}
    return {k: const_bytes(body, v) for k, v in names.items()}


def int_of(lit):
    return int(lit.replace("_", ""), 0)


def kats(txt):
    start = txt.index("fn serialization_kat()")
    body = txt[start:]
    c0 = body.index("= &[", body.index("const COMPRESSED"))
    u0 = body.index("= &[", body.index("const UNCOMPRESSED"))
    end = body.index("for (k, expected)", u0)
    pair = re.compile(r"\(\s*([0-9a-fA-Fx_]+),\s*\[([^\]]*)\],?\s*\)")
    comp = {int_of(k): bytes_of(b) for k, b in pair.findall(body[c0:u0])}
    unc = {int_of(k): bytes_of(b) for k, b in pair.findall(body[u0:end])}
    assert len(comp) == 5 and len(unc) == 2, (len(comp), len(unc))
    out = []
    for k in sorted(comp):
        assert len(comp[k]) == 96
        e = {"k": k, "compressed": comp[k].hex()}
        if k in unc:
            assert len(unc[k]) == 192
            e["uncompressed"] = unc[k].hex()
        out.append(e)
    return out


def off_subgroup(txt):
    start = txt.index("= &[", txt.index("const OFF_SUBGROUP"))
    body = txt[start: txt.index("\n        ];", start)]
    pairs = re.findall(r"\(\s*\[([^\]]*)\],\s*\[([^\]]*)\],?\s*\)", body)
    assert len(pairs) == 3
    out = []
    for c, u in pairs:
        c, u = bytes_of(c), bytes_of(u)
        assert len(c) == 96 and len(u) == 192
        out.append({"compressed": c.hex(), "uncompressed": u.hex()})
    return out


def comb():
    txt = read("src/params/comb/bls12_381_g2.rs")
    nw = int(re.search(r"COMB_WINDOWS: usize = (\d+);", txt).group(1))
    start = txt.index("pub static COMB_TABLE")
    start = txt.index("= [", start)
    entries = re.findall(r"\(\s*\[([^\]]*)\],\s*\[([^\]]*)\],?\s*\)", txt[start:])
    assert len(entries) == nw * 15, (len(entries), nw)
    h = hashlib.sha256()
    pts = []
    for xs, ys in entries:
        x, y = bytes_of(xs), bytes_of(ys)
        assert len(x) == 96 and len(y) == 96
        h.update(x)
        h.update(y)
        pts.append((x.hex(), y.hex()))
    sample_windows = sorted({0, 1, nw // 2 - 1, nw - 1})
    return {
        "windows": nw,
        "field_bytes": 96,
        "byte_order": "big, c1 || c0",
        "sha256_xy_concat": h.hexdigest(),
        "samples": {str(w): [list(pts[w * 15 + j]) for j in range(15)] for w in sample_windows},
    }


def main():
    g2 = read("src/curve/bls12_381/g2.rs")
    data = {"params": params(), "serialization_kat": kats(g2), "off_subgroup": off_subgroup(g2), "comb": comb()}
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    size = os.path.getsize(OUT)
    assert size < 64 * 1024, size
    print("wrote", os.path.normpath(OUT), size, "bytes")


if __name__ == "__main__":
    main()
