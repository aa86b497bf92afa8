#!/usr/bin/env python3
"""Extract the data of hashing to BLS12-381 G2 (RFC 9380 section 8.8.2) from the reference tree (read AS TEXT, nothing
is compiled or executed) into tests/golden/bls_h2c_g2.json.

    python tools/extract_h2c_g2_fixtures.py <reference-root>      (or ECCX_REFERENCE=<reference-root>)

What is extracted:
  * the appendix J.10 vectors   src/curve/bls12_381/hash_to_curve_vectors.rs, G2_RO and G2_NU: the tag and five
                                vectors each (msg, the field elements u, the mapped points q, the result p)
  * the constants of the map    src/params/bls12_381_h2c.rs, `mod g2`: A' = 240u, B' = 1012(1 + u), Z = -(2 + u), the
                                exponent c3 and the constants c6, c7 of sqrt_ratio (appendix F.2.1.1), and the appendix
                                E.3 coefficients of the 3-isogeny (4, 2, 4 and 3 entries)
  * h_eff                       src/curve/bls12_381/g2.rs, the 80-byte H_EFF of its tests

Field elements are hex of c1 || c0 (48 bytes big-endian each), the exponents plain big-endian.  The fixture is DATA; no
reference source text is stored.
"""
import json
import os
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ECCX_REFERENCE", "reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "bls_h2c_g2.json")

HEXBYTE = re.compile(r"0x([0-9a-fA-F]{2})\b")


def read(rel):
    with open(os.path.join(REF, rel), "r") as f:
        return f.read()


def bytes_of(txt):
    return bytes(int(h, 16) for h in HEXBYTE.findall(txt))


def const_bytes(txt, name, size):
    m = re.search(r"const %s: \[u8; %d\] = \[(.*?)\];" % (name, size), txt, re.S)
    assert m, name
    b = bytes_of(m.group(1))
    assert len(b) == size, name
    return b.hex()


def vectors():
    vec = read("src/curve/bls12_381/hash_to_curve_vectors.rs")
    out = {}
    for name in ("G2_RO", "G2_NU"):
        dst = re.search(r'pub const %s_DST: &str = "([^"]*)";' % name, vec).group(1)
        m = re.search(r"pub const %s: &\[Vector\] = &\[(.*?)\n\];" % name, vec, re.S)
        assert m, name
        vs = []
        for v in re.finditer(r'msg: "([^"]*)",\s*u: &\[(.*?)\],\s*q: &\[(.*?)\],\s*p: \("([0-9a-f]+)", "([0-9a-f]+)"\)', m.group(1), re.S):
            vs.append({"msg": v.group(1), "u": re.findall(r'"([0-9a-f]+)"', v.group(2)),
                       "q": [list(t) for t in re.findall(r'\("([0-9a-f]+)",\s*"([0-9a-f]+)"\)', v.group(3))],
                       "p": [v.group(4), v.group(5)]})
        count = 2 if name == "G2_RO" else 1
        assert len(vs) == 5 and all(len(v["u"]) == len(v["q"]) == count for v in vs), name
        assert all(len(h) == 192 for v in vs for h in v["u"] + v["p"] + sum(v["q"], []))
        out[name.lower()] = {"dst": dst, "vectors": vs}
    return out


def constants():
    par = read("src/params/bls12_381_h2c.rs")
    g2 = par[par.index("pub mod g2 {"):]
    c = {}
    for key, name in (("iso_a", "ISO_A_BYTES"), ("iso_b", "ISO_B_BYTES"), ("z", "ISO_Z_BYTES"), ("c3", "SQRT_RATIO_C3_BYTES"),
                      ("c6", "SQRT_RATIO_C6_BYTES"), ("c7", "SQRT_RATIO_C7_BYTES")):
        c[key] = const_bytes(g2, name, 96)
    for key, name, count in (("k1", "ISO_K1_BYTES", 4), ("k2", "ISO_K2_BYTES", 2), ("k3", "ISO_K3_BYTES", 4), ("k4", "ISO_K4_BYTES", 3)):
        m = re.search(r"const %s: \[\[u8; 96\]; %d\] = \[(.*?)\n    \];" % (name, count), g2, re.S)
        assert m, name
        raw = bytes_of(m.group(1))
        assert len(raw) == 96 * count, name
        c[key] = [raw[96 * i:96 * i + 96].hex() for i in range(count)]
    c["note"] = ("field elements are c1 || c0; c3 is an exponent, plain big-endian; k1 = x_num, k2 = x_den, k3 = y_num, "
                 "k4 = y_den ascend in x', the denominators monic (the leading 1 is not stored)")
    return c


def main():
    data = vectors()
    data["constants"] = constants()
    data["h_eff"] = const_bytes(read("src/curve/bls12_381/g2.rs"), "H_EFF", 80)
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    size = os.path.getsize(OUT)
    assert size < 64 * 1024, size
    print("wrote", os.path.normpath(OUT), size, "bytes")


if __name__ == "__main__":
    main()
