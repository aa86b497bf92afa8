#!/usr/bin/env python3
"""Extract the X448 golden data from the reference tree (read AS TEXT, nothing is compiled or
executed) into tests/golden/x448.json.

    python tools/extract_x448_fixtures.py [path/to/reference]

What is extracted: the three RFC 7748 vectors of src/protocol/x448.rs's test module -- section 5.2
vectors 1 and 2 (scalar, u, result) and the section 6.2 exchange (both secret keys, both public keys,
the shared secret).  The fixture is DATA (inputs and expected outputs); no reference source text is
stored.  The other fixtures (tools/extract_fixtures.py) are left as they are.
"""
import json
import os
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "x448.json")


def main():
    with open(os.path.join(REF, "src", "protocol", "x448.rs")) as f:
        txt = f.read()
    tests = txt[txt.index("mod tests"):]

    def body(name):
        start = tests.index("fn %s()" % name)
        return tests[start:tests.index("\n    }", start)]

    hexes = lambda s: re.findall(r'"([0-9a-f]{112})"', s)
    vectors = []
    for name in ("rfc7748_vector1", "rfc7748_vector2"):
        k, u, r = hexes(body(name))
        vectors.append({"k": k, "u": u, "r": r})
    a, b, a_pub, b_pub, shared = hexes(body("diffie_hellman_agrees"))
    data = {"rfc7748": vectors, "diffie_hellman": {"a": a, "b": b, "a_pub": a_pub, "b_pub": b_pub, "shared": shared}}
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.relpath(OUT), "-", len(vectors), "vectors and the exchange")


if __name__ == "__main__":
    main()
