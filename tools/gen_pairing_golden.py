#!/usr/bin/env python3
"""Writes tests/golden/bls_pairing.json from the Python model (tests/pairing_ref.py): a handful of pairing values as the
library's 576-byte encoding, inputs as the C ABI's records.  tests/test_pairing_cpu.py pins the model to the file.

    python tools/gen_pairing_golden.py > tests/golden/bls_pairing.json
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import pairing_ref as M  # noqa: E402

CASES = [[(1, 1)], [(2, 3)], [(7, 1)], [(0x9E3779B97F4A7C15, 0xDEADBEEF)], [(0x9E3779B97F4A7C15, 0x123456789ABCDEF0)],
         [(2, 3), (5, 7), (0x9E3779B97F4A7C15, 11)], []]


def main():
    out = []
    for case in CASES:
        terms = [(M.g1_mul(a), M.g2_mul(b)) for a, b in case]
        g1, _, g2, _ = M.term_records(terms)
        out.append({"scalars": [[hex(a), hex(b)] for a, b in case], "g1": g1.hex(), "g2": g2.hex(),
                    "value": M.f12_to_bytes(M.pairing_product(terms)).hex()})
    json.dump({"comment": "e([a]G1, [b]G2) products, written by tools/gen_pairing_golden.py from tests/pairing_ref.py",
               "cases": out}, sys.stdout, indent=1)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
