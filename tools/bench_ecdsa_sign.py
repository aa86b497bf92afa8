#!/usr/bin/env python3
"""Throughput of batched ECDSA signing and key derivation on one GPU, inputs resident in HBM, beside the bare
secret-scalar fixed-base comb they run on the same scalars in the same process: one JSON line per curve, operation and
lookup form.

usage: python tools/bench_ecdsa_sign.py [--curves p256r1,p384r1,p521r1,p256k1] [--log2n N] [--steps 10] [--warmup 2]
                                        [--label default]

  comb[_gather]        eccx_scalarmul_base_dev under ECCX_CT_SCAN (| ECCX_CT_GATHER) on the nonces: the yardstick
  sign[_gather]        eccx_ecdsa_sign_dev on 32-byte digests (48 on p384r1, 64 on p521r1)
  public_key[_gather]  eccx_ecdsa_public_key_dev

n is 2^20 on the 256-bit curves and 2^19 on p384r1 and p521r1 unless --log2n says otherwise.  Every signature timed must
verify (eccx_ecdsa_verify_dev under the keys derived here) and the first 64 lanes are compared with Python integers
before a number is printed; a process that misses either exits 1.  Average, minimum and maximum over --steps launches
timed with events after --warmup.  The sign rows carry the cost over the bare comb of the same run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIGEST_BYTES = {"p256r1": 32, "p384r1": 48, "p521r1": 64, "p256k1": 32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="p256r1,p384r1,p521r1,p256k1")
    ap.add_argument("--log2n", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--label", default="default")
    args = ap.parse_args()
    import numpy as np
    import torch

    import eccoxide_amd as E
    from eccoxide_amd import workload as W
    from tests import ecdsa_ref as M

    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)

    def fail(why):
        print(json.dumps({"error": why}), flush=True)
        eng.close()
        sys.exit(1)

    for curve in args.curves.split(","):
        c = M.CURVES[curve]
        sb, fb, db = c.sb, c.fb, DIGEST_BYTES[curve]
        n = 1 << (args.log2n or (20 if sb == 32 else 19))
        rng = np.random.default_rng(6979)
        d_np = W.random_scalars(curve, n, seed=41).reshape(n, sb)
        k_np = W.random_scalars(curve, n, seed=42).reshape(n, sb)
        dig_np = rng.integers(0, 256, size=(n, db), dtype=np.uint8)
        d, k, dig = (torch.from_numpy(a.reshape(-1)).to(dev) for a in (d_np, k_np, dig_np))
        eng.prepare(curve, base=True, ct=True, ct_gather=True)
        eng.reserve(curve, n, ecdsa=True, ecdsa_sign=True)
        out = torch.empty((n * 2 * fb,), dtype=torch.uint8, device=dev)
        fl = torch.empty((n,), dtype=torch.uint8, device=dev)
        sig = torch.empty((n * 2 * sb,), dtype=torch.uint8, device=dev)
        st = torch.empty((n,), dtype=torch.uint8, device=dev)
        pk = torch.empty((n * 2 * fb,), dtype=torch.uint8, device=dev)
        verdicts = torch.empty((n,), dtype=torch.uint8, device=dev)
        keys, kst = eng.ecdsa_public_key_t(curve, d)
        torch.cuda.synchronize(dev)
        if not bool((kst == E.SIGN_OK).all()):
            fail(f"{curve}: a key was refused")
        results = {}

        def timed(name, fn, ok_fn, unit):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize(dev)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for a, b in ev:
                a.record(stream)
                fn()
                b.record(stream)
            torch.cuda.synchronize(dev)
            ms = [a.elapsed_time(b) for a, b in ev]
            avg = sum(ms) / len(ms)
            if not ok_fn():
                fail(f"{curve} {name}: results do not check")
            results[name] = avg
            row = {"metric": f"ecdsa {curve} {name}", "label": args.label, "curve": curve, "n": n, "kernel_ms": avg, "min_ms": min(ms),
                   "max_ms": max(ms), "steps": args.steps, "warmup": args.warmup, "parity_ok": True, "unit": unit,
                   "value": n / (avg * 1e-3)}
            comb = results.get("comb_gather" if name.endswith("_gather") else "comb")
            if comb is not None and not name.startswith("comb"):
                row["comb_ms"] = comb
                row["over_comb_ms"] = avg - comb
                row["over_comb_ratio"] = avg / comb
            if name.startswith("sign"):
                row["digest_bytes"] = db
            print(json.dumps(row), flush=True)

        def sig_ok():
            eng.ecdsa_verify_t(curve, dig, sig, keys, verdicts, digest_bytes=db)
            torch.cuda.synchronize(dev)
            if not (bool((verdicts == E.SIG_VALID).all()) and bool((st == E.SIGN_OK).all())):
                return False
            s_np = sig[: 64 * 2 * sb].cpu().numpy().reshape(64, 2 * sb)
            for i in range(64):
                di, ki = int.from_bytes(d_np[i].tobytes(), "big"), int.from_bytes(k_np[i].tobytes(), "big")
                rs = M.sign_hashed(c, di, ki, M.digest_to_scalar(c, dig_np[i].tobytes()))
                if rs is None or M.sig_bytes(c, *rs) != s_np[i].tobytes():
                    return False
            return True

        def pk_ok():
            if not (bool((pk == keys).all()) and bool((st == E.SIGN_OK).all())):
                return False
            p_np = pk[: 64 * 2 * fb].cpu().numpy().reshape(64, 2 * fb)
            return all(M.key_bytes(c, M.mul(c, int.from_bytes(d_np[i].tobytes(), "big"))) == p_np[i].tobytes() for i in range(8))

        for gather in (False, True):
            g = "_gather" if gather else ""
            timed(f"comb{g}", lambda: eng.scalarmul_base_t(curve, k, out.view(n, 2 * fb), fl, ct_scan=True, ct_gather=gather),
                  lambda: int(fl.sum()) == 0, "multiplications/s")
            timed(f"sign{g}", lambda: eng.ecdsa_sign_t(curve, dig, d, k, sig, st, digest_bytes=db, ct_gather=gather), sig_ok, "signatures/s")
            timed(f"public_key{g}", lambda: eng.ecdsa_public_key_t(curve, d, pk, st, ct_gather=gather), pk_ok, "keys/s")
    eng.close()


if __name__ == "__main__":
    main()
