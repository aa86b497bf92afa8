#!/usr/bin/env python3
"""Throughput of batched ECDSA verification on one GPU, inputs resident in HBM: one JSON line per (curve, operation).

usage: python tools/bench_ecdsa.py [--log2n 20] [--steps 10] [--warmup 2] [--curves p256r1,p256k1,p384r1,p521r1]
                                   [--ops verify,verify_sec1,shape,shape_validate] [--label default]

  verify          eccx_ecdsa_verify_dev, affine keys
  verify_sec1     the same with SEC1 compressed keys (ECCX_PUBKEY_SEC1: the decoder runs first)
  shape           eccx_double_scalarmul_dev with ECCX_OUT_X_ONLY on the same u1, u2 and Q: the bare verify shape
  shape_validate  the same with ECCX_VALIDATE_POINTS, which ecdsa_verify always applies to the keys

2^log2n signatures on the 256-bit curves, half that on p384r1 / p521r1.  The signatures are made valid by construction:
random u1, u2 and keys, R = u1 G + u2 Q on the GPU, then r = x(R) mod n, s = r / u2, e = u1 s on the host; e goes in as
an SB-byte digest (bits2int leaves it as it is) on p256r1 / p256k1 / p384r1 and as a verify_hashed scalar
(digest_bytes 0) on p521r1, whose 66-byte digests are shifted.  Every timed verdict must be ECCX_SIG_VALID, and the
verify-shape output is checked against r.  Average over --steps launches timed with events after --warmup."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL_OPS = ["verify", "verify_sec1", "shape", "shape_validate"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--curves", default="p256r1,p256k1,p384r1,p521r1")
    ap.add_argument("--ops", default=",".join(ALL_OPS))
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
    for curve in args.curves.split(","):
        c = M.CURVES[curve]
        sb, fb = c.sb, c.fb
        n = 1 << (args.log2n if sb == 32 else args.log2n - 1)
        db = sb if 8 * sb <= c.n.bit_length() else 0
        d = torch.from_numpy(W.random_scalars(curve, n, seed=11)).to(dev)
        u1 = torch.from_numpy(W.random_scalars(curve, n, seed=12)).to(dev)
        u2 = torch.from_numpy(W.random_scalars(curve, n, seed=13)).to(dev)
        q, qfl = eng.scalarmul_base_t(curve, d)
        x, xfl = eng.double_scalarmul_t(curve, u1, u2, q, x_only=True)
        torch.cuda.synchronize(dev)
        assert int(qfl.sum()) == 0 and int(xfl.sum()) == 0
        xs, u1s, u2s = x.cpu().numpy(), u1.cpu().numpy(), u2.cpu().numpy()
        sig = np.zeros((n, 2 * sb), dtype=np.uint8)
        dig = np.zeros((n, sb), dtype=np.uint8)
        for i in range(n):
            r = int.from_bytes(xs[i].tobytes(), "big") % c.n
            a, b = int.from_bytes(u1s[i].tobytes(), "big"), int.from_bytes(u2s[i].tobytes(), "big")
            s = r * pow(b, -1, c.n) % c.n
            sig[i] = np.frombuffer(r.to_bytes(sb, "big") + s.to_bytes(sb, "big"), dtype=np.uint8)
            dig[i] = np.frombuffer((a * s % c.n).to_bytes(sb, "big"), dtype=np.uint8)
        sig_t, dig_t = torch.from_numpy(sig).to(dev), torch.from_numpy(dig).to(dev)
        sec = eng.point_compress_t(curve, q, qfl)
        eng.prepare(curve)
        eng.reserve(curve, n, ecdsa=True)
        verdicts = torch.empty((n,), dtype=torch.uint8, device=dev)
        xo, xofl = torch.empty_like(x), torch.empty_like(xfl)
        r_bytes = sig_t[:, :sb]
        all_valid = lambda: bool((verdicts == E.SIG_VALID).all())
        ops = {
            "verify": (lambda: eng.ecdsa_verify_t(curve, dig_t, sig_t, q, verdicts, digest_bytes=db), all_valid),
            "verify_sec1": (lambda: eng.ecdsa_verify_t(curve, dig_t, sig_t, sec, verdicts, digest_bytes=db, sec1=True), all_valid),
            # x(R) < n on all but a ~2^-128 (p256k1) or smaller fraction of the sample: compare bytes directly
            "shape": (lambda: eng.double_scalarmul_t(curve, u1, u2, q, xo, xofl, x_only=True),
                      lambda: bool((xo[:4096] == r_bytes[:4096]).all()) and int(xofl.sum()) == 0),
            "shape_validate": (lambda: eng.double_scalarmul_t(curve, u1, u2, q, xo, xofl, x_only=True, validate=True),
                               lambda: bool((xo[:4096] == r_bytes[:4096]).all()) and int(xofl.sum()) == 0),
        }
        for name in args.ops.split(","):
            fn, ok_fn = ops[name]
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
            ok = ok_fn()
            print(json.dumps({"metric": f"{curve} ecdsa {name}", "label": args.label, "value": n / (avg * 1e-3),
                              "unit": "verifications/s", "n": n, "digest_bytes": db, "kernel_ms": avg, "min_ms": min(ms),
                              "max_ms": max(ms), "steps": args.steps, "warmup": args.warmup, "parity_ok": ok}), flush=True)
            if not ok:
                eng.close()
                sys.exit(1)
    eng.close()


if __name__ == "__main__":
    main()
