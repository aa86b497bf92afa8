#!/usr/bin/env python3
"""Throughput of the Jubjub entry points on one GPU, inputs resident in HBM, and the same operations on edwards25519 in
the same process as the yardstick: one JSON line per (curve, operation) and one ratio line per operation.

usage: python tools/bench_jubjub.py [--log2n 20] [--steps 5] [--warmup 1] [--label default]

  var        eccx_scalarmul_var_dev, default ladder          var-ct   ... with ECCX_CT_SCAN
  base       eccx_scalarmul_base_dev, 16-bit-window table    base-l2  the reference's 64 x 15 comb    base-ct  ECCX_CT_SCAN
  verify     eccx_double_scalarmul_dev with ECCX_SUBTRACT    decompress / compress   the point codecs

The n units are a periodic tiling of 256 distinct ones (any point of the curve for jubjub, small-order components among
them).  Every output and flag of every timed configuration is compared ON THE DEVICE with the tiling of the expectation
for those 256 units: for jubjub the big-integer model (tests/jubjub_ref.py); for edwards25519 the engine's own
reference-mirroring kernels on the 256 units (which the test suite pins to the oracle).  Averages over --steps launches
timed with events after --warmup."""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TILE = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--label", default="default")
    args = ap.parse_args()
    import numpy as np
    import torch

    import eccoxide_amd as E
    from eccoxide_amd import workload as W
    from tests import jubjub_ref as J

    if not torch.cuda.is_available():
        sys.exit("tools/bench_jubjub.py needs a GPU")
    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)
    n = 1 << args.log2n
    idx = np.arange(n) % TILE

    def tiled(b, width):
        return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).reshape(TILE, width)[idx].copy()).to(dev)

    def expectations(curve):
        """Scalars, points and what each operation must return for the 256 units of the tile."""
        rng = random.Random(20)
        k = W.random_scalars(curve, TILE, seed=7).tobytes()
        u1 = W.random_scalars(curve, TILE, seed=8).tobytes()
        if curve == "jubjub":
            small = J.small_order_points(rng)
            pts = [J.random_point(rng) for _ in range(TILE - 4)] + [J.add(J.G, small[8]), small[4], J.neg(J.G), J.G]
            ks = [int.from_bytes(k[32 * i:32 * i + 32], "big") for i in range(TILE)]
            u1s = [int.from_bytes(u1[32 * i:32 * i + 32], "big") for i in range(TILE)]
            p = b"".join(map(J.point_bytes, pts))
            var = b"".join(map(J.point_bytes, J.mul_many(pts, ks)))
            base = b"".join(map(J.point_bytes, J.mul_many([J.G] * TILE, ks)))
            ver = b"".join(map(J.point_bytes, J.double_mul_many(u1s, ks, pts, True)))
            enc = b"".join(map(J.compress, pts))
        else:
            p = eng.scalarmul_base(curve, W.random_scalars(curve, TILE, seed=9).tobytes(), mirror=True)[0]
            var = eng.scalarmul_var(curve, k, p, mirror=True)[0]
            base = eng.scalarmul_base(curve, k, mirror=True)[0]
            neg = eng.point_add(curve, eng.scalarmul_base(curve, u1, mirror=True)[0], var, subtract=True, mirror=True)[0]
            ver = neg
            enc = eng.point_compress(curve, p)
        return {"k": k, "u1": u1, "p": p, "var": var, "base": base, "verify": ver, "enc": enc}

    results, failed = {}, False
    for curve in ("jubjub", "ed25519"):
        x = expectations(curve)
        eng.prepare(curve, base=True, ct=True)
        eng.reserve(curve, n, var=True, ct=True)
        k, u1, p, enc = tiled(x["k"], 32), tiled(x["u1"], 32), tiled(x["p"], 64), tiled(x["enc"], 32)
        out = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        out32 = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        fl = torch.empty((n,), dtype=torch.uint8, device=dev)
        zero = torch.zeros((n,), dtype=torch.uint8, device=dev)
        w_var, w_base, w_ver = tiled(x["var"], 64), tiled(x["base"], 64), tiled(x["verify"], 64)
        # flag 1 where the result is the neutral element (0, 1) -- a small-order base times a multiple of its order
        neutral = bytes(32) + ((1).to_bytes(32, "big") if curve == "jubjub" else (1).to_bytes(32, "little"))
        flags_of = lambda b: tiled(bytes(1 if b[64 * i:64 * i + 64] == neutral else 0 for i in range(TILE)), 1).reshape(n)
        f_var, f_base, f_ver = flags_of(x["var"]), flags_of(x["base"]), flags_of(x["verify"])
        configs = [
            ("var", lambda: eng.scalarmul_var_t(curve, k, p, out, fl), out, w_var, f_var),
            ("var-ct", lambda: eng.scalarmul_var_t(curve, k, p, out, fl, ct_scan=True), out, w_var, f_var),
            ("base", lambda: eng.scalarmul_base_t(curve, k, out, fl), out, w_base, f_base),
            ("base-l2", lambda: eng.scalarmul_base_t(curve, k, out, fl, table_in_lds=False), out, w_base, f_base),
            ("base-ct", lambda: eng.scalarmul_base_t(curve, k, out, fl, ct_scan=True), out, w_base, f_base),
            ("verify", lambda: eng.double_scalarmul_t(curve, u1, k, p, out, fl, subtract=True), out, w_ver, f_ver),
            ("decompress", lambda: eng.point_decompress_t(curve, enc, out, fl), out, p, zero),
            ("compress", lambda: eng.point_compress_t(curve, p, None, out32), out32, enc, None),
        ]
        for name, fn, got, want, wfl in configs:
            fl.fill_(0xFF)
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
            ok = bool((got == want).all()) and (wfl is None or bool((fl == wfl).all()))
            results[(curve, name)] = avg
            print(json.dumps({"metric": f"{curve} {name}", "label": args.label, "value": n / (avg * 1e-3), "unit": "units/s", "n": n,
                              "kernel_ms": avg, "min_ms": min(ms), "max_ms": max(ms), "steps": args.steps, "warmup": args.warmup,
                              "parity_ok": ok}), flush=True)
            failed = failed or not ok
    for name in ("var", "var-ct", "base", "base-l2", "base-ct", "verify", "decompress", "compress"):
        print(json.dumps({"metric": f"jubjub / ed25519 {name}", "label": args.label,
                          "value": results[("jubjub", name)] / results[("ed25519", name)], "unit": "ratio of kernel_ms", "n": n,
                          "by_multiplies": 1.8 if name != "compress" else 1.0}), flush=True)
    eng.close()
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
