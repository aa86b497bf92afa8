#!/usr/bin/env python3
"""Throughput of the BLS12-381 G2 kernels on one GPU, batches resident in HBM: one JSON line per operation.

usage: python tools/bench_g2.py [--log2n 20] [--steps 5] [--warmup 1] [--ops var,var_ct,base,base_ct,decompress,
                                 decompress_check,compress,g1_var] [--label default]

  var / var_ct                  eccx_scalarmul_var_dev on bls12_381_g2, default and ECCX_CT_SCAN, bases k_i G
  base / base_ct                eccx_scalarmul_base_dev, default and ECCX_CT_SCAN
  decompress / decompress_check eccx_point_decompress_dev without and with ECCX_CHECK_SUBGROUP
  compress                      eccx_point_compress_dev
  g1_var                        eccx_scalarmul_var_dev on bls12_381_g1 with default options, same n, same process: the
                                ladder the G2 one is measured against

Every timed output is checked before its number is printed: 32 sampled units against the Python model
(tests/g2_ref.py), and all of it by default == ct_scan (var, base), fixed base == variable base on G,
decompress(compress(P)) == P.  The two Fp2 multiplication forms are compared by running this script against a second
library built with tools/build_variant.sh <name> WORKTREE "-DECCX_FP2_KARATSUBA=1" (ECCX_LIB_PATH, --label).
Average over --steps launches timed with events after --warmup."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ops", default="var,var_ct,base,base_ct,decompress,decompress_check,compress,g1_var")
    ap.add_argument("--label", default="default")
    args = ap.parse_args()
    import numpy as np
    import torch

    import eccoxide_amd as E
    from eccoxide_amd import workload as W
    from tests import g2_ref as G2

    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)
    curve = "bls12_381_g2"
    n = 1 << args.log2n
    eng.prepare(curve, base=True, ct=True)
    eng.reserve(curve, n, var=True, ct=True)
    ks = W.random_scalars(curve, n, seed=41)
    ks2 = W.random_scalars(curve, n, seed=42)
    ks_t, ks2_t = torch.from_numpy(ks).to(dev), torch.from_numpy(ks2).to(dev)
    sample = np.random.default_rng(381).choice(n, size=min(32, n), replace=False)
    sample_t = torch.from_numpy(sample).to(dev)

    def rows(t, width):
        return t.reshape(-1, width)[sample_t].cpu().numpy()

    def new(width):
        return torch.empty((n * width,), dtype=torch.uint8, device=dev)

    # the bases k_i G by the fixed-base path, checked on the sample before anything is timed
    bases, bfl = new(192), new(1)
    eng.scalarmul_base_t(curve, ks_t, bases, bfl, ct_scan=False)
    torch.cuda.synchronize(dev)
    base_pts = {int(i): G2.mul(int.from_bytes(ks[i].tobytes(), "big"), G2.G) for i in sample}
    assert rows(bases, 192).tobytes() == b"".join(G2.to_record(base_pts[int(i)])[0] for i in sample), "fixed base differs from the model"
    out = {name: (new(192), new(1)) for name in ("var", "var_ct", "base", "base_ct", "decompress", "decompress_check")}
    enc = new(96)
    zeros = torch.zeros((n,), dtype=torch.uint8, device=dev)

    def same(a, b):
        return bool((out[a][0] == out[b][0]).all()) and bool((out[a][1] == out[b][1]).all())

    def var_ok(name):
        want = b"".join(G2.to_record(G2.mul(int.from_bytes(ks2[i].tobytes(), "big"), base_pts[int(i)]))[0] for i in sample)
        return rows(out[name][0], 192).tobytes() == want and int(out[name][1].max()) == 0

    def base_ok(name):
        return bool((out[name][0] == bases).all()) and int(out[name][1].max()) == 0

    def dec_ok(name):
        return bool((out[name][0] == bases).all()) and int(out[name][1].max()) == 0

    ops = {
        "var": (lambda: eng.scalarmul_var_t(curve, ks2_t, bases, *out["var"], ct_scan=False), lambda: var_ok("var")),
        "var_ct": (lambda: eng.scalarmul_var_t(curve, ks2_t, bases, *out["var_ct"], ct_scan=True),
                   lambda: var_ok("var_ct") and ("var" not in done or same("var", "var_ct"))),
        "base": (lambda: eng.scalarmul_base_t(curve, ks_t, *out["base"], ct_scan=False), lambda: base_ok("base")),
        "base_ct": (lambda: eng.scalarmul_base_t(curve, ks_t, *out["base_ct"], ct_scan=True), lambda: base_ok("base_ct")),
        "compress": (lambda: eng.point_compress_t(curve, bases, zeros, enc),
                     lambda: rows(enc, 96).tobytes() == b"".join(G2.compress(base_pts[int(i)]) for i in sample)),
        "decompress": (lambda: eng.point_decompress_t(curve, enc, *out["decompress"]), lambda: dec_ok("decompress")),
        "decompress_check": (lambda: eng.point_decompress_t(curve, enc, *out["decompress_check"], check_subgroup=True),
                             lambda: dec_ok("decompress_check")),
    }
    g1 = "bls12_381_g1"
    if "g1_var" in args.ops.split(","):
        eng.reserve(g1, n, var=True)
        g1_bases, g1_fl = eng.scalarmul_base_t(g1, ks_t)
        g1_out, g1_ofl = torch.empty((n * 96,), dtype=torch.uint8, device=dev), new(1)
        ops["g1_var"] = (lambda: eng.scalarmul_var_t(g1, ks2_t, g1_bases.reshape(-1), g1_out, g1_ofl), lambda: int(g1_ofl.max()) == 0)
    eng.point_compress_t(curve, bases, zeros, enc)   # the decoders' input, whichever operations are selected
    torch.cuda.synchronize(dev)
    done, failed = set(), False
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
        done.add(name)
        ok = bool(ok_fn())
        torch.cuda.synchronize(dev)
        metric = "bls12_381_g1 var (default ladder)" if name == "g1_var" else f"bls12_381_g2 {name}"
        print(json.dumps({"metric": metric, "label": args.label, "value": n / (avg * 1e-3), "unit": "units/s", "n": n, "kernel_ms": avg,
                          "min_ms": min(ms), "max_ms": max(ms), "steps": args.steps, "warmup": args.warmup, "parity_ok": ok}), flush=True)
        failed = failed or not ok
    eng.close()
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
