#!/usr/bin/env python3
"""Throughput of batched X448 on one GPU, inputs resident in HBM: one JSON line per mode, and eccx_x25519 at the same n
in the same process as the yardstick.

usage: python tools/bench_x448.py [--log2n 20] [--steps 10] [--warmup 2] [--label default] [--split-from SUMMARY.json]

  rfc-u     eccx_x448_dev, RFC 7748 semantics, u given
  rfc-base  eccx_x448_dev on the base point (u = NULL)
  raw-u     eccx_x448_dev with ECCX_X448_RAW_LADDER, u given
  x25519    eccx_x25519_dev, RFC semantics, u given

Every output and flag of every timed configuration is compared on the device against the expectation of a periodic
tiling of 97 units (tests/x448_cases.py, tests/x25519_cases.py: crafted and ordinary units, zero results among them)
before its number is printed.  Average over --steps launches timed with events after --warmup.

--split-from: a tools/prof_summary.py summary of a rocprofv3 --kernel-trace run of this tool (a run of its own); its
per-kernel lines for the ladder and the normalisation are appended as "split" lines."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--label", default="default")
    ap.add_argument("--split-from")
    args = ap.parse_args()
    import numpy as np
    import torch

    import eccoxide_amd as E
    from tests import x25519_cases as X2
    from tests import x448_cases as X4

    if not torch.cuda.is_available():
        sys.exit("tools/bench_x448.py needs a GPU")
    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)
    n = 1 << args.log2n
    eng.reserve("ed25519", n, var=False, x448=True)

    def tiled(mod, units, width):
        idx = np.arange(n) % len(units)
        k, u = mod.pack(units)
        out, fl = mod.want(units)
        rows = lambda b, w: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).reshape(len(units), w)[idx].copy()).to(dev)
        return rows(k, width), (None if u is None else rows(u, width)), rows(out, width), rows(fl, 1).reshape(n)

    configs = []
    for name, raw, with_u in (("rfc-u", False, True), ("rfc-base", False, False), ("raw-u", True, True)):
        k, u, want, wfl = tiled(X4, X4.periodic(raw, with_u), 56)
        out = torch.empty((n, 56), dtype=torch.uint8, device=dev)
        fl = torch.empty((n,), dtype=torch.uint8, device=dev)
        configs.append(("x448 " + name, (lambda k=k, u=u, out=out, fl=fl, raw=raw: eng.x448_t(k, u, out, fl, raw_ladder=raw)), out, fl, want, wfl))
    k, u, want, wfl = tiled(X2, X2.periodic(False, True), 32)
    out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    fl = torch.empty((n,), dtype=torch.uint8, device=dev)
    configs.append(("x25519 rfc-u", (lambda k=k, u=u, out=out, fl=fl: eng.x25519_t(k, u, out, fl)), out, fl, want, wfl))
    torch.cuda.synchronize(dev)
    failed = False
    results = {}
    for name, fn, out, fl, want, wfl in configs:
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
        ok = bool((out == want).all()) and bool((fl == wfl).all()) and int(wfl.sum()) > 0 if "base" not in name else \
            bool((out == want).all()) and bool((fl == wfl).all())
        results[name] = avg
        print(json.dumps({"metric": name, "label": args.label, "value": n / (avg * 1e-3), "unit": "units/s", "n": n,
                          "kernel_ms": avg, "min_ms": min(ms), "max_ms": max(ms), "steps": args.steps, "warmup": args.warmup,
                          "parity_ok": ok}), flush=True)
        failed = failed or not ok
    print(json.dumps({"metric": "x448 rfc-u / x25519 rfc-u", "label": args.label, "value": results["x448 rfc-u"] / results["x25519 rfc-u"],
                      "unit": "ratio of kernel_ms", "n": n, "by_multiplies": 5.4}), flush=True)
    if args.split_from:
        with open(args.split_from) as f:
            summary = json.load(f)
        for rec in summary.get("kernel_trace") or []:
            if "CURVE448U" in rec["kernel"]:
                print(json.dumps({"metric": "x448 split", "label": args.label, "kernel": rec["kernel"], "grid_threads": rec["grid_threads"],
                                  "calls": rec["calls"], "median_us": rec["median_us"], "min_us": rec["min_us"], "max_us": rec["max_us"],
                                  "resources": rec.get("resources")}), flush=True)
    eng.close()
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
