#!/usr/bin/env python3
"""Throughput of the batched BLS12-381 pairing on one GPU, units resident in HBM: one JSON line per operation.

usage: python tools/bench_pairing.py [--log2n 18] [--steps 5] [--warmup 2] [--ops pairing,check2,var] [--label default]
                                     [--out profiles/pairing_bench.jsonl]

  pairing  eccx_pairing_dev, pairs = 1: 576 bytes per unit
  check2   eccx_pairing_check_dev, pairs = 2, the BLS-verify shape: unit i is (-P, Q), (P, Q) for i % 3 == 0 (verdict
           "one") and two unrelated terms otherwise (verdict "not one")
  var      eccx_scalarmul_var_dev on bls12_381_g2 with default options at the same n in the same process: the yardstick
           the rows for G2 and for hashing use

The 13 distinct terms of tests/test_pairing_gpu.py, repeated with period 13.  Parity before a number is printed: every
verdict of check2, every flag, and 256 sampled values of `pairing` against the Python model (tests/pairing_ref.py).
Average over --steps calls timed with events after --warmup; the split by launch (prepare / Miller loop / final
exponentiation) is the device time of each kernel in one further call under torch's profiler."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PERIOD = 13


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ops", default="pairing,check2,var")
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import eccoxide_amd as E
    from eccoxide_amd import workload as W
    from tests import g2_ref as G2
    from tests import pairing_ref as M

    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)
    n = 1 << args.log2n
    rng = np.random.default_rng(381)
    sc = [(int.from_bytes(rng.bytes(32), "big") % M.R, int.from_bytes(rng.bytes(32), "big") % M.R) for _ in range(PERIOD)]
    pts = [(M.g1_mul(a), M.g2_mul(b)) for a, b in sc]
    r1 = np.frombuffer(b"".join(M.g1_record(p)[0] for p, _ in pts), dtype=np.uint8).reshape(PERIOD, 96)
    r1n = np.frombuffer(b"".join(M.g1_record(M.g1_neg(p))[0] for p, _ in pts), dtype=np.uint8).reshape(PERIOD, 96)
    r2 = np.frombuffer(b"".join(G2.to_record(q)[0] for _, q in pts), dtype=np.uint8).reshape(PERIOD, 192)
    vals = np.frombuffer(b"".join(M.f12_to_bytes(M.pairing(p, q)) for p, q in pts), dtype=np.uint8).reshape(PERIOD, 576)
    idx = np.arange(n) % PERIOD
    one = (np.arange(n) % 3 == 0)
    # pairs = 1
    g1_1 = torch.from_numpy(r1[idx]).to(dev).reshape(-1)
    g2_1 = torch.from_numpy(r2[idx]).to(dev).reshape(-1)
    # pairs = 2: (-P_k, Q_k), (P_k, Q_k) or (P_k, Q_k), (P_k+1, Q_k+1)
    idx2 = (idx + 1) % PERIOD
    a1 = np.where(one[:, None], r1n[idx], r1[idx])
    g1_2 = torch.from_numpy(np.stack([a1, np.where(one[:, None], r1[idx], r1[idx2])], axis=1)).to(dev).reshape(-1)
    g2_2 = torch.from_numpy(np.stack([r2[idx], np.where(one[:, None], r2[idx], r2[idx2])], axis=1)).to(dev).reshape(-1)
    out = torch.empty((n, 576), dtype=torch.uint8, device=dev)
    fl = torch.empty((n,), dtype=torch.uint8, device=dev)
    verdicts = torch.empty((n,), dtype=torch.uint8, device=dev)
    eng.reserve("bls12_381_g2", 2 * n, var=True, pairing=True)
    ks_t = torch.from_numpy(W.random_scalars("bls12_381_g2", n, seed=31)).to(dev)
    vout = torch.empty((n * 192,), dtype=torch.uint8, device=dev)
    vfl = torch.empty((n,), dtype=torch.uint8, device=dev)
    sample = rng.choice(n, size=min(256, n), replace=False)

    def parity_pairing():
        if int(fl.max()) != 0:
            return False
        got = out[torch.from_numpy(sample).to(dev)].cpu().numpy()
        return bool(np.array_equal(got, vals[sample % PERIOD]))

    ops = {
        "pairing": (lambda: eng.pairing_t(g1_1, g2_1, 1, out, fl), parity_pairing, 1),
        "check2": (lambda: eng.pairing_check_t(g1_2, g2_2, 2, verdicts),
                   lambda: bool(np.array_equal(verdicts.cpu().numpy(), one.astype(np.uint8))), 2),
        "var": (lambda: eng.scalarmul_var_t("bls12_381_g2", ks_t, g2_1, vout, vfl), lambda: int(vfl.max()) == 0, 0),
    }
    failed = False
    lines = []
    for name in args.ops.split(","):
        fn, ok_fn, pairs = ops[name]
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
        ok = bool(ok_fn())
        split = {}
        if pairs:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize(dev)
            for e in prof.key_averages():
                for k in ("k_pairing_prepare", "k_pairing_miller", "k_pairing_finalexp"):
                    if k in e.key:
                        t = getattr(e, "device_time_total", None)
                        split[k + "_ms"] = (t if t is not None else e.cuda_time_total) / 1e3
        rec = {"metric": f"bls12_381 pairing {name}", "label": args.label, "value": n / (avg * 1e-3), "unit": "units/s", "n": n,
               "pairs": pairs, "kernel_ms": avg, "min_ms": min(ms), "max_ms": max(ms), "steps": args.steps, "warmup": args.warmup,
               "parity_ok": ok, **split}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        failed = failed or not ok
    eng.close()
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
