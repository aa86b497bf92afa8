#!/usr/bin/env python3
"""Time of eccx_bls_batch_verify_dev beside eccx_bls_verify_dev on the same triples, and of eccx_scalarmul_u64_dev beside
eccx_scalarmul_var_dev on zero-padded scalars, on one GPU, inputs resident in HBM: one JSON line per section.

usage: python tools/bench_bls_batch.py [--log2-triples 16] [--log2-big 18] [--log2-mul 18] [--rounds 3] [--window-ms 300]
                                       [--profile-shape "one big batch"] [--label default] [--out profiles/bls_batch_bench.jsonl]

A record replaces the record of the same (metric, label) in --out; other records stay.

Keys and signatures (min-pk) are made by the library from random secrets and 32-byte messages; the coefficients are fixed
random bytes.  Before a shape is timed every verdict is compared ON THE DEVICE: all VALID, then with one signature replaced
by its neighbour's exactly that batch INVALID.  In one process, alternating over --rounds rounds, each operation repeated
until --window-ms of device time; reported: the best round in ms.
  shapes        2^log2-triples triples as one batch, as batches of 64 and as batches of 4, and 2^log2-big triples as one
                batch and as batches of 64; each beside eccx_bls_verify_dev on the same triples (the route a caller had
                before)
  by_kernel     the batch call's launches by kernel, from a call of their own under torch.profiler
  kernel trace  --profile-shape NAME runs five batch calls of one shape and exits, for
                    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o X -- python tools/bench_bls_batch.py --profile-shape NAME --out ""
                and --trace-csv DIR/X_kernel_trace.csv (no GPU needed) turns that trace into the "kernel trace" record of
                --out: the launches of the LAST call, from its first k_point_decompress on, by kernel
  short multiply  eccx_scalarmul_u64_dev on G1 and on G2 beside eccx_scalarmul_var_dev with the coefficient zero-padded to 32
                bytes, same points, outputs compared on the device"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def trace_record(path, shape, label):
    """the launches of the last batch call in a rocprofv3 kernel trace (csv), by kernel, in launch order"""
    import collections
    import csv
    import re

    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))

    def name(r):
        m = re.search(r"k_\w+", r["Kernel_Name"])
        return m.group(0) if m else r["Kernel_Name"][:40]

    starts = [i for i, r in enumerate(rows) if name(r) == "k_point_decompress"]
    if not starts:
        sys.exit("bench_bls_batch: no batch call in this trace")
    last, tot = rows[starts[-1]:], collections.OrderedDict()
    for r in last:
        t = tot.setdefault(name(r), [0, 0.0])
        t[0] += 1
        t[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    span = (int(last[-1]["End_Timestamp"]) - int(last[0]["Start_Timestamp"])) / 1e6
    return {"metric": "bls min-pk batch_verify kernel trace", "label": label, "shape": shape,
            "source": "rocprofv3 --kernel-trace --stats, a run of its own (--profile-shape): the last of its five calls",
            "span_ms": round(span, 3), "launches": {k: {"launches": c, "ms": round(ms, 4)} for k, (c, ms) in tot.items()}}


def write_records(out, lines):
    keep = []
    if os.path.exists(out):
        fresh = {(r["metric"], r["label"]) for r in lines}
        with open(out) as f:
            keep = [l for l in f.read().splitlines() if l.strip() and (json.loads(l)["metric"], json.loads(l).get("label")) not in fresh]
    with open(out, "w") as f:
        for l in keep:
            f.write(l + "\n")
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-csv", default="", help="summarise this rocprofv3 kernel trace into the 'kernel trace' record and exit")
    ap.add_argument("--trace-shape", default="one big batch", help="the shape the traced run was given (recorded with --trace-csv)")
    ap.add_argument("--log2-triples", type=int, default=16)
    ap.add_argument("--log2-big", type=int, default=18)
    ap.add_argument("--log2-mul", type=int, default=18)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--profile-shape", default="", help="run five batch calls of this shape and exit (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bls_batch_bench.jsonl"))
    args = ap.parse_args()
    if args.trace_csv:
        rec = trace_record(args.trace_csv, args.trace_shape, args.label)
        print(json.dumps(rec), flush=True)
        if args.out:
            write_records(args.out, [rec])
        sys.exit(0)
    import numpy as np
    import torch

    import eccoxide_amd as E
    from eccoxide_amd import engine as EN

    if not torch.cuda.is_available():
        sys.exit("bench_bls_batch: no GPU (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)
    G1, G2N, dst = "bls12_381_g1", "bls12_381_g2", EN.BLS_DST_POP
    n_small, n_big = 1 << args.log2_triples, 1 << max(args.log2_big, args.log2_triples)
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)

    def timed(fn, window_ms):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize(dev)
        reps = max(3, int(window_ms / max(a.elapsed_time(b), 1e-3)))
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / reps, reps

    def by_kernel(fn):
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize(dev)
        split = {}
        for e in prof.key_averages():
            if "k_" not in e.key:
                continue
            name = e.key[e.key.index("k_"):].split("<")[0].split("(")[0]
            t = getattr(e, "device_time_total", None)
            cur = split.setdefault(name, {"ms": 0.0, "launches": 0})
            cur["ms"] = round(cur["ms"] + (t if t is not None else e.cuda_time_total) / 1e3, 4)
            cur["launches"] += e.count
        return split

    # the triples, made once at the larger size
    rng = np.random.default_rng(4381)
    sk = np.frombuffer(rng.bytes(32 * n_big), dtype=np.uint8).copy()
    sk[::32] &= 0x3F  # below r
    d_sk = torch.from_numpy(sk).to(dev)
    d_msgs = torch.from_numpy(np.frombuffer(rng.bytes(32 * n_big), dtype=np.uint8).copy()).to(dev)
    d_offs = (torch.arange(n_big + 1, dtype=torch.int64, device=dev) * 32).contiguous()
    co = np.frombuffer(rng.bytes(8 * n_big), dtype=np.uint8).copy()
    co[7::8] |= 1  # nonzero
    d_co = torch.from_numpy(co).to(dev)
    eng.prepare(G1, base=False, ct=True)
    eng.reserve(G2N, n_big, var=False, bls=True)
    eng.reserve(G2N, 2 * n_big, var=False, bls_batch=True)
    keys, kst = eng.bls_public_key_t(d_sk)
    sigs, sst = eng.bls_sign_t(d_msgs, d_offs, d_sk, dst)
    torch.cuda.synchronize(dev)
    made = int(kst.min()) == 1 and int(sst.min()) == 1
    keys, sigs = keys.reshape(-1), sigs.reshape(-1)
    bad_sigs = sigs.clone()

    shapes = {"one batch": (n_small, n_small), "batches of 64": (n_small, 64), "batches of 4": (n_small, 4),
              "one big batch": (n_big, n_big), "big batches of 64": (n_big, 64)}
    ops, ok, info = {}, {"made": made}, {}
    for name, (n, per) in shapes.items():
        nb = n // per
        bo = (torch.arange(nb + 1, dtype=torch.int64, device=dev) * per).contiguous()
        a = (d_msgs[:32 * n], d_offs[:n + 1], sigs[:96 * n], keys[:48 * n], d_co[:8 * n], bo)
        verd, mst, single = u8(nb), u8(n), u8(n)
        eng.bls_batch_verify_t(*a, dst, verd, mst)
        torch.cuda.synchronize(dev)
        ok[f"{name}: valid"] = int(verd.min()) == 1 and int(verd.max()) == 1 and int(mst.min()) == 1
        t = (nb // 2) * per + per // 2  # one signature replaced by its neighbour's: that batch INVALID alone
        bad_sigs[96 * t:96 * t + 96] = sigs[96 * (t - 1):96 * t] if t else sigs[96:192]
        eng.bls_batch_verify_t(a[0], a[1], bad_sigs[:96 * n], a[3], a[4], bo, dst, verd, mst)
        torch.cuda.synchronize(dev)
        ok[f"{name}: invalid alone"] = int(verd[nb // 2]) == 0 and int(verd.sum()) == nb - 1
        bad_sigs[96 * t:96 * t + 96] = sigs[96 * t:96 * t + 96]
        eng.bls_verify_t(a[0], a[1], a[2], a[3], dst, single)
        torch.cuda.synchronize(dev)
        ok[f"{name}: single valid"] = int(single.min()) == 1 and int(single.max()) == 1
        ops[f"{name}: batch"] = lambda a=a, verd=verd, mst=mst: eng.bls_batch_verify_t(*a, dst, verd, mst)
        if per == n:  # eccx_bls_verify_dev depends on n alone: timed once per size
            ops[f"{name}: single"] = lambda a=a, single=single: eng.bls_verify_t(a[0], a[1], a[2], a[3], dst, single)
        info[name] = {"triples": n, "batches": nb}
    if args.profile_shape:  # under rocprofv3 --kernel-trace --stats: five calls of one shape and nothing else
        for _ in range(5):
            ops[f"{args.profile_shape}: batch"]()
        torch.cuda.synchronize(dev)
        eng.close()
        sys.exit(0 if all(ok.values()) else 1)
    ms = {name: [] for name in ops}
    for _ in range(args.rounds):  # the operations alternate
        for name, fn in ops.items():
            ms[name].append(timed(fn, args.window_ms)[0])
    best = {k: min(v) for k, v in ms.items()}
    single_of = {"one batch": "one batch: single", "batches of 64": "one batch: single", "batches of 4": "one batch: single",
                 "one big batch": "one big batch: single", "big batches of 64": "one big batch: single"}
    rec = {"metric": "bls min-pk batch_verify", "label": args.label, "shapes": info, "ms": {k: round(x, 4) for k, x in best.items()},
           "batch_over_single": {k: round(best[f"{k}: batch"] / best[single_of[k]], 4) for k in shapes},
           "by_kernel": {k: by_kernel(ops[f"{k}: batch"]) for k in shapes},
           "single_by_kernel": by_kernel(ops["one batch: single"]),
           "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "parity_ok": ok, "window_ms": args.window_ms}
    print(json.dumps(rec), flush=True)
    lines, failed = [rec], not all(ok.values())
    del ops, bad_sigs
    torch.cuda.empty_cache()

    # the short multiply beside the 255-bit ladder on the zero-padded coefficient
    nm = 1 << args.log2_mul
    cm = torch.from_numpy(np.frombuffer(rng.bytes(8 * nm), dtype=np.uint8).copy()).to(dev)
    padded = torch.zeros((nm, 32), dtype=torch.uint8, device=dev)
    padded[:, 24:] = cm.reshape(nm, 8)
    padded = padded.reshape(-1).contiguous()
    base_k = torch.from_numpy(np.frombuffer(rng.bytes(32 * nm), dtype=np.uint8).copy()).to(dev)
    base_k[::32] &= 0x3F
    mul_ms, mul_ok, mul_ops = {}, {}, {}
    for curve in (G1, G2N):
        eng.reserve(curve, nm, var=True)
        pts, _ = eng.scalarmul_base_t(curve, base_k)
        pts = pts.reshape(-1)
        pb = pts.numel() // nm
        o1, f1, o2, f2 = u8(nm * pb), u8(nm), u8(nm * pb), u8(nm)
        mul_ops[f"{curve}: u64"] = lambda curve=curve, pts=pts, o1=o1, f1=f1: eng.scalarmul_u64_t(curve, cm, pts, None, o1, f1)
        mul_ops[f"{curve}: var padded"] = lambda curve=curve, pts=pts, o2=o2, f2=f2: eng.scalarmul_var_t(curve, padded, pts, o2, f2)
        mul_ops[f"{curve}: u64"]()
        mul_ops[f"{curve}: var padded"]()
        torch.cuda.synchronize(dev)
        mul_ok[curve] = bool((o1 == o2).all()) and bool((f1 == f2).all())
    mms = {name: [] for name in mul_ops}
    for _ in range(args.rounds):
        for name, fn in mul_ops.items():
            mms[name].append(timed(fn, args.window_ms)[0])
    mbest = {k: min(v) for k, v in mms.items()}
    rec = {"metric": "bls12_381 scalarmul_u64", "label": args.label, "units": nm, "ms": {k: round(x, 4) for k, x in mbest.items()},
           "u64_over_var": {c: round(mbest[f"{c}: u64"] / mbest[f"{c}: var padded"], 4) for c in (G1, G2N)},
           "rounds_ms": {k: [round(x, 4) for x in v] for k, v in mms.items()}, "parity_ok": mul_ok, "window_ms": args.window_ms}
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    failed = failed or not all(mul_ok.values())
    eng.close()
    if args.out:
        write_records(args.out, lines)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
