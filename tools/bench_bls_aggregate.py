#!/usr/bin/env python3
"""Time of the ragged pairing product (eccx_pairing_check_groups_dev) and of eccx_bls_aggregate_verify_dev on one GPU,
inputs resident in HBM: one JSON line per section.

usage: python tools/bench_bls_aggregate.py [--log2-terms 18] [--log2-units 16] [--messages 4] [--rounds 3] [--window-ms 300]
                                           [--label default] [--out profiles/bls_aggregate_bench.jsonl]

A record replaces the record of the same (metric, label) in --out; other records stay.

Terms are the 13 modelled terms of tests/test_pairing_gpu.py and their negations.  Term j of a group is (P_k, Q_k) for even
j and (-P_k, Q_k) for odd j, k = (j / 2) mod 13, so a group's product is 1 exactly when its length is even: every verdict is
compared ON THE DEVICE before a shape is timed.  In one process, alternating over --rounds rounds, each operation repeated
until --window-ms of device time; reported: the best round in ms.
  uniform 2     2^log2-terms / 2 groups of 2: eccx_pairing_check_groups_dev beside eccx_pairing_check_dev (pairs = 2) on the
                same buffers; the ratio, and the new route's launches by kernel (the scan, the per-term prepare, the Miller
                loop, the product passes, the gather, the final exponentiation)
  uniform K+1   groups of K + 1 (two chunks each), the same pair of routes
  two halves    2 groups of 2^(log2-terms - 1) terms: the old route would run 2 lanes and is not timed
  skewed        lengths 1 .. 64 cycling over the same total, beside eccx_pairing_check_dev padded to pairs = 64 with
                flagged terms
Then the scheme (min-pk): 2^log2-units units of --messages (key, message) pairs, keys, signatures and aggregates made by the
library, every verdict VALID on the device and one flipped message per 64 units INVALID alone before timing:
  aggregate_verify   eccx_bls_aggregate_verify_dev beside its parts in the same process: the key decoder and the signature
                decoder with ECCX_CHECK_SUBGROUP, eccx_hash_to_g2_dev over all messages, eccx_pairing_check_groups_dev on
                term buffers assembled beforehand.  Reported: fused / sum."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PERIOD = 13
KERNELS = ("k_pgroups_scan", "k_pgroups_prepare", "k_pgroups_miller", "k_pgroups_product", "k_pgroups_gather", "k_pairing_finalexp",
           "k_pairing_prepare", "k_pairing_miller")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-terms", type=int, default=18)
    ap.add_argument("--log2-units", type=int, default=16)
    ap.add_argument("--messages", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bls_aggregate_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import eccoxide_amd as E
    from tests import g2_ref as G2
    from tests import pairing_ref as M

    if not torch.cuda.is_available():
        sys.exit("bench_bls_aggregate: no GPU (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)
    K = eng.pairing_group_chunk()
    total = 1 << args.log2_terms
    rng = np.random.default_rng(381)
    sc = [(int.from_bytes(rng.bytes(32), "big") % M.R, int.from_bytes(rng.bytes(32), "big") % M.R) for _ in range(PERIOD)]
    pts = [(M.g1_mul(a), M.g2_mul(b)) for a, b in sc]
    r1 = np.frombuffer(b"".join(M.g1_record(p)[0] for p, _ in pts), dtype=np.uint8).reshape(PERIOD, 96)
    r1n = np.frombuffer(b"".join(M.g1_record(M.g1_neg(p))[0] for p, _ in pts), dtype=np.uint8).reshape(PERIOD, 96)
    r2 = np.frombuffer(b"".join(G2.to_record(q)[0] for _, q in pts), dtype=np.uint8).reshape(PERIOD, 192)

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
            for k in KERNELS:
                if k in e.key:
                    t = getattr(e, "device_time_total", None)
                    split[k] = {"ms": round((t if t is not None else e.cuda_time_total) / 1e3, 4), "launches": e.count}
        return split

    def shape(lengths, pad_to=None):
        """the flat buffers of groups of these lengths, their offsets and expected verdicts; pad_to: also the old route's
        unit-major buffers with every group padded to pad_to flagged terms"""
        lengths = np.asarray(lengths, dtype=np.int64)
        offs = np.concatenate(([0], np.cumsum(lengths)))
        j = np.arange(int(offs[-1])) - np.repeat(offs[:-1], lengths)
        k, odd = (j // 2) % PERIOD, (j % 2 == 1)
        g1 = np.where(odd[:, None], r1n[k], r1[k])
        s = {"n": len(lengths), "terms": int(offs[-1]), "g1": torch.from_numpy(g1).to(dev).reshape(-1),
             "g2": torch.from_numpy(r2[k]).to(dev).reshape(-1), "offs": torch.from_numpy(offs).to(dev),
             "want": torch.from_numpy((lengths % 2 == 0).astype(np.uint8)).to(dev),
             "v": torch.empty((len(lengths),), dtype=torch.uint8, device=dev)}
        if pad_to:
            n = len(lengths)
            jj = np.tile(np.arange(pad_to), n)
            kk, oo = (jj // 2) % PERIOD, (jj % 2 == 1)
            s["p1"] = torch.from_numpy(np.where(oo[:, None], r1n[kk], r1[kk])).to(dev).reshape(-1)
            s["p2"] = torch.from_numpy(r2[kk]).to(dev).reshape(-1)
            s["pinf"] = torch.from_numpy((jj >= np.repeat(lengths, pad_to)).astype(np.uint8)).to(dev)
            s["pv"] = torch.empty((n,), dtype=torch.uint8, device=dev)
        return s

    skew = []
    while sum(skew) < total:
        skew.append(min(len(skew) % 64 + 1, total - sum(skew)))
    shapes = {
        "uniform 2": (shape([2] * (total // 2)), 2),
        "uniform K+1": (shape([K + 1] * (total // (2 * (K + 1)) * 2)), K + 1),
        "two halves": (shape([total // 2] * 2), 0),
        "skewed": (shape(skew, pad_to=64), 64),
    }
    eng.reserve("bls12_381_g2", 2 * total + 64 * len(skew), var=False, pairing=True, pairing_groups=True)
    ops, ok = {}, {}
    for name, (s, pairs) in shapes.items():
        ops[f"{name}: groups"] = lambda s=s: eng.pairing_check_groups_t(s["g1"], s["g2"], s["offs"], s["v"])
        if pairs and "p1" not in s:
            ops[f"{name}: uniform"] = lambda s=s, pairs=pairs: eng.pairing_check_t(s["g1"], s["g2"], pairs, s["v"])
        elif pairs:
            ops[f"{name}: padded"] = lambda s=s, pairs=pairs: eng.pairing_check_t(s["p1"], s["p2"], pairs, s["pv"], g1_inf=s["pinf"])
    for name, fn in ops.items():  # parity of every shape on the device, which also warms it
        fn()
        torch.cuda.synchronize(dev)
        s = shapes[name.split(":")[0]][0]
        ok[name] = bool((s["pv" if name.endswith("padded") else "v"] == s["want"]).all())
    ms = {name: [] for name in ops}
    for _ in range(args.rounds):  # the operations alternate
        for name, fn in ops.items():
            ms[name].append(timed(fn, args.window_ms)[0])
    best = {k: min(v) for k, v in ms.items()}
    rec = {"metric": "bls12_381 pairing_check_groups", "label": args.label, "terms": total, "K": K, "R": eng.pairing_group_fanin(),
           "groups": {name: s["n"] for name, (s, _) in shapes.items()}, "ms": {k: round(v, 4) for k, v in best.items()},
           "groups_over_uniform_pairs_2": round(best["uniform 2: groups"] / best["uniform 2: uniform"], 4),
           "groups_over_uniform_pairs_K+1": round(best["uniform K+1: groups"] / best["uniform K+1: uniform"], 4),
           "groups_over_padded_skewed": round(best["skewed: groups"] / best["skewed: padded"], 4),
           "ns_per_term": {k: round(best[f"{k}: groups"] * 1e6 / shapes[k][0]["terms"], 2) for k in shapes},
           "by_kernel": {k: by_kernel(ops[f"{k}: groups"]) for k in shapes},
           "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "parity_ok": ok, "window_ms": args.window_ms}
    print(json.dumps(rec), flush=True)
    lines, failed = [rec], not all(ok.values())
    del shapes, ops
    torch.cuda.empty_cache()
    if args.log2_units:
        rec = scheme(eng, torch, np, dev, 1 << args.log2_units, args.messages, args, timed)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        failed = failed or not all(rec["parity_ok"].values())
    eng.close()
    if args.out:
        keep = []
        if os.path.exists(args.out):
            fresh = {(r["metric"], r["label"]) for r in lines}
            with open(args.out) as f:
                keep = [l for l in f.read().splitlines() if l.strip() and (json.loads(l)["metric"], json.loads(l).get("label")) not in fresh]
        with open(args.out, "w") as f:
            for l in keep:
                f.write(l + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    sys.exit(1 if failed else 0)


def scheme(eng, torch, np, dev, n, per, args, timed):
    from eccoxide_amd import engine as EN
    from tests import pairing_ref as PR

    G1, G2N, dst = "bls12_381_g1", "bls12_381_g2", EN.BLS_DST_POP
    terms = n * per
    rng = np.random.default_rng(3381)
    sk = np.frombuffer(rng.bytes(32 * terms), dtype=np.uint8).copy()
    sk[::32] &= 0x3F  # below r
    d_sk = torch.from_numpy(sk).to(dev)
    d_msgs = torch.from_numpy(np.frombuffer(rng.bytes(32 * terms), dtype=np.uint8).copy()).to(dev)
    d_offs = (torch.arange(terms + 1, dtype=torch.int64, device=dev) * 32).contiguous()
    go = (torch.arange(n + 1, dtype=torch.int64, device=dev) * per).contiguous()
    eng.prepare(G1, base=False, ct=True)
    eng.reserve(G2N, terms, var=False, bls=True)
    eng.reserve(G2N, n + terms, var=False, bls_aggregate=True)
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)
    keys, kst = eng.bls_public_key_t(d_sk)
    psig, sst = eng.bls_sign_t(d_msgs, d_offs, d_sk, dst)
    sxy_all, sfl_all = eng.point_decompress_t(G2N, psig.reshape(-1))
    agg, afl = eng.point_sum_t(G2N, sxy_all.reshape(-1), go)
    sigs = eng.point_compress_t(G2N, agg.reshape(-1), afl).reshape(-1)
    keys = keys.reshape(-1)
    verd = u8(n)
    eng.bls_aggregate_verify_t(d_msgs, d_offs, sigs, keys, go, dst, verd)
    torch.cuda.synchronize(dev)
    ok = {"made": int(kst.min()) == 1 and int(sst.min()) == 1, "valid": int(verd.min()) == 1 and int(verd.max()) == 1}
    bad = d_msgs.clone()
    bad.reshape(n, per * 32)[::64, 32 * (per - 1)] ^= 1  # the last message of one unit in 64
    eng.bls_aggregate_verify_t(bad, d_offs, sigs, keys, go, dst, verd)
    torch.cuda.synchronize(dev)
    v = verd.reshape(n // 64, 64)
    ok["invalid_alone"] = int(v[:, 0].max()) == 0 and int(v[:, 1:].min()) == 1
    del bad, psig, sxy_all, sfl_all, agg
    # the parts' buffers: decoded keys, signatures, H(m), and the flat terms (pk, H(m)) x per, (-G1, sig) per unit
    kxy, kfl, sxy, sfl, hxy, hfl = u8(terms * 96), u8(terms), u8(n * 192), u8(n), u8(terms * 192), u8(terms)
    eng.point_decompress_t(G1, keys, kxy, kfl, check_subgroup=True)
    eng.point_decompress_t(G2N, sigs, sxy, sfl, check_subgroup=True)
    eng.hash_to_g2_t(d_msgs, d_offs, dst, hxy, hfl, check_bounds=False)
    neg = torch.from_numpy(np.frombuffer(PR.g1_record(PR.g1_neg(PR.G1))[0], dtype=np.uint8).copy()).to(dev)
    g1 = torch.cat([kxy.reshape(n, per * 96), neg.reshape(1, 96).expand(n, 96)], 1).reshape(-1).contiguous()
    g2 = torch.cat([hxy.reshape(n, per * 192), sxy.reshape(n, 192)], 1).reshape(-1).contiguous()
    to = (torch.arange(n + 1, dtype=torch.int64, device=dev) * (per + 1)).contiguous()
    pv = u8(n)
    eng.pairing_check_groups_t(g1, g2, to, pv)
    torch.cuda.synchronize(dev)
    ok["component_pairing"] = int(pv.min()) == 1 and int(pv.max()) == 1
    ops = {
        "aggregate_verify": lambda: eng.bls_aggregate_verify_t(d_msgs, d_offs, sigs, keys, go, dst, verd),
        "part: key decoder": lambda: eng.point_decompress_t(G1, keys, kxy, kfl, check_subgroup=True),
        "part: signature decoder": lambda: eng.point_decompress_t(G2N, sigs, sxy, sfl, check_subgroup=True),
        "part: hash_to_g2": lambda: eng.hash_to_g2_t(d_msgs, d_offs, dst, hxy, hfl, check_bounds=False),
        "part: pairing_check_groups": lambda: eng.pairing_check_groups_t(g1, g2, to, pv),
    }
    for fn in ops.values():
        fn()
    torch.cuda.synchronize(dev)
    ms = {name: [] for name in ops}
    for _ in range(args.rounds):
        for name, fn in ops.items():
            ms[name].append(timed(fn, args.window_ms)[0])
    best = {k: min(x) for k, x in ms.items()}
    parts = sum(x for k, x in best.items() if k.startswith("part: "))
    return {"metric": "bls min-pk aggregate_verify", "label": args.label, "units": n, "messages_per_unit": per,
            "ms": {k: round(x, 4) for k, x in best.items()}, "parts_ms": round(parts, 4),
            "fused_over_parts": round(best["aggregate_verify"] / parts, 4),
            "rounds_ms": {k: [round(x, 4) for x in xs] for k, xs in ms.items()}, "parity_ok": ok, "window_ms": args.window_ms}


if __name__ == "__main__":
    main()
