#!/usr/bin/env python3
"""Time of the sums of ragged groups of points (eccx_point_sum_dev) on BLS12-381 G1 and G2 on one GPU, inputs resident in
HBM: one JSON line per curve and group size.

usage: python tools/bench_bls.py [--log2-members 20] [--groups 512,64,2] [--log2-units 18] [--rounds 3] [--window-ms 300]
                                 [--label default] [--out profiles/bls_bench.jsonl]

A record replaces the record of the same (metric, label) in --out; other records stay.

Members are a table of 64 multiples r_j G repeated, member i = r_(i mod 64) G, so the expected sums have a short period
(one value for group sizes that are multiples of 64, 32 values for groups of 2) and come from the models
(tests/msm_ref.py, tests/g2_ref.py); every output record and flag is compared with them ON THE DEVICE before a shape is
timed.  Per curve, in one process, alternating over --rounds rounds, each operation repeated until --window-ms of device
time:
  sum s      eccx_point_sum_dev on 2^log2-members members in groups of s
  add        eccx_point_add_dev on as many PAIRS as there are members: one complete addition and one normalisation per
             unit, so its time per addition is context, not a bar (a sum normalises once per group)
Reported: best round in ms, and ns per member.

Then the scheme (min-pk), 2^log2-units units in HBM, keys and signatures made by the library itself from random secrets and
every verdict and status checked on the device before timing; in the same process and the same alternating rounds:
  verify     eccx_bls_verify_dev beside the calls a caller chained before it, on the same data: G1 decompress and G2
             decompress with ECCX_CHECK_SUBGROUP, eccx_hash_to_g2_dev, eccx_pairing_check_dev with pairs = 2 on term buffers
             interleaved beforehand (the host loop of the old route is NOT in the sum).  Reported: fused / sum.
  sign       eccx_bls_sign_dev beside eccx_hash_to_g2_dev, eccx_scalarmul_var_dev (G2, ECCX_CT_SCAN), eccx_point_compress_dev
  pubkey     eccx_bls_public_key_dev beside eccx_scalarmul_base_dev (G1, ECCX_CT_SCAN) and eccx_point_compress_dev
  fav 512    eccx_bls_fast_aggregate_verify_dev at 512 keys per unit over the same number of KEYS, beside its decoders'
             (eccx_point_decompress_dev of the keys, ECCX_CHECK_SUBGROUP) and its sum's (eccx_point_sum_dev) time alone"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLE = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-members", type=int, default=20)
    ap.add_argument("--groups", default="512,64,2")
    ap.add_argument("--log2-units", type=int, default=18)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bls_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import eccoxide_amd as E
    from tests import g2_ref as G2
    from tests import msm_ref as M

    if not torch.cuda.is_available():
        sys.exit("bench_bls: no GPU (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)
    members = 1 << args.log2_members
    sizes = [int(s) for s in args.groups.split(",")]
    assert all(members % s == 0 and (s % TABLE == 0 or TABLE % s == 0) for s in sizes)
    rng = np.random.default_rng(12381)
    raw = rng.bytes(32 * TABLE)
    rs = [int.from_bytes(raw[32 * j:32 * j + 32], "big") % M.ORDER for j in range(TABLE)]
    models = {
        "bls12_381_g1": (96, lambda k: M.record(M.R.affine_mul(M.C, k % M.ORDER, M.G))),
        "bls12_381_g2": (192, lambda k: G2.to_record(G2.mul(k % M.ORDER, G2.G))),
    }

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

    lines, failed = [], False
    for curve, (pb, model) in models.items():
        d_rs = torch.from_numpy(np.frombuffer(b"".join(r.to_bytes(32, "big") for r in rs), dtype=np.uint8).copy()).to(dev)
        table, fl = eng.scalarmul_base_t(curve, d_rs)
        torch.cuda.synchronize(dev)
        assert int(fl.max()) == 0
        d_pts = table.reshape(TABLE, pb).repeat(members // TABLE, 1).reshape(-1).contiguous()
        eng.reserve(curve, members, var=False)
        out = torch.empty((members * pb,), dtype=torch.uint8, device=dev)
        flags = torch.empty((members,), dtype=torch.uint8, device=dev)
        ops, ok = {}, {}
        for s in sizes:
            n = members // s
            d_offs = (torch.arange(n + 1, dtype=torch.int64, device=dev) * s).contiguous()
            period = max(1, TABLE // s)
            want = [model(sum(rs[(g * s + t) % TABLE] for t in range(s))) for g in range(period)]
            assert all(w[1] == 0 for w in want)
            d_want = torch.from_numpy(np.frombuffer(b"".join(w[0] for w in want), dtype=np.uint8).copy()).to(dev).reshape(period, pb)

            def run(n=n, d_offs=d_offs):
                eng.point_sum_t(curve, d_pts, d_offs, out[:n * pb], flags[:n])

            run()
            torch.cuda.synchronize(dev)
            got = out[:n * pb].reshape(n // period, period, pb)
            ok[f"sum {s}"] = bool((got == d_want.unsqueeze(0)).all()) and int(flags[:n].max()) == 0
            ops[f"sum {s}"] = run
        d_b = torch.roll(d_pts.reshape(members, pb), 1, 0).reshape(-1).contiguous()
        ops["add"] = lambda: eng.point_add_t(curve, d_pts, d_b, out, flags)
        for fn in ops.values():  # every shape warmed before any is timed
            fn()
        torch.cuda.synchronize(dev)
        ms = {name: [] for name in ops}
        reps = {}
        for _ in range(args.rounds):  # the operations alternate
            for name, fn in ops.items():
                t, reps[name] = timed(fn, args.window_ms)
                ms[name].append(t)
        best = {name: min(v) for name, v in ms.items()}
        rec = {"metric": f"{curve} point_sum", "label": args.label, "members": members,
               "ms": {k: round(v, 4) for k, v in best.items()},
               "ns_per_member": {k: round(v * 1e6 / members, 3) for k, v in best.items()},
               "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "calls_per_round": reps, "parity_ok": ok,
               "window_ms": args.window_ms}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        failed = failed or not all(ok.values())
        del d_pts, d_b, out, flags
    if args.log2_units:
        rec = scheme(eng, torch, np, dev, stream, 1 << args.log2_units, args, timed)
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


def scheme(eng, torch, np, dev, stream, n, args, timed):
    from eccoxide_amd import engine as EN
    from tests import pairing_ref as PR

    G1, G2N, dst = "bls12_381_g1", "bls12_381_g2", EN.BLS_DST_POP
    rng = np.random.default_rng(2381)
    sk = np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).copy()
    sk[::32] &= 0x3F  # below r
    d_sk = torch.from_numpy(sk).to(dev)
    d_msgs = torch.from_numpy(np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).copy()).to(dev)
    d_offs = (torch.arange(n + 1, dtype=torch.int64, device=dev) * 32).contiguous()
    eng.prepare(G1, base=False, ct=True)
    eng.reserve(G2N, n, var=False, bls=True)
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)
    keys, kst, sigs, sst, verd = u8(n * 48), u8(n), u8(n * 96), u8(n), u8(n)
    eng.bls_public_key_t(d_sk, keys, kst)
    eng.bls_sign_t(d_msgs, d_offs, d_sk, dst, sigs, sst)
    eng.bls_verify_t(d_msgs, d_offs, sigs, keys, dst, verd)
    torch.cuda.synchronize(dev)
    ok = {"pubkey": int(kst.min()) == 1, "sign": int(sst.min()) == 1, "verify": int(verd.min()) == 1 and int(verd.max()) == 1}
    # one wrong message per 64 units must come out INVALID and nothing else change
    bad = d_msgs.clone()
    bad.reshape(n, 32)[::64, 0] ^= 1
    eng.bls_verify_t(bad, d_offs, sigs, keys, dst, verd)
    torch.cuda.synchronize(dev)
    v = verd.reshape(n // 64, 64)
    ok["verify_invalid"] = int(v[:, 0].max()) == 0 and int(v[:, 1:].min()) == 1
    # the component chains' buffers
    kxy, kfl, sxy, sfl, hxy, hfl = u8(n * 96), u8(n), u8(n * 192), u8(n), u8(n * 192), u8(n)
    eng.point_decompress_t(G1, keys, kxy, kfl, check_subgroup=True)
    eng.point_decompress_t(G2N, sigs, sxy, sfl, check_subgroup=True)
    eng.hash_to_g2_t(d_msgs, d_offs, dst, hxy, hfl, check_bounds=False)
    neg = torch.from_numpy(np.frombuffer(PR.g1_record(PR.g1_neg(PR.G1))[0], dtype=np.uint8).copy()).to(dev)
    g1 = torch.cat([kxy.reshape(n, 96), neg.reshape(1, 96).expand(n, 96)], 1).reshape(-1).contiguous()
    g2 = torch.cat([hxy.reshape(n, 192), sxy.reshape(n, 192)], 1).reshape(-1).contiguous()
    pv = u8(n)
    eng.pairing_check_t(g1, g2, 2, pv)
    torch.cuda.synchronize(dev)
    ok["component_pairing"] = int(pv.min()) == 1 and int(pv.max()) == 1
    pxy, pfl, enc2, enc1 = u8(n * 192), u8(n), u8(n * 96), u8(n * 48)
    per = 512
    units = n // per
    ko = (torch.arange(units + 1, dtype=torch.int64, device=dev) * per).contiguous()
    # FastAggregateVerify's signatures: the sum of each committee's signatures, by the library
    fmsgs = d_msgs[:32].repeat(units)  # one message for everybody: signatures of it under each key
    fsigs, _ = eng.bls_sign_t(d_msgs[:32].repeat(n), d_offs, d_sk, dst)
    fxy, ffl = eng.point_decompress_t(G2N, fsigs.reshape(-1))
    agg, afl = eng.point_sum_t(G2N, fxy.reshape(-1), ko)
    asig = eng.point_compress_t(G2N, agg.reshape(-1), afl).reshape(-1)
    fverd = u8(units)
    eng.bls_fast_aggregate_verify_t(fmsgs, d_offs[:units + 1], asig, keys, ko, dst, fverd)
    torch.cuda.synchronize(dev)
    ok["fav"] = int(fverd.min()) == 1 and int(fverd.max()) == 1
    sumxy, sumfl = u8(units * 96), u8(units)
    ops = {
        "verify": lambda: eng.bls_verify_t(d_msgs, d_offs, sigs, keys, dst, verd),
        "verify: g1 decompress": lambda: eng.point_decompress_t(G1, keys, kxy, kfl, check_subgroup=True),
        "verify: g2 decompress": lambda: eng.point_decompress_t(G2N, sigs, sxy, sfl, check_subgroup=True),
        "verify: hash_to_g2": lambda: eng.hash_to_g2_t(d_msgs, d_offs, dst, hxy, hfl, check_bounds=False),
        "verify: pairing_check": lambda: eng.pairing_check_t(g1, g2, 2, pv),
        "sign": lambda: eng.bls_sign_t(d_msgs, d_offs, d_sk, dst, sigs, sst),
        "sign: ladder": lambda: eng.scalarmul_var_t(G2N, d_sk, hxy, pxy, pfl, ct_scan=True),
        "sign: compress": lambda: eng.point_compress_t(G2N, pxy, pfl, enc2),
        "pubkey": lambda: eng.bls_public_key_t(d_sk, keys, kst),
        "pubkey: comb": lambda: eng.scalarmul_base_t(G1, d_sk, kxy, kfl, ct_scan=True),
        "pubkey: compress": lambda: eng.point_compress_t(G1, kxy, kfl, enc1),
        "fav 512": lambda: eng.bls_fast_aggregate_verify_t(fmsgs, d_offs[:units + 1], asig, keys, ko, dst, fverd),
        "fav 512: key decoders": lambda: eng.point_decompress_t(G1, keys, kxy, kfl, check_subgroup=True),
        "fav 512: sum": lambda: eng.point_sum_t(G1, kxy, ko, sumxy, sumfl),
    }
    order = list(ops)
    order.remove("pubkey")  # the fused key derivation rewrites `keys`: it and its chain run last
    order.remove("pubkey: comb")
    order.remove("pubkey: compress")
    order += ["pubkey: comb", "pubkey: compress", "pubkey"]
    for name in order:
        ops[name]()
    torch.cuda.synchronize(dev)
    ms = {name: [] for name in order}
    for _ in range(args.rounds):
        for name in order:
            ms[name].append(timed(ops[name], args.window_ms)[0])
    best = {k: min(x) for k, x in ms.items()}
    vsum = sum(best[k] for k in best if k.startswith("verify: "))
    ssum = best["verify: hash_to_g2"] + best["sign: ladder"] + best["sign: compress"]
    ksum = best["pubkey: comb"] + best["pubkey: compress"]
    return {"metric": "bls min-pk scheme", "label": args.label, "units": n, "ms": {k: round(x, 4) for k, x in best.items()},
            "verify_components_ms": round(vsum, 4), "verify_fused_over_components": round(best["verify"] / vsum, 4),
            "verify_within_3_percent": best["verify"] <= 1.03 * vsum,
            "sign_components_ms": round(ssum, 4), "sign_fused_over_components": round(best["sign"] / ssum, 4),
            "pubkey_components_ms": round(ksum, 4), "pubkey_fused_over_components": round(best["pubkey"] / ksum, 4),
            "fav_512": {"units": units, "keys": n, "decoders_share": round(best["fav 512: key decoders"] / best["fav 512"], 4),
                        "sum_share": round(best["fav 512: sum"] / best["fav 512"], 4)},
            "rounds_ms": {k: [round(x, 4) for x in xs] for k, xs in ms.items()}, "parity_ok": ok, "window_ms": args.window_ms}


if __name__ == "__main__":
    main()
