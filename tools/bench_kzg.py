#!/usr/bin/env python3
"""Time of eccx_kzg_open_dev beside eccx_msm_batch_dev alone on the same quotient scalars, and of eccx_kzg_verify_dev
beside eccx_pairing_check_dev (pairs = 2) on the same count, on one GPU, inputs resident in HBM: one JSON line per section.

usage: python tools/bench_kzg.py [--log2-n 12] [--ms 1,6,64,256] [--log2-units 12,16] [--rounds 3] [--window-ms 300]
                                 [--label default] [--out profiles/kzg_bench.jsonl]

A record replaces the record of the same (metric, label) in --out; other records stay.

The setup is the insecure one of a known tau (tests/kzg_ref.py), its Lagrange points made by the library's fixed-base entry
point; polynomials are random, z random (outside the domain).  Before anything is timed the proofs of the first two
polynomials are compared with the model's, in the exponent, and every verdict of the verification is compared on the
device: all VALID, then with one y replaced exactly that opening INVALID.  In one process, alternating over --rounds
rounds, each operation repeated until --window-ms of device time; reported: the best round in ms.
  open     eccx_kzg_open_dev at N = 2^log2-n for each m; beside it eccx_msm_batch_dev on the quotient scalars of the same
           polynomials (from the test library that runs the Fr kernel alone) and eccx_kzg_eval_dev.  open - msm_batch is
           what the Fr kernel, the compressor and the zeroing cost; fr_share is that difference over the call.
  verify   eccx_kzg_verify_dev at each unit count (the openings of the largest m, repeated) beside eccx_pairing_check_dev
           with pairs = 2 on as many units of e(-G1, G2) e(G1, G2)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--log2-n", type=int, default=12)
    ap.add_argument("--ms", default="1,6,64,256")
    ap.add_argument("--log2-units", default="12,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import eccoxide_amd as E
    from tests import g2_ref as G2
    from tests import kzg_ref as K
    from tests import pairing_ref as PR

    if not torch.cuda.is_available():
        sys.exit("bench_kzg: no GPU (there is no CPU fallback)")
    check = ctypes.CDLL(os.path.join(ROOT, "tests", "hip_kzg", "libkzgcheck.so"))
    check.kzgcheck_eval_quotient.restype = ctypes.c_int
    check.kzgcheck_eval_quotient.argtypes = [ctypes.c_size_t, ctypes.c_size_t] + [ctypes.c_void_p] * 7
    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)
    N, ms_list = 1 << args.log2_n, [int(x) for x in args.ms.split(",")]
    units = [1 << int(x) for x in args.log2_units.split(",")]
    M = max(ms_list)
    G1 = "bls12_381_g1"

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
        return a.elapsed_time(b) / reps

    def dt(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    setup = K.Setup(0x5EC2E7, K.domain(N))
    rng = np.random.default_rng(4844)
    polys = np.frombuffer(rng.bytes(32 * N * M), dtype=np.uint8).copy()
    polys[::32] &= 0x3F  # below r
    zs = np.frombuffer(rng.bytes(32 * M), dtype=np.uint8).copy()
    zs[::32] &= 0x3F
    dom_b = K.fr_bytes(setup.dom)
    # the quotient scalars of the same polynomials, from the Fr kernel run alone
    ys_h, q_h, fl_h = ctypes.create_string_buffer(32 * M), ctypes.create_string_buffer(32 * N * M), ctypes.create_string_buffer(M)
    rc = check.kzgcheck_eval_quotient(N, M, polys.ctypes.data, zs.ctypes.data, dom_b, pow(N, -1, K.Q).to_bytes(32, "big"), ys_h, q_h, fl_h)
    if rc != 0 or fl_h.raw != bytes(M):
        sys.exit(f"bench_kzg: the Fr kernel alone failed ({rc})")
    d_p, d_z, d_d, d_q = torch.from_numpy(polys).to(dev), torch.from_numpy(zs).to(dev), dt(dom_b), dt(q_h.raw)
    d_srs, _ = eng.scalarmul_base_t(G1, dt(setup.lagrange_scalars()))
    d_srs = d_srs.reshape(-1).contiguous()
    eng.prepare(G1, base=True)
    eng.reserve_kzg(N, M)
    eng.reserve("bls12_381_g2", max(units), var=False, kzg=True, pairing=True)
    eng.reserve("bls12_381_g2", 2 * max(units), var=False, pairing=True)

    ok, ops, lines = {}, {}, []
    y_all, pi_all, fl_all = eng.kzg_open_t(d_p, d_z, d_d, d_srs)
    c_all, cf_all = eng.kzg_commit_t(d_p, d_srs)
    torch.cuda.synchronize(dev)
    ok["flags"] = int(fl_all.max()) == 0 and int(cf_all.max()) == 0
    ok["ys equal the kernel alone"] = bytes(y_all.cpu().numpy()) == ys_h.raw
    for g in range(min(2, M)):  # in the exponent
        poly = K.fr_list(polys[32 * N * g:32 * N * (g + 1)].tobytes())
        z = int.from_bytes(zs[32 * g:32 * g + 32].tobytes(), "big")
        y, pi = setup.open(poly, z)
        ok[f"opening {g}"] = bytes(y_all[32 * g:32 * g + 32].cpu().numpy()) == y.to_bytes(32, "big") and \
            bytes(pi_all[48 * g:48 * g + 48].cpu().numpy()) == K.compress(pi) and \
            bytes(c_all[48 * g:48 * g + 48].cpu().numpy()) == K.compress(setup.commit(poly))
    for m in ms_list:
        a = (d_p[:32 * N * m], d_z[:32 * m], d_d, d_srs)
        oy, op, of = (torch.empty(k * m, dtype=torch.uint8, device=dev) for k in (32, 48, 1))
        mo, mf = torch.empty(96 * m, dtype=torch.uint8, device=dev), torch.empty(m, dtype=torch.uint8, device=dev)
        ops[f"m={m}: open"] = lambda a=a, oy=oy, op=op, of=of: eng.kzg_open_t(*a, oy, op, of)
        ops[f"m={m}: msm_batch"] = lambda m=m, mo=mo, mf=mf: eng.msm_batch_t(G1, d_q[:32 * N * m], d_srs, m, mo, mf)
        ops[f"m={m}: eval"] = lambda a=a, oy=oy, of=of: eng.kzg_eval_t(a[0], a[1], a[2], oy, of)
        ops[f"m={m}: commit"] = lambda a=a, op=op, of=of: eng.kzg_commit_t(a[0], a[3], op, of)
    t_ms = {k: [] for k in ops}
    for _ in range(args.rounds):
        for k, fn in ops.items():
            t_ms[k].append(timed(fn, args.window_ms))
    best = {k: min(v) for k, v in t_ms.items()}
    rec = {"metric": "kzg open", "label": args.label, "N": N, "ms": {k: round(v, 4) for k, v in best.items()},
           "open_minus_msm_batch_ms": {f"m={m}": round(best[f"m={m}: open"] - best[f"m={m}: msm_batch"], 4) for m in ms_list},
           "fr_share": {f"m={m}": round((best[f"m={m}: open"] - best[f"m={m}: msm_batch"]) / best[f"m={m}: open"], 4) for m in ms_list},
           "rounds_ms": {k: [round(x, 4) for x in v] for k, v in t_ms.items()}, "parity_ok": dict(ok), "window_ms": args.window_ms}
    print(json.dumps(rec), flush=True)
    lines.append(rec)

    # verification beside the bare pairing check
    tau = setup.tau_g2_record()
    g1t = PR.g1_record(PR.g1_neg(PR.G1))[0] + PR.g1_record(PR.G1)[0]
    g2t = G2.to_record(G2.G)[0] * 2
    vops, vok = {}, {}
    for n in units:
        rep = (n + M - 1) // M
        cs, zz, yy, pp = (x.reshape(M, -1).repeat(rep, 1)[:n].reshape(-1).contiguous() for x in (c_all, d_z, y_all, pi_all))
        v = torch.empty(n, dtype=torch.uint8, device=dev)
        eng.kzg_verify_t(cs, zz, yy, pp, tau, v)
        torch.cuda.synchronize(dev)
        vok[f"n={n}: valid"] = int(v.min()) == 1 and int(v.max()) == 1
        bad = yy.clone()
        bad[32 * (n // 2) + 31] ^= 1
        eng.kzg_verify_t(cs, zz, bad, pp, tau, v)
        torch.cuda.synchronize(dev)
        vok[f"n={n}: invalid alone"] = int(v[n // 2]) == 0 and int(v.sum()) == n - 1
        d_g1, d_g2 = dt(g1t).repeat(n).contiguous(), dt(g2t).repeat(n).contiguous()
        pv = torch.empty(n, dtype=torch.uint8, device=dev)
        eng.pairing_check_t(d_g1, d_g2, 2, pv, n=n)
        torch.cuda.synchronize(dev)
        vok[f"n={n}: pairing one"] = int(pv.min()) == 1 and int(pv.max()) == 1
        vops[f"n={n}: verify"] = lambda a=(cs, zz, yy, pp), v=v: eng.kzg_verify_t(*a, tau, v)
        vops[f"n={n}: pairing_check"] = lambda d_g1=d_g1, d_g2=d_g2, pv=pv, n=n: eng.pairing_check_t(d_g1, d_g2, 2, pv, n=n)
    v_ms = {k: [] for k in vops}
    for _ in range(args.rounds):
        for k, fn in vops.items():
            v_ms[k].append(timed(fn, args.window_ms))
    vbest = {k: min(v) for k, v in v_ms.items()}
    rec = {"metric": "kzg verify", "label": args.label, "ms": {k: round(v, 4) for k, v in vbest.items()},
           "verify_over_pairing_check": {f"n={n}": round(vbest[f"n={n}: verify"] / vbest[f"n={n}: pairing_check"], 4) for n in units},
           "rounds_ms": {k: [round(x, 4) for x in v] for k, v in v_ms.items()}, "parity_ok": vok, "window_ms": args.window_ms}
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    eng.close()
    if args.out:
        write_records(args.out, lines)
    sys.exit(0 if all(ok.values()) and all(vok.values()) else 1)


if __name__ == "__main__":
    main()
