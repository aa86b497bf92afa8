#!/usr/bin/env python3
"""Time of the multi-scalar multiplication on BLS12-381 G1 (eccx_msm_dev) on one GPU, inputs resident in HBM: one JSON
line per size.

usage: python tools/bench_msm.py [--log2n 12,16,18,20,22] [--rounds 3] [--window-ms 300] [--sweep 2] [--skew-log2n 20]
                                 [--trace-only] [--label default] [--out profiles/msm_bench.jsonl]

Inputs: uniform scalars below r and points r_i G from eccx_scalarmul_base_dev; every size is a prefix of one pool.  Before a
size is timed its result is compared with the model's shortcut (tests/msm_ref.py: (sum k_i r_i mod r) G).  Per size, in one
process, alternating over --rounds rounds, each operation repeated until --window-ms of device time:
  msm        eccx_msm_dev
  var        eccx_scalarmul_var_dev on the same n terms, default options: what a caller had before, WITHOUT the sum of
             the n results it would still owe -- a lower bound on that route
  var_glv    the same with ECCX_ASSUME_SUBGROUP (these points are in G1)
  base       eccx_scalarmul_base_dev on the same scalars: time / (16 n) is the fixed-base comb's time per mixed addition, the
             project's best rate for the bucket stage's inner operation; reported is msm / (windows x n x that)
  skew       (--skew-log2n) all scalars equal, beside the uniform input
  c = ..     (--sweep d) the whole schedule at window widths eccx_msm_window_bits(n) - d .. + d through the test library
             (tests/hip_msm/libmsmcheck.so), each checked against the same expected bytes
--trace-only runs warmed msm calls alone, for a rocprofv3 --kernel-trace --stats run of its own."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G1 = "bls12_381_g1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", default="12,16,18,20,22")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--sweep", type=int, default=2)
    ap.add_argument("--skew-log2n", type=int, default=20)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import eccoxide_amd as E
    from tests import msm_ref as M

    if not torch.cuda.is_available():
        sys.exit("bench_msm: no GPU (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)
    sizes = sorted(1 << int(e) for e in args.log2n.split(","))
    top = max(sizes + ([1 << args.skew_log2n] if args.skew_log2n else []))
    rng = np.random.default_rng(381)

    def below_r(count):
        raw = rng.bytes(32 * count)
        vals = [int.from_bytes(raw[32 * i:32 * i + 32], "big") % M.ORDER for i in range(count)]
        return vals, torch.from_numpy(np.frombuffer(b"".join(v.to_bytes(32, "big") for v in vals), dtype=np.uint8).copy()).to(dev)

    rs, d_rs = below_r(top)
    ks, d_ks = below_r(top)
    d_pts = torch.empty((top * 96,), dtype=torch.uint8, device=dev)
    d_fl = torch.empty((top,), dtype=torch.uint8, device=dev)
    eng.scalarmul_base_t(G1, d_rs, d_pts, d_fl)
    torch.cuda.synchronize(dev)
    assert int(d_fl.max()) == 0
    # expected records for every prefix that is timed: running sum of k_i r_i
    want, acc, at = {}, 0, 0
    for n in sizes:
        acc += sum(k * r for k, r in zip(ks[at:n], rs[at:n]))
        at = n
        want[n] = M.record(M.R.affine_mul(M.C, acc % M.ORDER, M.G))
    eng.reserve(G1, top, var=True, msm=True)
    out = torch.empty((96,), dtype=torch.uint8, device=dev)
    flag = torch.empty((1,), dtype=torch.uint8, device=dev)
    vout = torch.empty((top * 96,), dtype=torch.uint8, device=dev)
    vfl = torch.empty((top,), dtype=torch.uint8, device=dev)

    def result():
        torch.cuda.synchronize(dev)
        return out.cpu().numpy().tobytes(), int(flag.cpu().numpy()[0])

    def timed(fn, window_ms):
        """mean ms per call over as many calls as fill window_ms (at least 3), from one pair of events around them all"""
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

    if args.trace_only:
        n = sizes[-1]
        for _ in range(5):
            eng.msm_t(G1, d_ks[:32 * n], d_pts[:96 * n], out, flag)
        assert result() == want[n]
        print(json.dumps({"trace_only": True, "n": n, "calls": 5}))
        eng.close()
        return

    chk = ctypes.CDLL(os.path.join(ROOT, "tests", "hip_msm", "libmsmcheck.so"))
    chk.msmcheck_msm_bytes.restype = ctypes.c_size_t
    chk.msmcheck_msm_bytes.argtypes = [ctypes.c_size_t, ctypes.c_int]
    chk.msmcheck_msm_dev.restype = ctypes.c_int
    chk.msmcheck_msm_dev.argtypes = [ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 6

    lines, failed = [], False
    for n in sizes:
        sk, sp = d_ks[:32 * n], d_pts[:96 * n]
        c0 = eng.msm_window_bits(n)
        ops = {
            "msm": lambda: eng.msm_t(G1, sk, sp, out, flag),
            "var": lambda: eng.scalarmul_var_t(G1, sk, sp, vout[:96 * n], vfl[:n]),
            "var_glv": lambda: eng.scalarmul_var_t(G1, sk, sp, vout[:96 * n], vfl[:n], assume_subgroup=True),
            "base": lambda: eng.scalarmul_base_t(G1, sk, vout[:96 * n], vfl[:n]),
        }
        ok = {}
        ops["msm"]()
        ok["msm"] = result() == want[n]
        if args.skew_log2n and n == 1 << args.skew_log2n:
            d_same = d_ks[:32].repeat(n)
            ops["skew"] = lambda: eng.msm_t(G1, d_same, sp, out, flag)
            ops["skew"]()
            ok["skew"] = result() == M.record(M.R.affine_mul(M.C, ks[0] * sum(rs[:n]) % M.ORDER, M.G))
        ws = []
        for c in range(max(4, c0 - args.sweep), min(16, c0 + args.sweep) + 1) if args.sweep else []:
            buf = torch.empty((chk.msmcheck_msm_bytes(n, c) + 256,), dtype=torch.uint8, device=dev)
            ws.append(buf)
            base_ptr = (buf.data_ptr() + 255) // 256 * 256

            def run(c=c, p=base_ptr):
                rc = chk.msmcheck_msm_dev(n, c, sk.data_ptr(), sp.data_ptr(), p, out.data_ptr(), flag.data_ptr(), stream.cuda_stream)
                assert rc == 0, rc

            ops[f"c={c}"] = run
            run()
            ok[f"c={c}"] = result() == want[n]
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
        madd_ms = best["base"] / (16.0 * n)
        windows = M.windows(c0)
        rec = {"metric": "bls12_381_g1 msm", "label": args.label, "n": n, "window_bits": c0, "windows": windows,
               "msm_ms": best["msm"], "var_ms": best["var"], "var_glv_ms": best["var_glv"], "base_ms": best["base"],
               "speedup_vs_var": best["var"] / best["msm"], "speedup_vs_var_glv": best["var_glv"] / best["msm"],
               "msm_over_comb_rate": best["msm"] / (windows * n * madd_ms),
               "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "calls_per_round": reps,
               "sweep_ms": {k: best[k] for k in best if k.startswith("c=")}, "parity_ok": ok, "window_ms": args.window_ms}
        if "skew" in best:
            rec["skew_ms"] = best["skew"]
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        failed = failed or not all(ok.values())
        del ws
    eng.close()
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
