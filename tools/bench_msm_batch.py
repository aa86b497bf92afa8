#!/usr/bin/env python3
"""Time of the batched multi-scalar multiplication over shared points (eccx_msm_batch_dev) on BLS12-381 G1 and G2 on one
GPU, inputs resident in HBM: one JSON line per shape.

usage: python tools/bench_msm_batch.py [--shapes g1:12:1,g1:12:16,...] [--rounds 3] [--window-ms 300] [--sweep]
                                       [--sweep-max-gib 8] [--parent-lib PATH] [--trace-only] [--label default]
                                       [--out profiles/msm_batch_bench.jsonl]

A shape is curve:log2(n):m.  Inputs: uniform scalars below r, m x n of them, and points r_i G from eccx_scalarmul_base_dev.
Before a shape is timed every one of its m results is compared with the model's shortcut (tests/msm_batch_ref.py:
(sum_i k_gi r_i mod r) G).  Per shape, in one process, alternating over --rounds rounds, each operation repeated until
--window-ms of device time, best round reported:
  batch      eccx_msm_batch_dev
  seq        (G1, --parent-lib) m sequential eccx_msm_dev calls of ANOTHER build of the library -- the parent commit's -- on
             the same data: what m commitments cost before
  msm        (G1, m = 1) eccx_msm_dev of this library in the same process: the same launch sequence
  var_sum    the route a caller has without this entry point on either curve: eccx_scalarmul_var_dev on the m x n units
             (the points repeated m times, outside the timing) followed by eccx_point_sum_dev over m groups
  c = ..     (--sweep) the whole schedule at every window width 4 .. 16 whose workspace stays below --sweep-max-gib, through
             the test library (tests/hip_msm_batch/libmsmbatchcheck.so), each checked against the same expected bytes
--trace-only runs warmed batch calls of the LAST shape alone, for a rocprofv3 --kernel-trace --stats run of its own."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_SHAPES = "g1:12:1,g1:12:16,g1:12:256,g1:16:16,g1:20:1,g2:12:1,g2:12:64,g2:16:4"
PREP_MSM = 1 << 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-max-gib", type=float, default=8.0)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_batch_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import eccoxide_amd as E
    from eccoxide_amd import engine as EN
    from tests import msm_batch_ref as MB

    if not torch.cuda.is_available():
        sys.exit("bench_msm_batch: no GPU (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)
    shapes = []
    for item in args.shapes.split(","):
        cv, lg, m = item.split(":")
        shapes.append(({"g1": MB.G1_NAME, "g2": MB.G2_NAME}[cv], 1 << int(lg), int(m)))
    rng = np.random.default_rng(4844)

    def below_r(count):
        raw = rng.bytes(32 * count)
        vals = [int.from_bytes(raw[32 * i:32 * i + 32], "big") % MB.ORDER for i in range(count)]
        return vals, torch.from_numpy(np.frombuffer(b"".join(v.to_bytes(32, "big") for v in vals), dtype=np.uint8).copy()).to(dev)

    top_n = max(n for _, n, _ in shapes)
    top_units = max(n * m for _, n, m in shapes)
    rs, d_rs = below_r(top_n)
    ks, d_ks = below_r(top_units)  # vector g of a shape is ks[g * n : g * n + n]
    d_pts = {}
    for curve in sorted({c for c, _, _ in shapes}):
        pb, nc = MB.point_bytes(curve), max(n for c, n, _ in shapes if c == curve)
        d_pts[curve] = torch.empty((nc * pb,), dtype=torch.uint8, device=dev)
        fl = torch.empty((nc,), dtype=torch.uint8, device=dev)
        eng.scalarmul_base_t(curve, d_rs[:32 * nc], d_pts[curve], fl)
        torch.cuda.synchronize(dev)
        assert int(fl.max()) == 0

    parent = pctx = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        pctx = ctypes.c_void_p()
        assert parent.eccx_init(0, ctypes.byref(pctx)) == 0
        parent.eccx_reserve.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint32]
        parent.eccx_msm_dev.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 5 + [ctypes.c_uint32,
                                                                                                                  ctypes.c_void_p]
    chk = None
    if args.sweep:
        chk = ctypes.CDLL(os.path.join(ROOT, "tests", "hip_msm_batch", "libmsmbatchcheck.so"))
        chk.msmbcheck_bytes.restype = ctypes.c_size_t
        chk.msmbcheck_bytes.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
        chk.msmbcheck_dev.restype = ctypes.c_int
        chk.msmbcheck_dev.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 7

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

    lines, failed = [], False
    for curve, n, m in shapes:
        cid, pb = EN.CURVE_IDS[curve], MB.point_bytes(curve)
        g2 = int(curve == MB.G2_NAME)
        sk, sp = d_ks[:32 * n * m], d_pts[curve][:pb * n]
        want = MB.expected_of_multiples(curve, [ks[n * g:n * g + n] for g in range(m)], rs[:n])
        out = torch.empty((m * pb,), dtype=torch.uint8, device=dev)
        flags = torch.empty((m,), dtype=torch.uint8, device=dev)

        def result(o=out, f=flags):
            torch.cuda.synchronize(dev)
            return o.cpu().numpy().tobytes(), f.cpu().numpy().tobytes()

        def clear():
            out.fill_(0xEE)
            flags.fill_(0xEE)

        eng.reserve_msm_batch(curve, n, m)
        c0 = eng.msm_batch_window_bits(n, m)
        ops, ok = {}, {}
        ops["batch"] = lambda: eng.msm_batch_t(curve, sk, sp, m, out, flags)
        clear()
        ops["batch"]()
        ok["batch"] = result() == want
        if args.trace_only:
            if (curve, n, m) != shapes[-1]:
                continue
            for _ in range(5):
                ops["batch"]()
            assert result() == want
            print(json.dumps({"trace_only": True, "curve": curve, "n": n, "m": m, "window_bits": c0, "calls": 6}))
            break
        if not g2 and m == 1:
            eng.reserve(curve, n, var=False, msm=True)
            ops["msm"] = lambda: eng.msm_t(curve, sk, sp, out, flags)
            clear()
            ops["msm"]()
            ok["msm"] = result() == want
        if parent is not None and not g2:
            assert parent.eccx_reserve(pctx, cid, n, PREP_MSM) == 0

            def seq():
                for g in range(m):
                    rc = parent.eccx_msm_dev(pctx, cid, n, sk.data_ptr() + 32 * n * g, sp.data_ptr(), None, out.data_ptr() + pb * g,
                                             flags.data_ptr() + g, 0, stream.cuda_stream)
                    assert rc == 0, rc

            ops["seq"] = seq
            clear()
            seq()
            ok["seq"] = result() == want
        # the route without this entry point: m x n independent multiplications, then m sums
        units = n * m
        rep_pts = sp.repeat(m)
        vout = torch.empty((units * pb,), dtype=torch.uint8, device=dev)
        vfl = torch.empty((units,), dtype=torch.uint8, device=dev)
        offs = torch.arange(0, units + 1, n, dtype=torch.int64, device=dev)
        eng.reserve(curve, units, var=True)

        def var_sum():
            eng.scalarmul_var_t(curve, sk, rep_pts, vout, vfl)
            eng.point_sum_t(curve, vout, offs, out, flags, inf=vfl)

        ops["var_sum"] = var_sum
        clear()
        var_sum()
        ok["var_sum"] = result() == want
        ws = []
        if chk is not None:
            for c in range(4, 17):
                need = chk.msmbcheck_bytes(g2, n, m, c)
                if need == 0 or need > args.sweep_max_gib * (1 << 30):
                    continue
                buf = torch.empty((need + 256,), dtype=torch.uint8, device=dev)
                ws.append(buf)
                base_ptr = (buf.data_ptr() + 255) // 256 * 256

                def run(c=c, p=base_ptr):
                    rc = chk.msmbcheck_dev(g2, n, m, c, sk.data_ptr(), sp.data_ptr(), None, p, out.data_ptr(), flags.data_ptr(),
                                           stream.cuda_stream)
                    assert rc == 0, rc

                ops[f"c={c}"] = run
                clear()
                run()
                ok[f"c={c}"] = result() == want
        for fn in ops.values():  # every operation warmed before any is timed
            fn()
        torch.cuda.synchronize(dev)
        ms = {name: [] for name in ops}
        reps = {}
        for _ in range(args.rounds):  # the operations alternate
            for name, fn in ops.items():
                t, reps[name] = timed(fn, args.window_ms)
                ms[name].append(t)
        best = {name: min(v) for name, v in ms.items()}
        rec = {"metric": f"{curve} msm_batch", "label": args.label, "n": n, "m": m, "window_bits": c0, "windows": MB.M.windows(c0),
               "batch_ms": best["batch"], "batch_ms_per_vector": best["batch"] / m, "var_sum_ms": best["var_sum"],
               "speedup_vs_var_sum": best["var_sum"] / best["batch"],
               "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "calls_per_round": reps,
               "sweep_ms": {k: best[k] for k in best if k.startswith("c=")}, "parity_ok": ok, "window_ms": args.window_ms}
        if "seq" in best:
            rec["seq_ms"], rec["speedup_vs_seq"] = best["seq"], best["seq"] / best["batch"]
        if "msm" in best:
            rec["msm_ms"], rec["batch_over_msm"] = best["msm"], best["batch"] / best["msm"]
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        failed = failed or not all(ok.values())
        del ws, rep_pts, vout, vfl
    if parent is not None:
        parent.eccx_shutdown.argtypes = [ctypes.c_void_p]
        parent.eccx_shutdown(pctx)
    eng.close()
    if args.out and lines:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
