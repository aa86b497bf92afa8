#!/usr/bin/env python3
"""Throughput of batched hashing to BLS12-381 G2 on one GPU, inputs resident in HBM: one JSON line per (message length,
operation).

usage: python tools/bench_h2c_g2.py [--log2n 20] [--steps 5] [--warmup 2] [--msg-bytes 32,200]
                                    [--ops hash,encode,field,map,clear,affine,var,hash_g1] [--label default]

  hash     eccx_hash_to_g2_dev, suite BLS12381G2_XMD:SHA-256_SSWU_RO_ (hash_to_curve)
  encode   eccx_hash_to_g2_dev with ECCX_H2C_NU (encode_to_curve)
  field, map, clear, affine
           each launch of `hash` on its own, through the slots of the library's CurveOps that tests/hip_h2c_g2's
           library calls (hash_to_field, the two maps and the addition, the cofactor chain, the normalisation), on rows of
           this tool's own that hold what the launch before left there
  var      eccx_scalarmul_var_dev on bls12_381_g2 with default options at the same n in the same process: the existing
           kernel the hash is measured against (it takes the hashed points as its bases)
  hash_g1  eccx_hash_to_g1_dev on the same messages

Parity before a number is printed: 256 sampled units of each hashing operation against the Python model
(tests/h2c_g2_ref.py), and every output through the library's subgroup kernel (compress, then decompress under
ECCX_CHECK_SUBGROUP: all flags 0, same bytes back).  Average over --steps launches timed with events after --warmup."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DST = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_"
DST_G1 = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_"
STAGES = ("field", "map", "clear", "affine")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--msg-bytes", default="32,200")
    ap.add_argument("--ops", default="hash,encode,field,map,clear,affine,var,hash_g1")
    ap.add_argument("--label", default="default")
    args = ap.parse_args()
    import numpy as np
    import torch

    import eccoxide_amd as E
    from eccoxide_amd import workload as W
    from tests import h2c_g2_ref as H

    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)
    curve = "bls12_381_g2"
    n = 1 << args.log2n
    rng = np.random.default_rng(9380)
    eng.reserve(curve, n, var=True, h2c=True)
    eng.reserve("bls12_381_g1", n, var=False, h2c=True)
    ks_t = torch.from_numpy(W.random_scalars(curve, n, seed=31)).to(dev)
    sample = rng.choice(n, size=min(256, n), replace=False)
    names = args.ops.split(",")
    stage_lib = None
    if any(s in names for s in STAGES):
        stage_lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hip_h2c_g2", "libh2cg2check.so"))
        stage_lib.h2cg2check_stage.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 4
    failed = False
    for mb in (int(x) for x in args.msg_bytes.split(",")):
        msgs = rng.integers(0, 256, size=(n, mb), dtype=np.uint8)
        msgs_t = torch.from_numpy(msgs.reshape(-1)).to(dev)
        offs_t = torch.arange(0, (n + 1) * mb, mb, dtype=torch.int64, device=dev)
        pts = torch.empty((n, 192), dtype=torch.uint8, device=dev)
        fl = torch.empty((n,), dtype=torch.uint8, device=dev)
        g1pts = torch.empty((n, 96), dtype=torch.uint8, device=dev)
        vout = torch.empty((n * 192,), dtype=torch.uint8, device=dev)
        vfl = torch.empty((n,), dtype=torch.uint8, device=dev)
        bases = torch.empty((n * 192,), dtype=torch.uint8, device=dev)
        rows = torch.empty((2 * n * 84,), dtype=torch.int32, device=dev) if stage_lib else None
        torch.cuda.synchronize(dev)

        def parity(nonuniform):
            torch.cuda.synchronize(dev)
            if int(fl.max()) != 0:
                return False
            enc = eng.point_compress_t(curve, pts.reshape(-1))
            back, bfl = eng.point_decompress_t(curve, enc, check_subgroup=True)
            torch.cuda.synchronize(dev)
            if int(bfl.max()) != 0 or not bool((back.reshape(-1) == pts.reshape(-1)).all()):
                return False
            got = pts[torch.from_numpy(sample).to(dev)].cpu().numpy()
            want, _ = H.hash_records([msgs[i].tobytes() for i in sample], DST, nonuniform)
            return got.tobytes() == want

        def stage(k):
            rc = stage_lib.h2cg2check_stage(k, n, msgs_t.data_ptr(), offs_t.data_ptr(), DST, len(DST), rows.data_ptr(),
                                            pts.data_ptr(), fl.data_ptr(), stream.cuda_stream)
            if rc:
                raise RuntimeError(f"stage {k}: {rc}")

        ops = {
            "hash": (lambda: eng.hash_to_g2_t(msgs_t, offs_t, DST, pts, fl, check_bounds=False), lambda: parity(False)),
            "encode": (lambda: eng.hash_to_g2_t(msgs_t, offs_t, DST, pts, fl, nonuniform=True, check_bounds=False),
                       lambda: parity(True)),
            "var": (lambda: eng.scalarmul_var_t(curve, ks_t, bases, vout, vfl), lambda: int(vfl.max()) == 0),
            "hash_g1": (lambda: eng.hash_to_g1_t(msgs_t, offs_t, DST_G1, g1pts, fl, check_bounds=False), lambda: int(fl.max()) == 0),
        }
        # a launch works on what the launches before it left in the rows, and the map and the chain overwrite their input:
        # every step of a stage replays the earlier stages first, outside the timed events
        for k, s in enumerate(STAGES):
            ops[s] = (lambda k=k: stage(k), (lambda: parity(False)) if s == "affine" else (lambda: True))
        # the ladder's bases: this batch's hashed points
        eng.hash_to_g2_t(msgs_t, offs_t, DST, pts, fl, check_bounds=False)
        bases.copy_(pts.reshape(-1))
        torch.cuda.synchronize(dev)
        for name in names:
            fn, ok_fn = ops[name]

            def prelude(upto=STAGES.index(name) if name in STAGES else 0):
                for j in range(upto):
                    stage(j)

            for _ in range(args.warmup):
                prelude()
                fn()
            torch.cuda.synchronize(dev)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for a, b in ev:
                prelude()
                a.record(stream)
                fn()
                b.record(stream)
            torch.cuda.synchronize(dev)
            ms = [a.elapsed_time(b) for a, b in ev]
            avg = sum(ms) / len(ms)
            ok = bool(ok_fn())
            torch.cuda.synchronize(dev)
            print(json.dumps({"metric": f"bls12_381_g2 h2c {name}", "label": args.label, "value": n / (avg * 1e-3),
                              "unit": "units/s", "n": n, "msg_bytes": mb, "kernel_ms": avg, "min_ms": min(ms), "max_ms": max(ms),
                              "steps": args.steps, "warmup": args.warmup, "parity_ok": ok}), flush=True)
            failed = failed or not ok
    eng.close()
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
