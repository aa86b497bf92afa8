#!/usr/bin/env python3
"""Throughput of batched Ed25519 verification on one GPU, inputs resident in HBM: one JSON line per (message length,
operation).

usage: python tools/bench_ed25519.py [--log2n 20] [--steps 10] [--warmup 2] [--msg-bytes 32,200] [--ops verify,shape]
                                     [--label default]

  verify   eccx_ed25519_verify_dev: decoding A, S and R's byte checks, SHA-512(R || A || M) mod l, the verify shape,
           the comparison with R
  shape    eccx_double_scalarmul_dev with ECCX_SUBTRACT on the same S, k and decoded A: the bare verify shape

The signatures are valid by construction: A = [a]B and R = [r]B from mul_base and compress on the GPU, then
k = SHA-512(R || A || M) mod l with hashlib and S = r + k a mod l on the host, outside the timed region.  Every timed
verdict must be ECCX_SIG_VALID, and the verify shape's output must encode to R.  Average over --steps launches timed
with events after --warmup."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ELL = 2**252 + 27742317777372353535851937790883648493


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--msg-bytes", default="32,200")
    ap.add_argument("--ops", default="verify,shape")
    ap.add_argument("--label", default="default")
    args = ap.parse_args()
    import numpy as np
    import torch

    import eccoxide_amd as E
    from eccoxide_amd import workload as W

    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    stream = torch.cuda.current_stream(dev)
    curve = "ed25519"
    n = 1 << args.log2n
    a_t = torch.from_numpy(W.random_scalars(curve, n, seed=21)).to(dev)
    r_t = torch.from_numpy(W.random_scalars(curve, n, seed=22)).to(dev)
    A_xy, afl = eng.scalarmul_base_t(curve, a_t)
    R_xy, rfl = eng.scalarmul_base_t(curve, r_t)
    A_enc, R_enc = eng.point_compress_t(curve, A_xy), eng.point_compress_t(curve, R_xy)
    torch.cuda.synchronize(dev)
    assert int(afl.sum()) == 0 and int(rfl.sum()) == 0
    A_np, R_np = A_enc.cpu().numpy().reshape(n, 32), R_enc.cpu().numpy().reshape(n, 32)
    a_np, r_np = a_t.cpu().numpy().reshape(n, 32), r_t.cpu().numpy().reshape(n, 32)
    rng = np.random.default_rng(23)
    eng.reserve(curve, n, ed25519=True)
    eng.prepare(curve)
    for mb in (int(x) for x in args.msg_bytes.split(",")):
        msgs = rng.integers(0, 256, size=(n, mb), dtype=np.uint8)
        sig = np.zeros((n, 64), dtype=np.uint8)
        k_be = np.zeros((n, 32), dtype=np.uint8)
        s_be = np.zeros((n, 32), dtype=np.uint8)
        for i in range(n):
            Rb, Ab = R_np[i].tobytes(), A_np[i].tobytes()
            k = int.from_bytes(hashlib.sha512(Rb + Ab + msgs[i].tobytes()).digest(), "little") % ELL
            s = (int.from_bytes(r_np[i].tobytes(), "big") + k * int.from_bytes(a_np[i].tobytes(), "big")) % ELL
            sig[i, :32] = R_np[i]
            sig[i, 32:] = np.frombuffer(s.to_bytes(32, "little"), dtype=np.uint8)
            k_be[i] = np.frombuffer(k.to_bytes(32, "big"), dtype=np.uint8)
            s_be[i] = np.frombuffer(s.to_bytes(32, "big"), dtype=np.uint8)
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dev)
        msgs_t, sig_t, pub_t = to(msgs), to(sig), A_enc
        offs_t = torch.arange(0, (n + 1) * mb, mb, dtype=torch.int64, device=dev)
        u1_t, u2_t = to(s_be), to(k_be)
        verdicts = torch.empty((n,), dtype=torch.uint8, device=dev)
        out = torch.empty((n * 64,), dtype=torch.uint8, device=dev)
        ofl = torch.empty((n,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ops = {
            "verify": (lambda: eng.ed25519_verify_t(msgs_t, offs_t, sig_t, pub_t, verdicts, check_bounds=False),
                       lambda: bool((verdicts == E.SIG_VALID).all())),
            "shape": (lambda: eng.double_scalarmul_t(curve, u1_t, u2_t, A_xy, out, ofl, subtract=True),
                      lambda: bool((eng.point_compress_t(curve, out[: 4096 * 64]).reshape(-1) == R_enc.reshape(-1)[: 4096 * 32]).all())),
        }
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
            ok = ok_fn()
            torch.cuda.synchronize(dev)
            print(json.dumps({"metric": f"ed25519 {name}", "label": args.label, "value": n / (avg * 1e-3),
                              "unit": "verifications/s", "n": n, "msg_bytes": mb, "kernel_ms": avg, "min_ms": min(ms),
                              "max_ms": max(ms), "steps": args.steps, "warmup": args.warmup, "parity_ok": ok}), flush=True)
            if not ok:
                eng.close()
                sys.exit(1)
    eng.close()


if __name__ == "__main__":
    main()
