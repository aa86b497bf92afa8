#!/usr/bin/env python3
"""Throughput of batched Ed25519 signing and key derivation on one GPU, inputs resident in HBM, beside the bare
secret-scalar fixed-base comb they run: one JSON line per operation.

usage: python tools/bench_ed25519_sign.py [--log2n 20] [--steps 10] [--warmup 2] [--msg-bytes 32,200] [--label default]
                                          [--only sign_supplied,comb_n,...]

  sign_supplied   eccx_ed25519_sign_dev with the public keys given (Keypair::sign): n lanes of the comb
  sign_derived    eccx_ed25519_sign_dev with pubkeys = NULL (SecretKey::sign): 2n lanes of the comb in one launch
  ..._gather      the same under ECCX_CT_GATHER
  public_key      eccx_ed25519_public_key_dev
  comb_n, comb_2n           eccx_scalarmul_base_dev under ECCX_CT_SCAN on n and on 2n random scalars: the yardstick
  comb_gather_n, _2n        ... under ECCX_CT_SCAN | ECCX_CT_GATHER

Every signature timed must verify (eccx_ed25519_verify_dev), keys derived and supplied must give the same bytes, and
the first 64 lanes are compared with hashlib and Python integers.  After the table: the condition that the derived-keys
form costs no more than the supplied-keys form plus one bare comb of n lanes from this process, with 10 % on top -- a
process that misses it exits 1 (the 2n-lane launch would not be fused).  Average over --steps launches timed with
events after --warmup."""
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
    ap.add_argument("--label", default="default")
    ap.add_argument("--only", default="")
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
    only = set(x for x in args.only.split(",") if x)
    rng = np.random.default_rng(31)
    seeds_np = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    seeds = torch.from_numpy(seeds_np.reshape(-1)).to(dev)
    k2 = torch.from_numpy(W.random_scalars(curve, 2 * n, seed=32)).to(dev).reshape(-1)
    eng.prepare(curve, base=True, ct=True, ct_gather=True)
    eng.reserve(curve, n, ed25519=True, ed25519_sign=True)
    pubs = eng.ed25519_public_key_t(seeds)
    out2 = torch.empty((2 * n * 64,), dtype=torch.uint8, device=dev)
    fl2 = torch.empty((2 * n,), dtype=torch.uint8, device=dev)
    sig = torch.empty((n * 64,), dtype=torch.uint8, device=dev)
    pk = torch.empty((n * 32,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    results = {}

    def timed(name, fn, ok_fn, extra):
        if only and name.split("@")[0] not in only:
            return
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
        torch.cuda.synchronize(dev)
        results[name] = avg
        row = {"metric": f"ed25519 {name.split('@')[0]}", "label": args.label, "kernel_ms": avg, "min_ms": min(ms), "max_ms": max(ms),
               "steps": args.steps, "warmup": args.warmup, "parity_ok": ok}
        row.update(extra)
        row["value"] = extra["n"] / (avg * 1e-3)
        print(json.dumps(row), flush=True)
        if not ok:
            eng.close()
            sys.exit(1)

    # the yardstick: the bare secret-scalar comb and its normalisation, as eccx_scalarmul_base_dev runs them
    for gather in (False, True):
        for lanes, tag in ((n, "n"), (2 * n, "2n")):
            name = f"comb_{'gather_' if gather else ''}{tag}"
            timed(name,
                  lambda: eng.scalarmul_base_t(curve, k2[: lanes * 32], out2[: lanes * 64].view(lanes, 64), fl2[:lanes], ct_scan=True,
                                               ct_gather=gather),
                  lambda: int(fl2[:lanes].sum()) == 0,
                  {"unit": "multiplications/s", "n": lanes})

    def pk_ok():  # the keys themselves are held to the model below: every signature verifies under them
        return bool((pk == pubs).all())

    for gather in (False, True):
        timed(f"public_key{'_gather' if gather else ''}", lambda: eng.ed25519_public_key_t(seeds, pk, ct_gather=gather), pk_ok,
              {"unit": "keys/s", "n": n})

    pubs_np = pubs.cpu().numpy().reshape(n, 32)
    for mb in (int(x) for x in args.msg_bytes.split(",")):
        msgs_np = rng.integers(0, 256, size=(n, mb), dtype=np.uint8)
        msgs = torch.from_numpy(msgs_np.reshape(-1)).to(dev)
        offs = torch.arange(0, (n + 1) * mb, mb, dtype=torch.int64, device=dev)
        verdicts = torch.empty((n,), dtype=torch.uint8, device=dev)
        first = torch.empty((n * 64,), dtype=torch.uint8, device=dev)

        def model_ok(s):
            s_np = s[: 64 * 64].cpu().numpy().reshape(64, 64)
            for i in range(64):
                h = bytearray(hashlib.sha512(seeds_np[i].tobytes()).digest())
                h[0] &= 248
                h[31] = (h[31] & 63) | 64
                a = int.from_bytes(h[:32], "little")
                m = msgs_np[i].tobytes()
                r = int.from_bytes(hashlib.sha512(bytes(h[32:]) + m).digest(), "little") % ELL
                k = int.from_bytes(hashlib.sha512(s_np[i, :32].tobytes() + pubs_np[i].tobytes() + m).digest(), "little") % ELL
                if int.from_bytes(s_np[i, 32:].tobytes(), "little") != (r + k * a) % ELL:
                    return False
            return True

        def sig_ok():
            eng.ed25519_verify_t(msgs, offs, sig, pubs, verdicts, check_bounds=False)
            return bool((verdicts == E.SIG_VALID).all()) and model_ok(sig)

        for gather in (False, True):
            g = "_gather" if gather else ""
            timed(f"sign_supplied{g}@{mb}", lambda: eng.ed25519_sign_t(msgs, offs, seeds, pubs, sig, ct_gather=gather, check_bounds=False),
                  sig_ok, {"unit": "signatures/s", "n": n, "msg_bytes": mb})
            first.copy_(sig)
            timed(f"sign_derived{g}@{mb}", lambda: eng.ed25519_sign_t(msgs, offs, seeds, None, sig, ct_gather=gather, check_bounds=False),
                  lambda: sig_ok() and bool((sig == first).all()), {"unit": "signatures/s", "n": n, "msg_bytes": mb})
            s_name, d_name, c_name = f"sign_supplied{g}@{mb}", f"sign_derived{g}@{mb}", f"comb_{'gather_' if gather else ''}n"
            if all(x in results for x in (s_name, d_name, c_name)):
                bound = 1.10 * (results[s_name] + results[c_name])
                fused = results[d_name] <= bound
                print(json.dumps({"metric": f"ed25519 sign{g} fused check", "label": args.label, "msg_bytes": mb, "n": n,
                                  "derived_ms": results[d_name], "supplied_ms": results[s_name], "comb_n_ms": results[c_name],
                                  "bound_ms": bound, "overhead_supplied_over_comb_n_ms": results[s_name] - results[c_name],
                                  "overhead_derived_over_comb_2n_ms":
                                      results[d_name] - results.get(f"comb_{'gather_' if gather else ''}2n", float("nan")),
                                  "signatures_per_s_supplied": n / (results[s_name] * 1e-3),
                                  "signatures_per_s_derived": n / (results[d_name] * 1e-3), "fused_ok": fused}), flush=True)
                if not fused:
                    eng.close()
                    sys.exit(1)
    eng.close()


if __name__ == "__main__":
    main()
