#!/usr/bin/env python3
"""Throughput of the secp256k1 (p256k1) operations on one GPU, inputs resident in HBM: one JSON line per operation.

usage: python tools/bench_p256k1.py [--log2n 20] [--steps 10] [--warmup 2] [--label glv] [--ops var,base,...]

Operations: var (default variable base: the endomorphism ladder, or the plain ladder in a build with
-DECCX_P256K1_GLV=0 loaded through ECCX_LIB_PATH), base (mul_base), var_ct / base_ct (secret scalars, ECCX_CT_SCAN),
verify (u1 G + u2 Q, x only), compress, decompress; p256r1_var is p256r1's default variable base on the same box, for
scale.  Average launch time over --steps launches measured with events on the launch stream after --warmup untimed
ones; a sample of every timed output is checked against the Python reference (tests/p256k1_ref.py)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL_OPS = ["var", "base", "var_ct", "base_ct", "verify", "compress", "decompress", "p256r1_var"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--label", default="default")
    ap.add_argument("--ops", default=",".join(ALL_OPS))
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps must be at least 10")
    import torch

    import eccoxide_amd as E
    from eccoxide_amd import workload as W
    from tests import p256k1_ref as K

    dev = torch.device("cuda", 0)
    eng = E.Engine(0)
    n = 1 << args.log2n
    stream = torch.cuda.current_stream(dev)
    C = "p256k1"
    ks = torch.from_numpy(W.random_scalars(C, n, seed=3)).to(dev)
    ks2 = torch.from_numpy(W.random_scalars(C, n, seed=4)).to(dev)
    pts, fl = eng.scalarmul_base_t(C, ks)
    torch.cuda.synchronize(dev)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:48].sort().values.tolist()
    ks_h, ks2_h, pts_h = ks.cpu().numpy(), ks2.cpu().numpy(), pts.cpu().numpy()
    base_pts = {i: K.mul_bytes(ks_h[i].tobytes()) for i in idx}
    assert all(pts_h[i].tobytes() == K.point_bytes(base_pts[i]) for i in idx), "fixed-base parity"

    def check_xy(out, want_fn):
        o = out.cpu().numpy()
        return all(o[i].tobytes() == K.point_bytes(want_fn(i)) for i in idx)

    var_want = lambda i: K.mul_bytes(ks2_h[i].tobytes(), base_pts[i])
    out, ofl = eng.scalarmul_var_t(C, ks2, pts)
    enc = eng.point_compress_t(C, pts, fl)
    back, bfl = eng.point_decompress_t(C, enc)
    xo, xfl = eng.double_scalarmul_t(C, ks2, ks, pts, x_only=True)
    ops = {
        "var": (lambda: eng.scalarmul_var_t(C, ks2, pts, out, ofl), lambda: check_xy(out, var_want), "scalar mults/s"),
        "base": (lambda: eng.scalarmul_base_t(C, ks, out, ofl), lambda: check_xy(out, lambda i: base_pts[i]), "scalar mults/s"),
        "var_ct": (lambda: eng.scalarmul_var_t(C, ks2, pts, out, ofl, ct_scan=True), lambda: check_xy(out, var_want),
                   "scalar mults/s"),
        "base_ct": (lambda: eng.scalarmul_base_t(C, ks, out, ofl, ct_scan=True), lambda: check_xy(out, lambda i: base_pts[i]),
                    "scalar mults/s"),
        "verify": (lambda: eng.double_scalarmul_t(C, ks2, ks, pts, xo, xfl, x_only=True),
                   lambda: all(xo.cpu().numpy()[i].tobytes() == K.R.affine_add(K.K1, K.mul_bytes(ks2_h[i].tobytes()),
                                                                              K.mul_bytes(ks_h[i].tobytes(), base_pts[i]))[0]
                               .to_bytes(32, "big") for i in idx), "verifications/s"),
        "compress": (lambda: eng.point_compress_t(C, pts, fl, enc),
                     lambda: all(enc.cpu().numpy()[i].tobytes() == K.compress(base_pts[i]) for i in idx), "points/s"),
        "decompress": (lambda: eng.point_decompress_t(C, enc, back, bfl),
                       lambda: torch.equal(back, pts) and int(bfl.sum()) == 0, "points/s"),
    }
    if "p256r1_var" in args.ops.split(","):
        from oracle import ecc_ref as R

        rk = torch.from_numpy(W.random_scalars("p256r1", n, seed=3)).to(dev)
        rk2 = torch.from_numpy(W.random_scalars("p256r1", n, seed=4)).to(dev)
        rp, _ = eng.scalarmul_base_t("p256r1", rk)
        rout, rfl = eng.scalarmul_var_t("p256r1", rk2, rp)
        c256 = R.CURVES["p256r1"]

        def r_ok():
            o, k1, k2 = rout.cpu().numpy(), rk.cpu().numpy(), rk2.cpu().numpy()
            for i in idx[:8]:
                Pb = R.affine_mul(c256, int.from_bytes(k1[i].tobytes(), "big"), (c256.gx, c256.gy))
                want = R.affine_mul(c256, int.from_bytes(k2[i].tobytes(), "big"), Pb)
                if o[i].tobytes() != want[0].to_bytes(32, "big") + want[1].to_bytes(32, "big"):
                    return False
            return True

        ops["p256r1_var"] = (lambda: eng.scalarmul_var_t("p256r1", rk2, rp, rout, rfl), r_ok, "scalar mults/s")
    for name in args.ops.split(","):
        fn, ok_fn, unit = ops[name]
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
        curve = "p256r1" if name == "p256r1_var" else C
        print(json.dumps({"metric": f"{curve} {name.replace('p256r1_', '')}", "label": args.label, "value": n / (avg * 1e-3),
                          "unit": unit, "n": n, "kernel_ms": avg, "min_ms": min(ms), "max_ms": max(ms), "steps": args.steps,
                          "warmup": args.warmup, "parity_sample_ok": ok}), flush=True)
        if not ok:
            eng.close()
            sys.exit(1)
    eng.close()


if __name__ == "__main__":
    main()
