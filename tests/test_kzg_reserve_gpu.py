"""eccx_kzg_reserve and eccx_reserve(ECCX_PREP_KZG) against the calls they promise to cover: on a fresh context, with the
comb table of bls12_381_g1 prepared, after one reserve of each no device-resident KZG call at the reserved sizes grows a
buffer (eccx_device_bytes stays where the reserves left it), and smaller shapes do not either.  N = 512 is two evaluations
per lane; m = 3 and n = 300 (more than one workgroup, ragged)."""
import random

import pytest

from tests import kzg_ref as K

pytestmark = pytest.mark.gpu

Q = K.Q
N, M, UNITS = 512, 3, 300


def test_reserve_covers_the_device_calls():
    import torch

    import eccoxide_amd as E

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()

    rng = random.Random("kzg reserve")
    setup = K.Setup(0xC0FFEE_1234_5678_9ABC, K.domain(N))
    polys = [[rng.randrange(Q) for _ in range(N)] for _ in range(M)]
    zs = [rng.randrange(Q), setup.dom[300], 0]
    with E.Engine(0) as eng:
        srs, _ = eng.scalarmul_base("bls12_381_g1", setup.lagrange_scalars())
        d_p, d_z, d_d, d_s = t(K.fr_bytes([p for poly in polys for p in poly])), t(K.fr_bytes(zs)), t(K.fr_bytes(setup.dom)), t(srs)
        # the Engine's one-time check that [tau]G2 is in G2 goes through the host codec: paid here, on the identity's opening
        assert eng.kzg_verify(K.INFINITY_ENC, bytes(32), bytes(32), K.INFINITY_ENC, setup.tau_g2_record()) == bytes([K.SIG_VALID])
        eng.prepare("bls12_381_g1", base=True)
        eng.reserve_kzg(N, M)
        eng.reserve("bls12_381_g2", UNITS, var=False, kzg=True)
        torch.cuda.synchronize()
        last = [eng.device_bytes()]
        grew = []

        def run(label, call):
            got = call()
            torch.cuda.synchronize()
            now = eng.device_bytes()
            print(f"{label}: device_bytes {now} ({now - last[0]:+d})")
            if now != last[0]:
                grew.append((label, now - last[0]))
                last[0] = now
            return got

        c, cf = run("commit", lambda: eng.kzg_commit_t(d_p, d_s))
        y, pi, of = run("open", lambda: eng.kzg_open_t(d_p, d_z, d_d, d_s))
        run("eval", lambda: eng.kzg_eval_t(d_p, d_z, d_d))
        run("open smaller", lambda: eng.kzg_open_t(d_p[: 2 * 64 * 32], d_z[:64], d_d[: 64 * 32].clone(), d_s[: 64 * 96]))
        rep = UNITS // M
        cs, zz, yy, pp = (x.reshape(M, -1).repeat(rep, 1).reshape(-1).contiguous() for x in (c, d_z, y, pi))
        v = run("verify", lambda: eng.kzg_verify_t(cs, zz, yy, pp, setup.tau_g2_record()))
        run("verify smaller", lambda: eng.kzg_verify_t(cs[:48], zz[:32], yy[:32], pp[:48], setup.tau_g2_record()))
        assert bytes(cf.cpu().numpy()) == bytes(M) and bytes(of.cpu().numpy()) == bytes(M)
        assert bytes(v.cpu().numpy()) == bytes([K.SIG_VALID]) * UNITS
        assert not grew, f"a buffer grew after the reserves in {grew}"
