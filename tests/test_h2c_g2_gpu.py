"""eccx_hash_to_g2 / eccx_hash_to_g2_dev through ctypes and libeccx.so against the Python model (tests/h2c_g2_ref.py): the
RFC 9380 vectors, a ragged batch with every message length 0 .. 139, tags of every kind of length, the grid-stride path
of every launch, the outputs through the library's own subgroup test and secret-scalar ladder, the ABI's argument checks
and what eccx_reserve promises.  The model's results for each set are computed once per module."""
import ctypes

import numpy as np
import pytest

import eccoxide_amd as E
from eccoxide_amd import engine as EN
from tests import g2_ref as G2
from tests import h2c_g2_ref as H

pytestmark = pytest.mark.gpu

DST43 = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_"
assert len(DST43) == 43
PB = 192


@pytest.fixture(scope="module")
def eng():
    with E.Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    return torch


def _dev_hash(eng, torch, msgs, dst, *, nonuniform=False, stream=None, lead=0):
    """The _dev form: the messages packed behind `lead` bytes of padding (an odd lead gives an odd base address)."""
    blob = bytes(lead) + b"".join(msgs)
    offs = np.zeros(len(msgs) + 1, dtype=np.int64)
    np.cumsum([len(m) for m in msgs], out=offs[1:])
    d_blob = torch.frombuffer(bytearray(blob if blob else b"\0"), dtype=torch.uint8).cuda()
    d_offs = torch.from_numpy(offs + 7).cuda()  # offsets[0] != 0: only differences count
    out, flags = eng.hash_to_g2_t(d_blob[lead:] if lead else d_blob, d_offs, dst, nonuniform=nonuniform, stream=stream,
                                  check_bounds=False)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), flags.cpu().numpy().tobytes()


@pytest.mark.parametrize("key,nu", [("g2_ro", False), ("g2_nu", True)])
def test_fixture_vectors(eng, torch_mod, key, nu):
    fx = H.FIXTURE[key]
    dst = fx["dst"].encode()
    msgs = [v["msg"].encode() for v in fx["vectors"]]
    want = b"".join(bytes.fromhex(v["p"][0] + v["p"][1]) for v in fx["vectors"])
    assert eng.hash_to_g2(msgs, dst, nonuniform=nu) == (want, bytes(5))
    side = torch_mod.cuda.Stream()
    assert _dev_hash(eng, torch_mod, msgs, dst, nonuniform=nu, stream=side.cuda_stream) == (want, bytes(5))


@pytest.fixture(scope="module")
def ragged():
    """n = 549 from 140 distinct messages: message i is base[i % 140], of length i % 140"""
    rng = np.random.default_rng(549)
    base = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in range(140)]
    msgs = [base[i % 140] for i in range(549)]
    return msgs, H.hash_records(msgs, DST43)


def test_ragged_batch(eng, torch_mod, ragged):
    """two workgroups and a partial one, through both forms"""
    msgs, want = ragged
    assert want[1] == bytes(549)
    assert eng.hash_to_g2(msgs, DST43) == want
    assert _dev_hash(eng, torch_mod, msgs, DST43) == want
    # a sub-batch with its own offsets[0] and an odd message base address
    for lead in (1, 3):
        got = _dev_hash(eng, torch_mod, msgs[100:300], DST43, lead=lead)
        assert got == (want[0][PB * 100:PB * 300], want[1][100:300]), lead


@pytest.fixture(scope="module")
def tagged():
    msgs = [b"", b"tag test", bytes(range(100))]
    tags = [bytes((7 * i + k) & 0xFF for i in range(k)) for k in (0, 1, 43, 255, 256, 300)]
    return msgs, tags, {(len(t), nu): H.hash_records(msgs, t, nu) for t in tags for nu in (False, True)}


def test_tag_lengths(eng, tagged):
    """0 and 1 bytes, the usual 43, the largest plain tag, and two that are hashed down on the host (RFC 9380 5.3.3)"""
    msgs, tags, want = tagged
    for t in tags:
        for nu in (False, True):
            assert eng.hash_to_g2(msgs, t, nonuniform=nu) == want[(len(t), nu)], (len(t), nu)


@pytest.fixture(scope="module")
def periodic():
    msgs = [str(i).encode() for i in range(61)]
    return msgs, H.hash_records(msgs, DST43)


def test_grid_stride_path(eng, torch_mod, periodic):
    """n above every launch's lane count (256 CUs x 8 workgroups x 256 lanes = 524288 for the hashing kernel, one
    workgroup per CU for the map and the cofactor chain), messages of period 61 so that lanes a grid apart differ; every
    output is compared."""
    base, (wp, wf) = periodic
    n = 600_000
    assert wf == bytes(61)
    msgs = [base[i % 61] for i in range(n)]
    got_p, got_f = _dev_hash(eng, torch_mod, msgs, DST43)
    want = np.frombuffer(wp, dtype=np.uint8).reshape(61, PB)[np.arange(n) % 61]
    assert got_f == bytes(n)
    assert np.array_equal(np.frombuffer(got_p, dtype=np.uint8).reshape(n, PB), want)


def test_outputs_through_existing_kernels(eng, ragged):
    """independent of the new code: 200 outputs pass the subgroup kernel behind the decoder, and sk * H(m) on the
    secret-scalar ladder equals the model's product of the model's points for 16 of them"""
    msgs, (wp, wf) = ragged
    n = 200
    pts, flags = eng.hash_to_g2(msgs[:n], DST43)
    enc = eng.point_compress("bls12_381_g2", pts, flags)
    back, bflags = eng.point_decompress("bls12_381_g2", enc, check_subgroup=True)
    assert bflags == bytes(n) and back == pts
    k = 16
    ks = np.random.default_rng(1).integers(0, 256, 32 * k, dtype=np.uint8).tobytes()
    got = eng.scalarmul_var("bls12_381_g2", ks, pts[:PB * k], ct_scan=True)
    want = [G2.to_record(G2.mul(int.from_bytes(ks[32 * i:32 * i + 32], "big"), G2.from_record(wp[PB * i:PB * i + PB])))
            for i in range(k)]
    assert got == (b"".join(w[0] for w in want), bytes(w[1] for w in want))


def test_abi_behaviour(eng, torch_mod):
    lib, ctx = eng._lib, eng._ctx
    offs = (ctypes.c_uint64 * 3)(0, 1, 2)
    out, flags = ctypes.create_string_buffer(2 * PB), ctypes.create_string_buffer(2)
    err = lambda: lib.eccx_last_error(ctx).decode()
    ERR_ARG = -2
    assert lib.eccx_hash_to_g2(ctx, 2, b"ab", offs, DST43, 43, None, flags, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_hash_to_g2(ctx, 2, b"ab", None, DST43, 43, out, flags, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_hash_to_g2(ctx, 2, None, offs, DST43, 43, out, flags, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_hash_to_g2(ctx, 2, b"ab", offs, None, 43, out, flags, 0) == ERR_ARG and "null buffer" in err()
    for bad in (EN.CT_SCAN, 1 << 0, EN.H2C_NU | EN.CT_SCAN, 1 << 20):
        assert lib.eccx_hash_to_g2(ctx, 2, b"ab", offs, DST43, 43, out, flags, bad) == ERR_ARG and "opts" in err()
        assert lib.eccx_hash_to_g2_dev(ctx, 2, None, None, DST43, 43, None, None, bad, None) == ERR_ARG and "opts" in err()
    assert lib.eccx_hash_to_g2_dev(ctx, 2, None, None, DST43, 43, None, None, 0, None) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_hash_to_g2(ctx, 0, None, None, None, 0, None, None, 0) == 0
    assert lib.eccx_hash_to_g2_dev(ctx, 0, None, None, None, 0, None, None, EN.H2C_NU, None) == 0
    # an empty tag with a null pointer is legal
    assert lib.eccx_hash_to_g2(ctx, 2, b"ab", offs, None, 0, out, flags, 0) == 0
    assert (out.raw, flags.raw) == H.hash_records([b"a", b"b"], b"")
    # decreasing offsets: refused by the host form before the device is touched ...
    down = (ctypes.c_uint64 * 4)(0, 2, 1, 3)
    out3, flags3 = ctypes.create_string_buffer(3 * PB), ctypes.create_string_buffer(3)
    assert lib.eccx_hash_to_g2(ctx, 3, b"abc", down, DST43, 43, out3, flags3, 0) == ERR_ARG and "offsets decrease" in err()
    # ... and flagged on that lane alone by the _dev form
    d_msgs = torch_mod.frombuffer(bytearray(b"abc"), dtype=torch_mod.uint8).cuda()
    d_offs = torch_mod.tensor([0, 2, 1, 3], dtype=torch_mod.int64).cuda()
    pts, fl = eng.hash_to_g2_t(d_msgs, d_offs, DST43, check_bounds=False)
    torch_mod.cuda.synchronize()
    pts, fl = pts.cpu().numpy().tobytes(), fl.cpu().numpy().tobytes()
    wp, _ = H.hash_records([b"ab", b"bc"], DST43)
    assert fl == bytes([0, 2, 0])
    assert pts == wp[:PB] + bytes(PB) + wp[PB:]


def test_reserve_covers_the_dev_call(torch_mod, ragged):
    msgs, want = ragged
    with E.Engine(0) as fresh:
        fresh.reserve("bls12_381_g2", 549, var=False, h2c=True)
        before = fresh.device_bytes()
        assert before > 0
        assert _dev_hash(fresh, torch_mod, msgs, DST43) == want
        assert _dev_hash(fresh, torch_mod, msgs[:100], DST43, nonuniform=True)[1] == bytes(100)
        assert fresh.device_bytes() == before
