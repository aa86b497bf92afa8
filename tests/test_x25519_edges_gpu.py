"""The crafted units of tests/x25519_cases.py through eccx_x25519[_dev]: low-order and non-canonical u, the twist, one
scalar per bit position, the clamped bits, the raw ladder's scalar extremes -- among ordinary lanes, filling whole
wavefronts, and as zero results inside the normalisation's shared inversion (a lane's whole column, half of it, a
wavefront, a whole batch); the second trip of the ladder's grid-stride loop; the chunked host path; device buffers at odd
addresses, on a side stream and caller-supplied; the RFC 7748 section 5.2 iteration; the ladder against the Edwards
kernels; the ABI's argument checks.  Outputs and flags byte for byte against the Python model (oracle/ecc_ref.py), which
is evaluated on the distinct units only."""
import ctypes

import numpy as np
import pytest

from eccoxide_amd import engine as EN
from tests import ed25519_ref as ED
from tests import x25519_cases as X

pytestmark = pytest.mark.gpu

ERR_ARG = -2
MODES = [(False, True), (False, False), (True, True), (True, False)]   # (raw, u given)
MODE_IDS = ["rfc-u", "rfc-base", "raw-u", "raw-base"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    return torch


def _dev(torch, b, lead=0):
    t = torch.frombuffer(bytearray(bytes(lead) + b), dtype=torch.uint8).cuda()
    return t[lead:lead + len(b)] if lead else t


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _mismatches(units, want, got):
    bad = [i for i in range(len(units)) if want[0][32 * i:32 * i + 32] != got[0][32 * i:32 * i + 32] or want[1][i] != got[1][i]]
    return len(bad), [(i, units[i].group, units[i].label, got[0][32 * i:32 * i + 32].hex(), got[1][i]) for i in bad[:6]]


def _run_host(engine, units):
    k, u = X.pack(units)
    return engine.x25519(k, u, raw_ladder=units[0].raw)


def _run_dev(engine, torch, units, **kw):
    k, u = X.pack(units)
    out, fl = engine.x25519_t(_dev(torch, k), None if u is None else _dev(torch, u), raw_ladder=units[0].raw, **kw)
    torch.cuda.synchronize()
    return _bytes(out), _bytes(fl)


def _check(engine, torch, units, dev=True):
    want = X.want(units)
    got = _run_host(engine, units)
    assert got == want, ("host", _mismatches(units, want, got))
    if dev:
        got = _run_dev(engine, torch, units)
        assert got == want, ("dev", _mismatches(units, want, got))
    return want


def _tiled(units, n):
    """n units repeating `units`: (scalars, u or None, wanted outputs, wanted flags) as numpy arrays"""
    idx = np.arange(n) % len(units)
    k, u = X.pack(units)
    out, fl = X.want(units)
    rows = lambda b, w: np.frombuffer(b, dtype=np.uint8).reshape(len(units), w)[idx]
    return rows(k, 32), (None if u is None else rows(u, 32)), rows(out, 32), rows(fl, 1).reshape(n)


@pytest.mark.parametrize("raw,with_u", MODES, ids=MODE_IDS)
def test_edge_cases_among_ordinary_lanes(engine, torch_mod, raw, with_u):
    """every crafted unit with an ordinary one after it, host and device form"""
    units = X.interleaved(raw, with_u)
    want = _check(engine, torch_mod, units)
    assert set(want[1]) == ({0, 1} if raw or with_u else {0})   # clamped scalars on the base point never give zero
    by = {(c.group, c.label): (want[0][32 * i:32 * i + 32], want[1][i]) for i, c in enumerate(units)}
    if not raw:   # what the clamp ignores, on the bytes the device returned (the model's, as compared above)
        tag = "u" if with_u else "base"
        zero = by[("extreme", f"k=0x0 {tag}")]
        assert all(by[("bit", f"2^{t} {tag}")] == zero for t in (0, 1, 2, 254, 255))
        if with_u:
            assert all(len({by[("clamp", f"s{s} m{m}")] for m in range(32)}) == 1 for s in range(2))


@pytest.mark.parametrize("raw", [False, True], ids=["rfc", "raw"])
def test_each_crafted_case_fills_a_wavefront(engine, torch_mod, raw):
    """64 copies of each low-order u, and of a handful of scalar extremes, at a wavefront boundary between ordinary units"""
    for with_u in (True, False):
        plain = X.ordinary(raw, with_u)
        crafted = X.select(raw, with_u, ("low_order",))
        ext = {c.label: c for c in X.select(raw, with_u, ("extreme",))}
        tag = "u" if with_u else "base"
        crafted += [ext[f"k={k:#x} {tag}"] for k in ((0, X.L - 1, X.L, 8 * X.L, 2**256 - 1) if raw else (0, 2**256 - 1))]
        units = []
        for j, c in enumerate(crafted):
            units += [plain[(j + i) % len(plain)] for i in range(64)] + [c] * 64
        units += [plain[i % len(plain)] for i in range(37)]
        assert len(units) == 128 * len(crafted) + 37 and all(units[128 * j + 64] is c for j, c in enumerate(crafted))
        _check(engine, torch_mod, units)


def _zero_patterns(raw):
    """{name: (units, where the low-order ones are)}: zero results placed against the normalisation's tile of 256 lanes
    x 16 units; the low-order values cycle along each pattern"""
    n = 4096 + 300
    plain = X.ordinary(raw, True)

    def put(pred):
        where = [i for i in range(n) if pred(i)]
        low = dict(zip(where, X.low_order_units(raw, len(where))))
        return [low.get(i, plain[i % len(plain)]) for i in range(n)], where

    return {
        "column": put(lambda i: i % 256 == 5),                         # all 16 units of lane 5, and 2 of the next tile
        "half column": put(lambda i: i % 256 == 7 and (i // 256) % 2 == 0),
        "wavefront": put(lambda i: 128 <= i < 192),
        "all": (X.low_order_units(raw, 300), list(range(300))),
    }


@pytest.mark.parametrize("raw", [False, True], ids=["rfc", "raw"])
def test_zero_results_inside_the_shared_inversion(engine, torch_mod, raw):
    for name, (units, where) in _zero_patterns(raw).items():
        want = X.want(units)
        assert [i for i, f in enumerate(want[1]) if f] == where and len(where) >= 9, name
        got = _run_dev(engine, torch_mod, units)
        assert got == want, (name, "dev", _mismatches(units, want, got))
        got = _run_host(engine, units)
        assert got == want, (name, "host", _mismatches(units, want, got))


@pytest.mark.parametrize("raw,with_u", [(False, True), (True, False)], ids=["rfc-u", "raw-base"])
def test_grid_stride_second_trip(engine, torch_mod, raw, with_u):
    """n = 2^20 + 300 exceeds the ladder's launch of 8 x 256 lanes per compute unit: a second trip with a ragged tail,
    whose idle lanes re-read unit n - 1.  97 distinct units, every output and flag compared."""
    torch = torch_mod
    n = (1 << 20) + 300
    assert n > 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count
    k, u, want_out, want_fl = _tiled(X.periodic(raw, with_u), n)
    out, fl = engine.x25519_t(torch.from_numpy(k).cuda(), None if u is None else torch.from_numpy(u).cuda(), raw_ladder=raw)
    torch.cuda.synchronize()
    bad = torch.nonzero((out != torch.from_numpy(want_out).cuda()).any(dim=1) | (fl != torch.from_numpy(want_fl).cuda()))
    assert bad.numel() == 0, (bad.numel(), bad.flatten()[:8].tolist())
    assert int(fl.sum()) == int(want_fl.sum()) > 0


@pytest.mark.parametrize("raw,with_u", MODES, ids=MODE_IDS)
def test_chunked_host_path(engine, raw, with_u):
    """host buffers of 2^17 + 371 units: four chunks, the last one shorter"""
    n = (1 << 17) + 371
    k, u, want_out, want_fl = _tiled(X.periodic(raw, with_u), n)
    out, fl = engine.x25519(k.tobytes(), None if u is None else u.tobytes(), raw_ladder=raw)
    got_out, got_fl = np.frombuffer(out, dtype=np.uint8).reshape(n, 32), np.frombuffer(fl, dtype=np.uint8)
    bad = np.nonzero((got_out != want_out).any(axis=1) | (got_fl != want_fl))[0]
    assert bad.size == 0, (bad.size, bad[:8].tolist())


def test_dev_shapes(engine, torch_mod):
    torch = torch_mod
    for raw in (False, True):
        units = X.interleaved(raw, True)[:700]
        k, u = X.pack(units)
        want = X.want(units)
        # a sub-batch whose four buffers start at odd addresses
        for lead in (1, 3):
            lo, hi = 100, 433
            m = hi - lo
            out = torch.full((lead + 32 * m,), 0xA5, dtype=torch.uint8).cuda()
            fl = torch.full((lead + m,), 0xA5, dtype=torch.uint8).cuda()
            engine.x25519_t(_dev(torch, k[32 * lo:32 * hi], lead), _dev(torch, u[32 * lo:32 * hi], lead),
                            out[lead:], fl[lead:], raw_ladder=raw)
            torch.cuda.synchronize()
            assert (_bytes(out[lead:]), _bytes(fl[lead:])) == (want[0][32 * lo:32 * hi], want[1][lo:hi]), (raw, lead)
            assert _bytes(out[:lead]) == b"\xa5" * lead == _bytes(fl[:lead])   # nothing in front of them is touched
        # a side stream, and caller-supplied outputs filled beforehand so that an unwritten byte shows
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            tk, tu = _dev(torch, k), _dev(torch, u)
            out = torch.full((len(units), 32), 0xA5, dtype=torch.uint8, device="cuda")
            fl = torch.full((len(units),), 0xA5, dtype=torch.uint8, device="cuda")
            r_out, r_fl = engine.x25519_t(tk, tu, out, fl, raw_ladder=raw, stream=side.cuda_stream)
            b_out, b_fl = engine.x25519_t(tk, None, raw_ladder=raw, stream=side.cuda_stream)
        side.synchronize()
        assert r_out is out and r_fl is fl
        assert (_bytes(out), _bytes(fl)) == want, (raw, _mismatches(units, want, (_bytes(out), _bytes(fl))))
        base = [c._replace(u=None) for c in units]
        assert (_bytes(b_out), _bytes(b_fl)) == X.want(base)


def test_rfc7748_iteration_on_the_device(engine, torch_mod):
    """RFC 7748 section 5.2, 1000 steps as 1000 calls of one unit each: k = u = 9, then k, u = X25519(k, u), k"""
    torch = torch_mod
    k = u = _dev(torch, X.BASE_U).reshape(1, 32)
    for i in range(1000):
        k, u = engine.x25519_t(k, u)[0], k
        if i == 0:
            assert _bytes(k).hex() == X.RFC_ITER_1
    torch.cuda.synchronize()
    assert _bytes(k).hex() == X.RFC_ITER_1000


def _u_of_records(recs, flags, n):
    """Montgomery u of n Edwards records x || y (little-endian), 0 for the neutral element"""
    us = []
    for i in range(n):
        x, y = (int.from_bytes(recs[64 * i + 32 * j:64 * i + 32 * j + 32], "little") for j in (0, 1))
        assert (flags[i] == 1) == ((x, y) == ED.IDENTITY)
        us.append(X.montgomery_u((x, y)))
    return us


def test_ladder_against_the_edwards_kernels(engine):
    """curve25519.rs:1654-1665 on the device.  The Edwards entry points take the scalar as 32 big-endian bytes and
    points as x || y little-endian (include/eccx.h, byte conventions), so the raw ladder reads the same scalar bytes."""
    rng = np.random.default_rng(1654)
    be = lambda v: v.to_bytes(32, "big")
    # [k](u = 9) == u([k]B)
    ks = [0, 1, 2, 3, 4, 8, X.L - 1, X.L - 2, (X.L - 1) // 2, (X.L + 1) // 2, 1 << 251, 1 << 252, (1 << 252) - 1]
    ks += [int.from_bytes(rng.bytes(32), "big") % X.L for _ in range(500 - len(ks))]
    kb = b"".join(map(be, ks))
    recs, fl = engine.scalarmul_base("ed25519", kb)[:2]
    want = _u_of_records(recs, fl, len(ks))
    assert want[0] == 0 and want[1] == 9 and fl[0] == 1 and sum(fl) == 1
    got, gfl = engine.x25519(kb, None, raw_ladder=True)
    assert got == b"".join(map(X.le, want))
    assert gfl == bytes(1 if w == 0 else 0 for w in want)
    # [k]u(P) == u([k]P) for P = [a]B, some with an 8-torsion component, some of them pure torsion
    m = 300
    pts_rec, pfl = engine.scalarmul_base("ed25519", b"".join(be(int.from_bytes(rng.bytes(32), "big") % X.L) for _ in range(m)))[:2]
    assert pfl == bytes(m)
    pts = [tuple(int.from_bytes(pts_rec[64 * i + 32 * j:64 * i + 32 * j + 32], "little") for j in (0, 1)) for i in range(m)]
    tors = ED.torsion()
    for i in range(8):
        pts[8 + i] = ED.add(pts[8 + i], tors[i])     # mixed order
        pts[24 + i] = tors[i]                        # order 1, 2, 4, 8
        pts[40 + i] = tors[i]
    ks = [int.from_bytes(rng.bytes(32), "big") % X.L for _ in range(m)]
    ks[0], ks[1], ks[2], ks[3] = 0, X.L, 1, X.L - 1
    ks[8:16] = [X.L] * 4 + [0, 1, 2, 8 * X.L]         # [l]P leaves the torsion component
    ks[40:48] = [1, 2, 3, 4, 5, 6, 7, 8]
    kb = b"".join(map(be, ks))
    recs, fl = engine.scalarmul_var("ed25519", kb, b"".join(X.le(x) + X.le(y) for x, y in pts))[:2]
    want = _u_of_records(recs, fl, m)
    assert want[0] == 0 and want[1] == 0 and want[2] == X.montgomery_u(pts[2]) and 0 not in want[48:]
    got, gfl = engine.x25519(kb, b"".join(X.le(X.montgomery_u(p)) for p in pts), raw_ladder=True)
    bad = [(i, ks[i]) for i in range(m) if got[32 * i:32 * i + 32] != X.le(want[i])]
    assert not bad, bad[:8]
    assert gfl == bytes(1 if w == 0 else 0 for w in want)


def test_abi_behaviour(engine, torch_mod):
    lib, ctx = engine._lib, engine._ctx
    k, u = X.pack(X.ordinary(False, True)[:1])
    out, fl = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1)
    err = lambda: lib.eccx_last_error(ctx).decode()
    plain = engine.x25519(k, u)
    dev = [torch_mod.zeros(w, dtype=torch_mod.uint8, device="cuda").data_ptr() for w in (32, 32, 32, 1)]
    for hole in (0, 2, 3):   # scalars, out, flags
        args = [k, u, out, fl]
        args[hole] = None
        assert lib.eccx_x25519(ctx, 1, *args, 0) == ERR_ARG and "null buffer" in err()
        assert lib.eccx_x25519_dev(ctx, 1, *(None if i == hole else d for i, d in enumerate(dev)), 0, None) == ERR_ARG
        assert "null buffer" in err()
    assert lib.eccx_x25519(ctx, 1, k, None, out, fl, 0) == 0                       # u = NULL is the base point
    assert (out.raw, fl.raw) == engine.x25519(k, None) == X.want([X.ordinary(False, True)[0]._replace(u=None)])
    for opts in (0, EN.X25519_RAW_LADDER):
        assert lib.eccx_x25519(ctx, 0, None, None, None, None, opts) == 0
        assert lib.eccx_x25519_dev(ctx, 0, None, None, None, None, opts, None) == 0
    assert lib.eccx_x25519(None, 1, k, u, out, fl, 0) == ERR_ARG
    assert lib.eccx_x25519_dev(None, 1, None, None, None, None, 0, None) == ERR_ARG
    assert lib.eccx_x25519(None, 0, None, None, None, None, 0) == ERR_ARG
    for args in ((k + b"\0", None), (k, u + u), (k, u[:31]), (k + k, u)):
        with pytest.raises(ValueError):
            engine.x25519(*args)
    # unknown option bits are refused before anything is launched or written, as the sibling entry points do
    for bad in (EN.CT_SCAN, EN.VALIDATE_POINTS, 1 << 20, EN.X25519_RAW_LADDER | EN.CT_SCAN):
        out = ctypes.create_string_buffer(b"\xa5" * 32, 32)
        assert lib.eccx_x25519(ctx, 1, k, u, out, fl, bad) == ERR_ARG and "opts" in err()
        assert out.raw == b"\xa5" * 32
        assert lib.eccx_x25519_dev(ctx, 1, None, None, None, None, bad, None) == ERR_ARG and "opts" in err()
        assert lib.eccx_x25519(ctx, 0, None, None, None, None, bad) == ERR_ARG and "opts" in err()
    assert engine.x25519(k, u) == plain == X.want(X.ordinary(False, True)[:1])      # the context still works
