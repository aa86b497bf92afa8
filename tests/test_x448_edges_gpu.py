"""The crafted units of tests/x448_cases.py through eccx_x448[_dev]: low-order and non-canonical u, the twist, one scalar
per bit position, the clamped bits, the raw ladder's scalar extremes -- among ordinary lanes, filling whole wavefronts,
and as zero results inside the normalisation's shared inversion (a lane's whole column, half of it, a wavefront, a whole
batch); the second trip of the ladder's grid-stride loop; the chunked host path; device buffers at odd addresses, on a
side stream and caller-supplied; the RFC 7748 section 5.2 iteration; commutativity on the device; the ABI's argument
checks; the reservation.  Outputs and flags byte for byte against the Python model (tests/x448_ref.py), which is
evaluated on the distinct units only."""
import ctypes

import numpy as np
import pytest

from eccoxide_amd import engine as EN
from tests import x448_cases as X

pytestmark = pytest.mark.gpu

ERR_ARG = -2
W = 56
MODES = [(False, True), (False, False), (True, True), (True, False)]   # (raw, u given)
MODE_IDS = ["rfc-u", "rfc-base", "raw-u", "raw-base"]
NORM_U = 8            # units per lane of the normalisation (kernels_x448.hpp X448_NORM_U): tiles of 256 x 8
LADDER_WAVES = 2      # waves per SIMD of the ladder (X448_LADDER_WAVES): 2 workgroups of 256 lanes per compute unit


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
    bad = [i for i in range(len(units)) if want[0][W * i:W * i + W] != got[0][W * i:W * i + W] or want[1][i] != got[1][i]]
    return len(bad), [(i, units[i].group, units[i].label, got[0][W * i:W * i + W].hex(), got[1][i]) for i in bad[:6]]


def _run_host(engine, units):
    k, u = X.pack(units)
    return engine.x448(k, u, raw_ladder=units[0].raw)


def _run_dev(engine, torch, units, **kw):
    k, u = X.pack(units)
    out, fl = engine.x448_t(_dev(torch, k), None if u is None else _dev(torch, u), raw_ladder=units[0].raw, **kw)
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
    return rows(k, W), (None if u is None else rows(u, W)), rows(out, W), rows(fl, 1).reshape(n)


@pytest.mark.parametrize("raw,with_u", MODES, ids=MODE_IDS)
def test_edge_cases_among_ordinary_lanes(engine, torch_mod, raw, with_u):
    """every crafted unit with an ordinary one after it, host and device form"""
    units = X.interleaved(raw, with_u)
    want = _check(engine, torch_mod, units)
    assert set(want[1]) == ({0, 1} if raw or with_u else {0})   # clamped scalars on the base point never give zero
    by = {(c.group, c.label): (want[0][W * i:W * i + W], want[1][i]) for i, c in enumerate(units)}
    if not raw:   # what the clamp ignores, on the bytes the device returned (the model's, as compared above)
        tag = "u" if with_u else "base"
        zero = by[("extreme", f"k=0x0 {tag}")]
        assert all(by[("bit", f"2^{t} {tag}")] == zero for t in X.CLAMPED_BITS)
        if with_u:
            assert all(len({by[("clamp", f"s{s} m{m}")] for m in range(8)}) == 1 for s in range(2))


@pytest.mark.parametrize("raw", [False, True], ids=["rfc", "raw"])
def test_each_crafted_case_fills_a_wavefront(engine, torch_mod, raw):
    """64 copies of each low-order u, and of the scalar extremes, at a wavefront boundary between ordinary units"""
    for with_u in (True, False):
        plain = X.ordinary(raw, with_u)
        crafted = X.select(raw, with_u, ("low_order",))
        ext = {c.label: c for c in X.select(raw, with_u, ("extreme",))}
        tag = "u" if with_u else "base"
        crafted += [ext[f"k={k:#x} {tag}"] for k in ((0, X.L - 1, X.L, 4 * X.L, 2**448 - 1) if raw else (0, 2**448 - 1))]
        units = []
        for j, c in enumerate(crafted):
            units += [plain[(j + i) % len(plain)] for i in range(64)] + [c] * 64
        units += [plain[i % len(plain)] for i in range(37)]
        assert len(units) == 128 * len(crafted) + 37 and all(units[128 * j + 64] is c for j, c in enumerate(crafted))
        _check(engine, torch_mod, units)


def _zero_patterns(raw):
    """{name: (units, where the low-order ones are)}: zero results placed against the normalisation's tile of 256 lanes
    x NORM_U units, over two tiles plus 300 units; the low-order values cycle along each pattern"""
    n = 2 * 256 * NORM_U + 300
    plain = X.ordinary(raw, True)

    def put(pred):
        where = [i for i in range(n) if pred(i)]
        low = dict(zip(where, X.low_order_units(raw, len(where))))
        return [low.get(i, plain[i % len(plain)]) for i in range(n)], where

    return {
        "column": put(lambda i: i % 256 == 5),                         # all NORM_U units of lane 5 in both tiles, 2 of the third
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
    """n = the ladder's launch (LADDER_WAVES workgroups of 256 lanes per compute unit) + 300: a second trip with a ragged
    tail, whose idle lanes re-read unit n - 1.  97 distinct units, every output and flag compared on the device."""
    torch = torch_mod
    launch = LADDER_WAVES * 256 * torch.cuda.get_device_properties(0).multi_processor_count
    n = launch + 300
    assert launch < n <= (1 << 20) + 300
    k, u, want_out, want_fl = _tiled(X.periodic(raw, with_u), n)
    out, fl = engine.x448_t(torch.from_numpy(k).cuda(), None if u is None else torch.from_numpy(u).cuda(), raw_ladder=raw)
    torch.cuda.synchronize()
    bad = torch.nonzero((out != torch.from_numpy(want_out).cuda()).any(dim=1) | (fl != torch.from_numpy(want_fl).cuda()))
    assert bad.numel() == 0, (bad.numel(), bad.flatten()[:8].tolist())
    assert int(fl.sum()) == int(want_fl.sum()) > 0


@pytest.mark.parametrize("raw,with_u", MODES, ids=MODE_IDS)
def test_chunked_host_path(engine, raw, with_u):
    """host buffers of 2^17 + 371 units: four chunks, the last one shorter"""
    n = (1 << 17) + 371
    k, u, want_out, want_fl = _tiled(X.periodic(raw, with_u), n)
    out, fl = engine.x448(k.tobytes(), None if u is None else u.tobytes(), raw_ladder=raw)
    got_out, got_fl = np.frombuffer(out, dtype=np.uint8).reshape(n, W), np.frombuffer(fl, dtype=np.uint8)
    bad = np.nonzero((got_out != want_out).any(axis=1) | (got_fl != want_fl))[0]
    assert bad.size == 0, (bad.size, bad[:8].tolist())


def test_dev_shapes(engine, torch_mod):
    torch = torch_mod
    for raw in (False, True):
        units = X.interleaved(raw, True)[:160]
        k, u = X.pack(units)
        want = X.want(units)
        # a sub-batch whose four buffers start at odd addresses
        for lead in (1, 3):
            lo, hi = 20, 133
            m = hi - lo
            out = torch.full((lead + W * m,), 0xA5, dtype=torch.uint8).cuda()
            fl = torch.full((lead + m,), 0xA5, dtype=torch.uint8).cuda()
            engine.x448_t(_dev(torch, k[W * lo:W * hi], lead), _dev(torch, u[W * lo:W * hi], lead),
                          out[lead:], fl[lead:], raw_ladder=raw)
            torch.cuda.synchronize()
            assert (_bytes(out[lead:]), _bytes(fl[lead:])) == (want[0][W * lo:W * hi], want[1][lo:hi]), (raw, lead)
            assert _bytes(out[:lead]) == b"\xa5" * lead == _bytes(fl[:lead])   # nothing in front of them is touched
        # a side stream, and caller-supplied outputs filled beforehand so that an unwritten byte shows
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            tk, tu = _dev(torch, k), _dev(torch, u)
            out = torch.full((len(units), W), 0xA5, dtype=torch.uint8, device="cuda")
            fl = torch.full((len(units),), 0xA5, dtype=torch.uint8, device="cuda")
            r_out, r_fl = engine.x448_t(tk, tu, out, fl, raw_ladder=raw, stream=side.cuda_stream)
            b_out, b_fl = engine.x448_t(tk, None, raw_ladder=raw, stream=side.cuda_stream)
        side.synchronize()
        assert r_out is out and r_fl is fl
        assert (_bytes(out), _bytes(fl)) == want, (raw, _mismatches(units, want, (_bytes(out), _bytes(fl))))
        base = [c._replace(u=None) for c in units]
        assert (_bytes(b_out), _bytes(b_fl)) == X.want(base)


def test_rfc7748_iteration_on_the_device(engine, torch_mod):
    """RFC 7748 section 5.2, 1000 steps as 1000 calls of one unit each: k = u = 5, then k, u = X448(k, u), k"""
    torch = torch_mod
    k = u = _dev(torch, X.BASE_U).reshape(1, W)
    for i in range(1000):
        k, u = engine.x448_t(k, u)[0], k
        if i == 0:
            assert _bytes(k).hex() == X.RFC_ITER_1
    torch.cuda.synchronize()
    assert _bytes(k).hex() == X.RFC_ITER_1000


def test_diffie_hellman_commutes_on_the_device(engine, torch_mod):
    """[a]([b]5) == [b]([a]5) on 64 random pairs (curve448.rs:375-383), in both modes, without leaving the device"""
    torch = torch_mod
    g = torch.Generator().manual_seed(448)
    a, b = (torch.randint(0, 256, (64, W), dtype=torch.uint8, generator=g).cuda() for _ in range(2))
    for raw in (False, True):
        pa, fa = engine.x448_t(a, None, raw_ladder=raw)
        pb, fb = engine.x448_t(b, None, raw_ladder=raw)
        ab, f1 = engine.x448_t(a, pb, raw_ladder=raw)
        ba, f2 = engine.x448_t(b, pa, raw_ladder=raw)
        torch.cuda.synchronize()
        assert bool((ab == ba).all()) and int(fa.sum() + fb.sum() + f1.sum() + f2.sum()) == 0
        assert bool((ab != pa).any(dim=1).all()) and bool((ab != 0).any(dim=1).all())
    # one pair against the model
    k0, k1 = _bytes(a[0]), _bytes(b[0])
    assert _bytes(ab[0]) == X.R.ladder(X.R.ladder(5, k1), k0).to_bytes(W, "little")


def test_abi_behaviour(engine, torch_mod):
    lib, ctx = engine._lib, engine._ctx
    k, u = X.pack(X.ordinary(False, True)[:1])
    out, fl = ctypes.create_string_buffer(W), ctypes.create_string_buffer(1)
    err = lambda: lib.eccx_last_error(ctx).decode()
    plain = engine.x448(k, u)
    dev = [torch_mod.zeros(w, dtype=torch_mod.uint8, device="cuda").data_ptr() for w in (W, W, W, 1)]
    for hole in (0, 2, 3):   # scalars, out, flags
        args = [k, u, out, fl]
        args[hole] = None
        assert lib.eccx_x448(ctx, 1, *args, 0) == ERR_ARG and "null buffer" in err()
        assert lib.eccx_x448_dev(ctx, 1, *(None if i == hole else d for i, d in enumerate(dev)), 0, None) == ERR_ARG
        assert "null buffer" in err()
    assert lib.eccx_x448(ctx, 1, k, None, out, fl, 0) == 0                       # u = NULL is the base point
    assert (out.raw, fl.raw) == engine.x448(k, None) == X.want([X.ordinary(False, True)[0]._replace(u=None)])
    for opts in (0, EN.X448_RAW_LADDER):
        assert lib.eccx_x448(ctx, 0, None, None, None, None, opts) == 0
        assert lib.eccx_x448_dev(ctx, 0, None, None, None, None, opts, None) == 0
    assert lib.eccx_x448(None, 1, k, u, out, fl, 0) == ERR_ARG
    assert lib.eccx_x448_dev(None, 1, None, None, None, None, 0, None) == ERR_ARG
    assert lib.eccx_x448(None, 0, None, None, None, None, 0) == ERR_ARG
    for args in ((k + b"\0", None), (k, u + u), (k, u[:55]), (k + k, u)):
        with pytest.raises(ValueError):
            engine.x448(*args)
    # unknown option bits are refused before anything is launched or written, as the sibling entry points do
    for bad in (EN.CT_SCAN, EN.VALIDATE_POINTS, 1 << 20, EN.X448_RAW_LADDER | EN.CT_SCAN):
        out = ctypes.create_string_buffer(b"\xa5" * W, W)
        assert lib.eccx_x448(ctx, 1, k, u, out, fl, bad) == ERR_ARG and "opts" in err()
        assert out.raw == b"\xa5" * W
        assert lib.eccx_x448_dev(ctx, 1, None, None, None, None, bad, None) == ERR_ARG and "opts" in err()
        assert lib.eccx_x448(ctx, 0, None, None, None, None, bad) == ERR_ARG and "opts" in err()
    assert engine.x448(k, u) == plain == X.want(X.ordinary(False, True)[:1])      # the context still works


def test_reservation_covers_the_calls(engine, torch_mod):
    """a fresh context beside the session's: reserve(x448=True, host=True) for 300 units under a curve id that is not X448's (it has none),
    then _dev and host calls in all four modes leave eccx_device_bytes where it was"""
    import eccoxide_amd

    torch = torch_mod
    with eccoxide_amd.Engine(0) as eng:
        eng.reserve("p256r1", 300, var=False, host=True, x448=True)
        held = eng.device_bytes()
        assert held >= 300 * (192 + 3 * W + 1)
        for raw, with_u in MODES:
            units = (list(X.ordinary(raw, with_u)) + X.select(raw, with_u, ("low_order", "extreme", "non_canonical")))
            units = [units[i % len(units)] for i in range(300)]
            want = X.want(units)
            assert _run_dev(eng, torch, units) == want and eng.device_bytes() == held, (raw, with_u, "dev")
            assert _run_host(eng, units) == want and eng.device_bytes() == held, (raw, with_u, "host")
