"""Every capped-grid kernel added since the pairing on a SECOND, ragged trip of its grid-stride loop.

n = tests/grid_cases.second_trip_units(CUs) = 8 * CUs * 256 + 300 units (524588 on 256 compute units): more than any
persistent_grid, grid(ctx, n, 8) or msm_grid(n, cus * 8) launch covers in one trip, so the loop comes round again -- over
one full workgroup and 44 lanes, the other 212 lanes of that workgroup clamped to unit n - 1.  The fixed-base combs run
on grid(ctx, n, 16) and get 16 * CUs * 256 + 300 units.  The pairing-groups kernels loop over chunk slots, not groups:
see their tests for what each reaches and DESIGN.md section 3.7p for what none can reach inside 1 GB.  What a kernel keeps across
trips (a slab row per lane, LDS rows, a wave-cooperative call, the clamped index) is then in use for the second time.

Unit i takes row i % 13 of a table of 13 rows, so the Python models compute 13 values per case; 13 is coprime to 64 and
256, so every lane position meets every row.  Each table holds a row whose result is the identity (flag 1), one that is
rejected (flag 2 over zero bytes) where the entry point can reject, and ordinary rows.  Outputs that the caller hands in
start as 0xAA, and ALL n records and flags are compared with the tiled expectation.

test_tables_have_the_required_rows needs no GPU: it builds every table from the models and checks their shape."""
import functools
import math
import random

import numpy as np
import pytest

from tests import bls_batch_ref as BR
from tests import bls_sig_ref as B
from tests import g2_ref as G2
from tests import grid_cases as GC
from tests import jubjub_ref as J
from tests import msm_ref as M
from tests import pairing_ref as PR

PERIOD = GC.PERIOD
G1N, G2N, JJ = "bls12_381_g1", "bls12_381_g2", "jubjub"
ORDER = G2.R
GB = 576
P48 = G2.P.to_bytes(48, "big")
gpu = pytest.mark.gpu


def kb32(k):
    return k.to_bytes(32, "big")


# ---- the 13-row tables (models only) -----------------------------------------------------------------------------------
class Table:
    """columns: name -> 13 byte strings of one width; want: 13 records; flags: 13 flag bytes"""

    def __init__(self, want, flags, **columns):
        self.want, self.flags, self.cols = list(want), list(flags), {k: list(v) for k, v in columns.items()}
        assert len(self.want) == len(self.flags) == PERIOD and all(len(v) == PERIOD for v in self.cols.values())

    @classmethod
    def of(cls, results, **columns):
        """results: 13 (record, flag)"""
        return cls([r[0] for r in results], [r[1] for r in results], **columns)


@functools.lru_cache(maxsize=None)
def g2_special():
    from tests.test_g2_gpu import _special

    return _special()


@functools.lru_cache(maxsize=None)
def g2_points(count, seed):
    rng = random.Random(seed)
    return tuple(G2.mul(rng.randrange(1, ORDER), G2.G) for _ in range(count))


def g2_off_twist():
    g = G2.to_record(G2.G)[0]
    return g[:191] + bytes([g[191] ^ 1])


@functools.lru_cache(maxsize=None)
def g2_var_table():
    """(variable base under ECCX_VALIDATE_POINTS, fixed base on the same scalars)"""
    rng = random.Random(1301)
    sp, walk = g2_special(), g2_points(9, 1)
    m = rng.randrange(1, 1 << 240)
    units = [(0, walk[0]), (ORDER, G2.G), (13 * m, sp["t13"]), (rng.randrange(ORDER), None), (13 * m + 5, sp["t13"]),
             (rng.randrange(ORDER), sp["q1"]), ((1 << 256) - 1, walk[1])]
    units += [(rng.randrange(1 << 256) if i % 2 else rng.randrange(ORDER), walk[2 + i]) for i in range(PERIOD - len(units))]
    res = [(bytes(192), 2) if p is None else G2.to_record(G2.mul(k, p)) for k, p in units]
    var = Table.of(res, scalars=[kb32(k) for k, _ in units], points=[g2_off_twist() if p is None else G2.to_record(p)[0] for _, p in units])
    base = Table.of([G2.to_record(G2.mul(k, G2.G)) for k, _ in units], scalars=var.cols["scalars"])
    return var, base


@functools.lru_cache(maxsize=None)
def g2_add_table():
    a, b = g2_points(PERIOD, 2), g2_points(PERIOD, 3)
    pairs = [(a[i], 0, b[i], 0) for i in range(PERIOD)]
    pairs[0] = (a[0], 0, a[0], 0)                       # P + P
    pairs[1] = (a[1], 0, G2.neg(a[1]), 0)               # P + (-P): the identity
    pairs[2] = (None, 1, b[2], 0)                       # an operand flagged 1 over 0xFF bytes
    pairs[3] = (a[3], 0, None, 1)
    pairs[4] = (None, 1, None, 1)
    pairs[5] = (a[5], 2, b[5], 0)                       # a rejected operand stays rejected
    pairs[6] = (g2_special()["t13"], 0, G2.mul(7, g2_special()["t13"]), 0)
    res = [(bytes(192), 2) if 2 in (fa, fb) else G2.to_record(G2.add(p, q)) for p, fa, q, fb in pairs]
    rec = lambda p: b"\xff" * 192 if p is None else G2.to_record(p)[0]
    return Table.of(res, a=[rec(p) for p, _, _, _ in pairs], b=[rec(q) for _, _, q, _ in pairs],
                    a_inf=[bytes([f]) for _, f, _, _ in pairs], b_inf=[bytes([f]) for _, _, _, f in pairs])


@functools.lru_cache(maxsize=None)
def g2_codec_tables():
    """compress (both flavours), decompress, from_uncompressed, decompress under ECCX_CHECK_SUBGROUP"""
    pts = list(g2_points(PERIOD, 4))
    pts[0], pts[7] = None, None
    recs = [G2.to_record(p) for p in pts]
    xy, inf = [r[0] for r in recs], [bytes([r[1]]) for r in recs]
    comp = Table([G2.compress(p) for p in pts], [0] * PERIOD, xy=xy, inf=inf)
    raw = Table([G2.uncompressed(p) for p in pts], [0] * PERIOD, xy=xy, inf=inf)
    g = G2.compress(G2.G)
    x_off = next(x for x in ((i, i + 1) for i in range(40)) if G2.point_of_x(x) is None)
    xb = G2.f2_to_bytes(x_off)
    enc = [G2.compress(p) for p in pts]
    enc[1] = bytes([g[0] & 0x7F]) + g[1:]               # compression bit clear
    enc[2] = bytes([0x80 | xb[0]]) + xb[1:]             # x without a point
    enc[3] = bytes([0xE0]) + bytes(95)                  # infinity with the sort bit
    enc[4] = bytes([P48[0] | 0x80]) + P48[1:] + bytes(48)  # c1 = p
    dec = Table.of([G2.decode_result(G2.decompress(c)) for c in enc], enc=enc)
    good = G2.uncompressed(G2.G)
    unc = [G2.uncompressed(p) for p in pts]
    unc[1] = bytes([good[0] | 0x80]) + good[1:]         # compression bit set
    unc[2] = good[:191] + bytes([good[191] ^ 1])        # y off the curve
    unc[3] = bytes([0x40]) + bytes(190) + b"\x01"       # infinity with a payload
    unc[4] = good[:144] + P48                           # y.c0 = p
    undec = Table.of([G2.decode_result(G2.from_uncompressed(u)) for u in unc], enc=unc)
    sp = g2_special()
    sub = [G2.compress(p) for p in pts]
    sub[1], sub[2], sub[3] = G2.compress(sp["q1"]), G2.compress(sp["g+q1"]), G2.compress(sp["t13"])
    subgroup = Table.of([G2.decode_result(G2.decompress(c, check_subgroup=True)) for c in sub], enc=sub)
    return comp, raw, dec, undec, subgroup


def jj_records(points):
    return [(J.point_bytes(p), 1 if p == J.NEUTRAL else 0) for p in points]


@functools.lru_cache(maxsize=None)
def jubjub_tables():
    """(variable base under validation, variable base for the secret-scalar form, fixed base, [u1]G - [u2]Q under validation,
    compress, decompress)"""
    rng = random.Random(909)
    small = J.small_order_points(rng)
    pool = [J.mul(J.G, rng.randrange(1, J.R)) for _ in range(5)] + [J.random_point(rng) for _ in range(3)]
    units = [(0, pool[0]), (J.R, J.G), (8 * J.R, J.add(J.G, small[8])), (5, None), (J.R, small[8]), (8 * J.R, pool[6]),
             ((1 << 256) - 1, pool[5])]
    units += [(rng.randrange(1 << 256) if i % 2 else rng.randrange(J.R), pool[i % len(pool)]) for i in range(PERIOD - len(units))]
    off_curve = J.G[0].to_bytes(32, "big") + ((J.G[1] + 1) % J.Q).to_bytes(32, "big")
    ks = [kb32(k) for k, _ in units]
    good = [(k, pool[1] if p is None else p) for k, p in units]
    res_ct = jj_records(J.mul_many([p for _, p in good], [k for k, _ in good]))
    res = [(bytes(64), 2) if p is None else r for (_, p), r in zip(units, res_ct)]
    var = Table.of(res, scalars=ks, points=[off_curve if p is None else J.point_bytes(p) for _, p in units])
    var_ct = Table.of(res_ct, scalars=ks, points=[J.point_bytes(p) for _, p in good])
    base = Table.of(jj_records(J.mul_many([J.G] * PERIOD, [k for k, _ in units])), scalars=ks)
    u1 = [rng.randrange(1 << 256) for _ in range(PERIOD)]
    u2, qs = [k for k, _ in good], [p for _, p in good]
    u1[0], u2[0] = 0, 0                                 # neutral
    u1[1], u2[1], qs[1] = 9, 9, J.G                     # [9]G - [9]G
    fused_res = jj_records(J.double_mul_many(u1, u2, qs, True))
    fused_res[3] = (bytes(64), 2)
    fused = Table.of(fused_res, u1=[kb32(k) for k in u1], u2=[kb32(k) for k in u2], q=var.cols["points"])
    pts = [J.G, J.NEUTRAL, small[2], small[4], small[8], (0, J.Q - 1)] + pool[:7]
    comp = Table([J.compress(p) for p in pts], [0] * PERIOD, xy=[J.point_bytes(p) for p in pts])
    nosq = next(y for y in range(2, 100) if not J.is_square((y * y - 1) * pow(J.D * y * y + 1, -1, J.Q)))
    top = lambda b: b[:31] + bytes([b[31] | 0x80])
    enc = [J.compress(p) for p in pts]
    enc[1] = J.Q.to_bytes(32, "little")                 # y >= q
    enc[2] = nosq.to_bytes(32, "little")                # no point above y
    enc[3] = top((1).to_bytes(32, "little"))            # x = 0 with the sign bit set
    dres = [(bytes(64), 2) if J.decompress(c) is None else (J.point_bytes(J.decompress(c)), 0) for c in enc]
    dec = Table.of(dres, enc=enc)
    return var, var_ct, base, fused, comp, dec


class U64:
    def __init__(self, name):
        self.name, self.g2 = name, name == G2N
        self.group = B._G2 if self.g2 else B._G1
        self.pb = 192 if self.g2 else 96
        self.off = G2.torsion_point(13) if self.g2 else M.point_off_subgroup()  # G2: of order 13; G1: outside the subgroup


@functools.lru_cache(maxsize=None)
def u64_table(name):
    cv = U64(name)
    rng = random.Random(64 + cv.pb)
    pts = [cv.group.mul(rng.randrange(1, ORDER), cv.group.gen) for _ in range(PERIOD)]
    cs = [rng.randrange(1 << 64) for _ in range(PERIOD)]
    inf = [0] * PERIOD
    cs[0], cs[1], cs[2] = 0, 1, (1 << 64) - 1
    cs[3], pts[3] = 13 * rng.randrange(1, 1 << 59), cv.off  # G2: a multiple of the point's order, the identity
    cs[4], inf[4] = 5, 1
    cs[5], inf[5] = 5, 2
    pts[6] = cv.off
    res = []
    for c, p, f in zip(cs, pts, inf):
        res.append((bytes(cv.pb), 2) if f == 2 else BR.record(cv.group, None if f == 1 else BR.scalarmul_u64(cv.group, c, p)))
    recs = [b"\xff" * cv.pb if f == 1 else BR.record(cv.group, p)[0] for p, f in zip(pts, inf)]
    return Table.of(res, coeffs=[c.to_bytes(8, "big") for c in cs], points=recs, inf=[bytes([f]) for f in inf])


class SumPool:
    """13 multiples r_j G with r_0 + r_1 + r_2 = 0 and r_0 + .. + r_12 = 0 (mod r): member t of a call is row t % 13, so a
    group is known by (start % 13, length) and its sum is ONE model multiplication"""

    def __init__(self, name):
        self.name, self.g2 = name, name == G2N
        self.pb = 192 if self.g2 else 96
        rng = random.Random(130 + self.pb)
        rs = [rng.randrange(1, ORDER) for _ in range(PERIOD)]
        rs[2] = (-rs[0] - rs[1]) % ORDER
        rs[12] = (-sum(rs[:12])) % ORDER
        self.rs = rs
        self.recs = [self.record_of(r)[0] for r in rs]
        self._sums = {}

    def record_of(self, k):
        return G2.to_record(G2.mul(k % ORDER, G2.G)) if self.g2 else M.record(M.R.affine_mul(M.C, k % ORDER, M.G))

    def expect(self, start, length):
        key = (start % PERIOD, length)
        if key not in self._sums:
            self._sums[key] = self.record_of(sum(self.rs[(start + t) % PERIOD] for t in range(length)))
        return self._sums[key]


@functools.lru_cache(maxsize=None)
def sum_pool(name):
    return SumPool(name)


@functools.lru_cache(maxsize=None)
def pairing_terms():
    """the 13 terms of tests/test_pairing_gpu.py's `terms` fixture (same seed), their records and e(P, Q)"""
    rng = np.random.default_rng(381)
    sc = [(int.from_bytes(rng.bytes(32), "big") % PR.R, int.from_bytes(rng.bytes(32), "big") % PR.R) for _ in range(PERIOD)]
    sc[0], sc[1] = (1, 1), (0x9E3779B97F4A7C15, 0xDEADBEEF)
    pts = [(PR.g1_mul(a), PR.g2_mul(b)) for a, b in sc]
    recs = [(PR.g1_record(p)[0], G2.to_record(q)[0]) for p, q in pts]
    vals = [PR.pairing(p, q) for p, q in pts]
    return pts, recs, vals


GROUP_CYCLE = (1, 2, 1, 0, 3)


def pairing_product(start, length):
    vals = pairing_terms()[2]
    acc = PR.ONE12
    for t in range(length):
        acc = PR.f12_mul(acc, vals[(start + t) % PERIOD])
    return acc


def ragged(n, cycle, short_every=0, short=3):
    """(lengths, offsets) of n groups with lengths cycling through `cycle`; short_every: every such position is `short`"""
    lengths = np.asarray(cycle, dtype=np.int64)[np.arange(n) % len(cycle)]
    if short_every:
        lengths[short_every - 1::short_every] = short
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=offs[1:])
    return lengths, offs


def expect_by_key(offs, lengths, width, fn):
    """(n x width records, n flags): fn(start % 13, length) -> (record, flag), called once per distinct pair"""
    keys = (offs[:-1] % PERIOD) * (int(lengths.max()) + 1) + lengths
    uniq, inv = np.unique(keys, return_inverse=True)
    recs = [fn(int(k) // (int(lengths.max()) + 1), int(k) % (int(lengths.max()) + 1)) for k in uniq]
    rows = np.frombuffer(b"".join(r[0] for r in recs), dtype=np.uint8).reshape(len(uniq), width)
    flags = np.asarray([r[1] for r in recs], dtype=np.uint8)
    return rows[inv].copy(), flags[inv].copy()


def test_tables_have_the_required_rows():
    """every 13-row table, built from the models alone: flags 0, 1 and 2 present where the entry point has them, rows of
    one width, and the tiling itself"""
    assert math.gcd(PERIOD, GC.WAVE) == 1 and math.gcd(PERIOD, GC.WG) == 1
    for cus in (1, 80, 256, 304):
        n = GC.second_trip_units(cus)
        assert GC.second_trip_units(cus, per_cu=16) == 16 * cus * 256 + 300
        assert n == 8 * cus * 256 + 300 and n % 256 == 44 and (n - 8 * cus * 256) // 256 == 1
        assert GC.second_trip_wave_groups(cus) == 32 * cus + 37
    assert GC.second_trip_units(256) == 524588
    var, base = g2_var_table()
    comp, raw, dec, undec, subgroup = g2_codec_tables()
    jvar, jvar_ct, jbase, jfused, jcomp, jdec = jubjub_tables()
    all_three = {"g2 var": var, "g2 add": g2_add_table(), "g2 decompress": dec, "g2 from_uncompressed": undec,
                 "g2 subgroup": subgroup, "jubjub var": jvar, "jubjub fused": jfused, "u64 g1": u64_table(G1N), "u64 g2": u64_table(G2N)}
    for name, t in all_three.items():
        assert set(t.flags) == {0, 1, 2}, name
        assert t.flags.count(0) >= 6, name
    for name, t in {"g2 base": base, "jubjub var ct": jvar_ct, "jubjub base": jbase}.items():
        assert set(t.flags) == {0, 1}, name
    assert set(jdec.flags) == {0, 2}                      # jubjub's neutral element decodes as a point
    assert subgroup.flags[1:4] == [2, 2, 2] and dec.flags[1:5] == [2, 2, 2, 2] and undec.flags[1:5] == [2, 2, 2, 2]
    assert [f for f in comp.cols["inf"]].count(b"\1") == 2
    for t in list(all_three.values()) + [base, comp, raw, jvar_ct, jbase, jcomp, jdec]:
        for col in list(t.cols.values()) + [t.want]:
            assert len({len(r) for r in col}) == 1
        for w, f in zip(t.want, t.flags):
            assert f != 2 or not any(w)
    # rejected and identity rows of G2 and G1 are zero bytes; jubjub's neutral element is (0, 1)
    assert all(not any(w) for w, f in zip(var.want, var.flags) if f)
    assert all(w == J.point_bytes(J.NEUTRAL) for w, f in zip(jbase.want, jbase.flags) if f == 1)
    # sums: a group that sums to the identity in both shapes
    for name in (G1N, G2N):
        sp = sum_pool(name)
        assert sp.expect(0, 3)[1] == 1 and sp.expect(4, 65)[1] == 1 and sp.expect(0, 0)[1] == 1 and sp.expect(5, 7)[1] == 0
        assert len(set(sp.recs)) == PERIOD
    # the pairing's terms: 13 distinct values, and the ragged cycle meets every (start, length)
    _, recs, vals = pairing_terms()
    assert len({PR.f12_to_bytes(v) for v in vals}) == PERIOD and PR.ONE12 not in vals
    lengths, offs = ragged(5 * PERIOD * 3, GROUP_CYCLE)
    assert len(set(zip((offs[:-1] % PERIOD).tolist(), lengths.tolist()))) == len(set(GROUP_CYCLE)) * PERIOD
    # tile: unit i is row i % 13, for tables given as byte strings and as arrays
    for n in (1, 13, 300, 1000):
        tiled = GC.tile(var.want, n)
        assert tiled.shape == (n, 192) and all(tiled[i].tobytes() == var.want[i % PERIOD] for i in range(n))
        assert np.array_equal(GC.tile(GC.tile(var.want, PERIOD), n), tiled)
        assert GC.tile_flags(var.flags, n).tolist() == [var.flags[i % PERIOD] for i in range(n)]


# ---- the GPU side -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_mod():
    import torch

    return torch


@pytest.fixture(scope="module")
def eng():
    import eccoxide_amd as E

    with E.Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def units():
    n = GC.second_trip_units(GC.device_cus())
    assert n % GC.WG == 44
    return n


class Run:
    """uploads tiled columns, hands out 0xAA-filled outputs and compares whole arrays"""

    def __init__(self, torch, n):
        self.torch, self.n = torch, n

    def col(self, table, name):
        return self.up(GC.tile(table.cols[name], self.n))

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        return self.torch.from_numpy(arr if arr.flags.writeable else arr.copy()).cuda().reshape(-1)

    def aa(self, n, width=1):
        return self.torch.full((n * width,), 0xAA, dtype=self.torch.uint8, device="cuda")

    def same(self, out, flags, table, label=""):
        self.torch.cuda.synchronize()
        if flags is not None:
            assert np.array_equal(flags.cpu().numpy().reshape(-1), GC.tile_flags(table.flags, self.n)), f"{label}: flags"
        want = GC.tile(table.want, self.n)
        assert np.array_equal(out.cpu().numpy().reshape(self.n, want.shape[1]), want), f"{label}: records"

    def same_arrays(self, out, flags, want, wflags, label=""):
        self.torch.cuda.synchronize()
        assert np.array_equal(flags.cpu().numpy().reshape(-1), wflags), f"{label}: flags"
        assert np.array_equal(out.cpu().numpy().reshape(want.shape), want), f"{label}: records"


@pytest.fixture()
def run(torch_mod, units):
    return Run(torch_mod, units)


@pytest.fixture()
def run16(torch_mod):
    """the fixed-base combs run on grid(ctx, n, 16), sixteen workgroups per CU whatever is resident: twice the units"""
    return Run(torch_mod, GC.second_trip_units(GC.device_cus(), per_cu=16))


@gpu
@pytest.mark.parametrize("ct", [False, True], ids=["public", "ct_scan"])
def test_g2_scalarmul_var(eng, run, ct):
    var, _ = g2_var_table()
    out, fl = eng.scalarmul_var_t(G2N, run.col(var, "scalars"), run.col(var, "points"), run.aa(run.n, 192), run.aa(run.n),
                                  validate=True, ct_scan=ct)
    run.same(out, fl, var, f"k_g2_scalarmul_var ct_scan={ct}")


@gpu
@pytest.mark.parametrize("ct", [False, True], ids=["public", "ct_scan"])
def test_g2_scalarmul_base(eng, run16, ct):
    run = run16
    _, base = g2_var_table()
    out, fl = eng.scalarmul_base_t(G2N, run.col(base, "scalars"), run.aa(run.n, 192), run.aa(run.n), ct_scan=ct)
    run.same(out, fl, base, f"k_g2_scalarmul_base ct_scan={ct}")


@gpu
def test_g2_point_add(eng, run):
    t = g2_add_table()
    out, fl = eng.point_add_t(G2N, run.col(t, "a"), run.col(t, "b"), run.aa(run.n, 192), run.aa(run.n),
                              a_inf=run.col(t, "a_inf"), b_inf=run.col(t, "b_inf"))
    run.same(out, fl, t, "k_g2_point_add")


@gpu
def test_g2_codec(eng, run):
    comp, raw, dec, undec, subgroup = g2_codec_tables()
    xy, inf = run.col(comp, "xy"), run.col(comp, "inf")
    run.same(eng.point_compress_t(G2N, xy, inf, run.aa(run.n, 96)), None, comp, "k_g2_compress")
    run.same(eng.point_compress_t(G2N, xy, inf, run.aa(run.n, 192), uncompressed=True), None, raw, "k_g2_compress uncompressed")
    del xy, inf
    out, fl = eng.point_decompress_t(G2N, run.col(dec, "enc"), run.aa(run.n, 192), run.aa(run.n))
    run.same(out, fl, dec, "k_g2_decompress")
    out, fl = eng.point_decompress_t(G2N, run.col(undec, "enc"), run.aa(run.n, 192), run.aa(run.n), uncompressed=True)
    run.same(out, fl, undec, "k_g2_from_uncompressed")


@gpu
def test_g2_subgroup_check(eng, run):
    subgroup = g2_codec_tables()[4]
    out, fl = eng.point_decompress_t(G2N, run.col(subgroup, "enc"), run.aa(run.n, 192), run.aa(run.n), check_subgroup=True)
    run.same(out, fl, subgroup, "k_g2_subgroup_check")


@gpu
def test_jubjub_variable_base(eng, run):
    var, var_ct = jubjub_tables()[:2]
    out, fl = eng.scalarmul_var_t(JJ, run.col(var, "scalars"), run.col(var, "points"), run.aa(run.n, 64), run.aa(run.n), validate=True)
    run.same(out, fl, var, "jubjub var, public")
    out, fl = eng.scalarmul_var_t(JJ, run.col(var_ct, "scalars"), run.col(var_ct, "points"), run.aa(run.n, 64), run.aa(run.n), ct_scan=True)
    run.same(out, fl, var_ct, "jubjub var, ct_scan")


@gpu
def test_jubjub_fixed_base(eng, run16):
    run, base = run16, jubjub_tables()[2]
    ks = run.col(base, "scalars")
    for ct in (False, True):
        out, fl = eng.scalarmul_base_t(JJ, ks, run.aa(run.n, 64), run.aa(run.n), ct_scan=ct)
        run.same(out, fl, base, f"jubjub base ct_scan={ct}")


@gpu
def test_jubjub_fused(eng, run):
    fused = jubjub_tables()[3]
    out, fl = eng.double_scalarmul_t(JJ, run.col(fused, "u1"), run.col(fused, "u2"), run.col(fused, "q"), run.aa(run.n, 64),
                                     run.aa(run.n), subtract=True, validate=True)
    run.same(out, fl, fused, "jubjub [u1]G - [u2]Q")


@gpu
def test_jubjub_codec(eng, run):
    comp, dec = jubjub_tables()[4:6]
    run.same(eng.point_compress_t(JJ, run.col(comp, "xy"), None, run.aa(run.n, 32)), None, comp, "jubjub compress")
    out, fl = eng.point_decompress_t(JJ, run.col(dec, "enc"), run.aa(run.n, 64), run.aa(run.n))
    run.same(out, fl, dec, "jubjub decompress")


@gpu
@pytest.mark.parametrize("name", [G1N, G2N], ids=["g1", "g2"])
def test_scalarmul_u64(eng, run, name):
    t = u64_table(name)
    pb = len(t.want[0])
    cs, pts, inf = run.col(t, "coeffs"), run.col(t, "points"), run.col(t, "inf")
    out, fl = eng.scalarmul_u64_t(name, cs, pts, inf, run.aa(run.n, pb), run.aa(run.n))
    run.same(out, fl, t, "k_scalarmul_u64, separate outputs")
    del out, fl
    # in place: a lane of the second trip must still find its own unread operand
    eng.scalarmul_u64_t(name, cs, pts, inf, pts, inf)
    run.same(pts, inf, t, "k_scalarmul_u64, in place")


def _sum_inputs(run, sp, members):
    return run.up(GC.tile(sp.recs, members))


@gpu
@pytest.mark.parametrize("name", [G1N, G2N], ids=["g1", "g2"])
def test_point_sum_short_groups(eng, run, torch_mod, name):
    """k_point_sum_short: one lane per group, lengths 0 .. 7; in the second trip one group holds a member flagged 2 and one
    range decreases (its successor then starts one member early): both are rejected alone"""
    sp, n = sum_pool(name), run.n
    lengths, offs = ragged(n, range(8))
    bad_member = n - 150 + int(np.argmax(lengths[n - 150:] >= 2))
    bad_range = n - 60 + int(np.argmax(lengths[n - 60:] == 0))  # an empty group: its successor stays a short one
    assert n - 300 <= bad_member < bad_range < n - 1 and lengths[bad_member] >= 2 and lengths[bad_range] == 0
    members = int(offs[-1])
    inf = np.zeros(members, dtype=np.uint8)
    inf[offs[bad_member] + 1] = 2
    offs[bad_range + 1] = offs[bad_range] - 1
    lengths = np.diff(offs)
    assert (lengths < 0).sum() == 1 and lengths[bad_range] == -1 and lengths.max() == 7
    want, wfl = expect_by_key(offs, np.maximum(lengths, 0), sp.pb, sp.expect)
    for g in (bad_member, bad_range):
        want[g], wfl[g] = 0, 2
    assert {0, 1, 2} <= set(wfl[n - 300:].tolist())
    out, fl = eng.point_sum_t(name, _sum_inputs(run, sp, members), torch_mod.from_numpy(offs + 5).cuda(), run.aa(n, sp.pb), run.aa(n),
                              inf=run.up(inf))
    run.same_arrays(out, fl, want, wfl, "k_point_sum_short")


@gpu
@pytest.mark.parametrize("name", [G1N, G2N], ids=["g1", "g2"])
def test_point_sum_wave_groups(eng, run, torch_mod, name):
    """k_point_sum: one wave per group over 32 * CUs + 37 groups, the LDS tree at every span (8, 9, 63, 64, 65, 70 members),
    and a group of 3 at every 11th position, which the wave passes over between two long groups"""
    sp = sum_pool(name)
    n = GC.second_trip_wave_groups(GC.device_cus())
    lengths, offs = ragged(n, (8, 9, 63, 64, 65, 70), short_every=11)
    assert (lengths == 3).sum() >= n // 11 and (lengths[-37:] == 3).any()
    want, wfl = expect_by_key(offs, lengths, sp.pb, sp.expect)
    assert {0, 1} <= set(wfl[-37:].tolist())
    out, fl = eng.point_sum_t(name, _sum_inputs(run, sp, int(offs[-1])), torch_mod.from_numpy(offs).cuda(), run.aa(n, sp.pb), run.aa(n))
    run.same_arrays(out, fl, want, wfl, "k_point_sum")


def _group_inputs(n):
    """n ragged groups over the 13 terms; near the end one group of two terms (-P, Q), (P, Q), whose product is 1, and one
    group of three whose middle term is off the curve.  k_pgroups_miller and k_pgroups_product loop over the chunk slots,
    4 n / 5 here (one per group that is not empty): 419670 on 256 CUs against 256 * CUs and 512 * CUs slots per trip (306
    and 185 VGPRs: one and two workgroups per CU), so both stride -- as long as the occupancy is at most 6, not
    'whatever the query answers'.  Every group is one chunk: the product lanes find no work.  k_pgroups_prepare and
    k_pgroups_gather run on up to 4096 workgroups (2^20 terms, 2^20 groups) and take one trip."""
    pts, recs, _ = pairing_terms()
    lengths, offs = ragged(n, GROUP_CYCLE)
    terms = int(offs[-1])
    g1 = GC.tile([r[0] for r in recs], terms)
    g2 = GC.tile([r[1] for r in recs], terms)
    one_at = n - 150 + (1 - (n - 150) % 5) % 5       # a group of two terms
    bad_at = n - 40 + (4 - (n - 40) % 5) % 5         # a group of three
    assert lengths[one_at] == 2 and lengths[bad_at] == 3 and n - 300 <= one_at < bad_at < n
    t, k = int(offs[one_at]), 7
    g1[t] = np.frombuffer(PR.g1_record(PR.g1_neg(pts[k][0]))[0], dtype=np.uint8)
    g1[t + 1] = np.frombuffer(recs[k][0], dtype=np.uint8)
    g2[t] = g2[t + 1] = np.frombuffer(recs[k][1], dtype=np.uint8)
    x, y = PR.G1
    g1[int(offs[bad_at]) + 1] = np.frombuffer(x.to_bytes(48, "big") + ((y + 1) % PR.P).to_bytes(48, "big"), dtype=np.uint8)
    want, wfl = expect_by_key(offs, lengths, GB, lambda s, length: (PR.f12_to_bytes(pairing_product(s, length)), 0))
    want[one_at] = np.frombuffer(PR.ONE_BYTES, dtype=np.uint8)
    want[bad_at], wfl[bad_at] = 0, 2
    verdicts = np.where(lengths == 0, 1, 0).astype(np.uint8)
    verdicts[one_at], verdicts[bad_at] = 1, 2
    return g1, g2, offs, want, wfl, verdicts


@gpu
def test_pairing_groups_values(eng, run, torch_mod):
    g1, g2, offs, want, wfl, _ = _group_inputs(run.n)
    out, fl = eng.pairing_groups_t(run.up(g1), run.up(g2), torch_mod.from_numpy(offs).cuda(), run.aa(run.n, GB), run.aa(run.n), validate=True)
    run.same_arrays(out, fl, want, wfl, "pairing_groups")


@gpu
def test_pairing_groups_verdicts(eng, run, torch_mod):
    from eccoxide_amd import engine as EN

    assert (EN.PAIRING_NOT_ONE, EN.PAIRING_ONE, EN.PAIRING_REJECTED) == (0, 1, 2)
    g1, g2, offs, _, _, verdicts = _group_inputs(run.n)
    v = eng.pairing_check_groups_t(run.up(g1), run.up(g2), torch_mod.from_numpy(offs).cuda(), run.aa(run.n), validate=True)
    torch_mod.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy(), verdicts)
    assert {0, 1, 2} <= set(verdicts[-300:].tolist())


@gpu
def test_pairing_groups_one_long_group(eng, run, torch_mod):
    """one group of 9 n / 8 terms, 73771 chunks of 8 on 256 CUs: more than the 256 * CUs slots k_pgroups_miller covers in
    one trip (306 VGPRs: one workgroup per CU), so the Miller pass strides inside one group.  k_pgroups_product (185 VGPRs,
    two workgroups per CU, 512 * CUs slots) covers these chunks in one trip: its second trip is
    test_pairing_groups_two_chunk_groups'."""
    _, recs, vals = pairing_terms()
    terms = 9 * run.n // 8
    g1, g2 = run.up(GC.tile([r[0] for r in recs], terms)), run.up(GC.tile([r[1] for r in recs], terms))
    offs = torch_mod.tensor([0, terms], dtype=torch_mod.int64).cuda()
    acc = PR.ONE12
    for j in range(PERIOD):
        acc = PR.f12_mul(acc, PR.f12_pow(vals[j], len(range(j, terms, PERIOD))))
    out, fl = eng.pairing_groups_t(g1, g2, offs, run.aa(1, GB), run.aa(1))
    v = eng.pairing_check_groups_t(g1, g2, offs, run.aa(1))
    torch_mod.cuda.synchronize()
    assert (out.cpu().numpy().tobytes(), fl.cpu().numpy().tobytes(), v.cpu().numpy().tobytes()) == (PR.f12_to_bytes(acc), b"\0", b"\0")


@gpu
def test_pairing_groups_two_chunk_groups(eng, run, torch_mod):
    """256 * CUs + 300 groups of 9 terms, two chunks each: 512 * CUs + 600 chunk slots, more than k_pgroups_product covers
    in one trip at its two workgroups per CU, so the lanes of its second trip multiply two chunk values each (`work`);
    in the tests above they only pass single-chunk groups by.  13 expected values: nine consecutive terms from start % 13."""
    _, recs, _ = pairing_terms()
    n = GC.WG * GC.device_cus() + GC.TAIL
    lengths, offs = ragged(n, (9,))
    terms = int(offs[-1])
    want, wfl = expect_by_key(offs, lengths, GB, lambda s, length: (PR.f12_to_bytes(pairing_product(s, length)), 0))
    out, fl = eng.pairing_groups_t(run.up(GC.tile([r[0] for r in recs], terms)), run.up(GC.tile([r[1] for r in recs], terms)),
                                   torch_mod.from_numpy(offs).cuda(), run.aa(n, GB), run.aa(n))
    torch_mod.cuda.synchronize()
    assert np.array_equal(fl.cpu().numpy(), wfl) and not wfl.any()
    assert np.array_equal(out.cpu().numpy().reshape(n, GB), want)


MSM_POOL = 1 << 19


@pytest.fixture(scope="module")
def msm_pool(eng):
    """tests/test_msm_gpu.py's pool (same seed): r_i and the records of r_i G for i < 2^19"""
    rng = np.random.default_rng(12381)
    rb = rng.bytes(32 * MSM_POOL)
    rs = [int.from_bytes(rb[32 * i:32 * i + 32], "big") % ORDER for i in range(MSM_POOL)]
    rs[0], rs[1] = 1, 2
    recs, fl = eng.scalarmul_base(G1N, b"".join(kb32(r) for r in rs))
    assert fl == bytes(MSM_POOL)
    return rs, np.frombuffer(recs, dtype=np.uint8).reshape(MSM_POOL, 96)


@gpu
def test_msm(eng, run, msm_pool):
    """k_msm_prepare<G, false / true> on a second trip whose last wave is partial; then the last 300 terms flagged 1 over
    0xEE bytes, which must contribute nothing"""
    rs, recs = msm_pool
    n = run.n
    idx = np.arange(n) % MSM_POOL
    kb = np.random.default_rng(n).bytes(32 * n)
    ks = [int.from_bytes(kb[32 * i:32 * i + 32], "big") for i in range(n)]
    total = 0
    for i in range(n - 300):
        total += ks[i] * rs[i % MSM_POOL]
    tail = sum(ks[i] * rs[i % MSM_POOL] for i in range(n - 300, n))
    d_k = run.up(np.frombuffer(kb, dtype=np.uint8))
    pts = recs[idx]
    out, fl = eng.msm_t(G1N, d_k, run.up(pts), run.aa(1, 96), run.aa(1))
    run.torch.cuda.synchronize()
    assert (out.cpu().numpy().tobytes(), fl.cpu().numpy()[0]) == M.record(M.R.affine_mul(M.C, (total + tail) % ORDER, M.G))
    pts[n - 300:] = 0xEE
    inf = np.zeros(n, dtype=np.uint8)
    inf[n - 300:] = 1
    out, fl = eng.msm_t(G1N, d_k, run.up(pts), run.aa(1, 96), run.aa(1), inf=run.up(inf))
    run.torch.cuda.synchronize()
    assert (out.cpu().numpy().tobytes(), fl.cpu().numpy()[0]) == M.record(M.R.affine_mul(M.C, total % ORDER, M.G))
