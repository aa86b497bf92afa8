"""eccx_point_sum / eccx_point_sum_dev through ctypes and libeccx.so against the Python models: one sum per ragged group
of points on BLS12-381 G1 (oracle/ecc_ref.py's textbook layer, as tests/msm_ref.py uses it) and G2 (tests/g2_ref.py).

Members are drawn from 13 multiples r_j G of the generator, so the expected value of a group is ONE model multiplication,
(sum r_j mod r) G, plus a model addition for every member that is no multiple of the generator (a point outside the
prime-order subgroup: the sum must hold for any curve point).  Each curve's table and expected values are made once per
module.  Group lengths sit around the kernel's boundaries: one wavefront sums a group, lane l folding members l, l + 64,
.. and the 64 partial sums halving through LDS, so 63 / 64 / 65 and 128 / 129 are where a lane gains a member and the
tree its full height; groups of at most 7 members are summed by one lane each, in a kernel of their own, so 7 / 8 is
where a group changes kernels."""
import ctypes

import numpy as np
import pytest

import eccoxide_amd as E
from eccoxide_amd import engine as EN
from oracle import ecc_ref as R1
from tests import g2_ref as G2
from tests import msm_ref as M

pytestmark = pytest.mark.gpu

ORDER = M.ORDER
P = M.C.p
ERR_ARG, ERR_CURVE = -2, -1
NMULT = 13
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 128, 129, 200)


class G1Model:
    name, pb = "bls12_381_g1", 96
    gen_mul = staticmethod(lambda k: R1.affine_mul(M.C, k % ORDER, M.G))
    add = staticmethod(lambda p, q: R1.affine_add(M.C, p, q))
    neg = staticmethod(M.neg)
    record = staticmethod(M.record)
    outsider = staticmethod(M.point_off_subgroup)  # a curve point outside G1

    @staticmethod
    def off_curve(p):
        return p[0].to_bytes(48, "big") + ((p[1] + 1) % P).to_bytes(48, "big")

    @staticmethod
    def big_x(p):  # the same residue, not canonical
        return (p[0] + P).to_bytes(48, "big") + p[1].to_bytes(48, "big")


class G2Model:
    name, pb = "bls12_381_g2", 192
    gen_mul = staticmethod(lambda k: G2.mul(k % ORDER, G2.G))
    add = staticmethod(G2.add)
    neg = staticmethod(G2.neg)
    record = staticmethod(G2.to_record)
    outsider = staticmethod(lambda: G2.torsion_point(13))  # a point of the twist of order 13

    @staticmethod
    def off_curve(p):
        return G2.f2_to_bytes(p[0]) + G2.f2_to_bytes(G2.f2_add(p[1], G2.ONE))

    @staticmethod
    def big_x(p):  # c0 of x lifted by p: the record is c1 || c0
        (x0, x1), y = p
        return x1.to_bytes(48, "big") + (x0 + P).to_bytes(48, "big") + G2.f2_to_bytes(y)


class Case:
    """The 13 multiples, the outsider, and the expected sums of groups given as lists of members: an int j stands for
    r_j G, ("pt", affine) for that point, ("raw", record bytes, flag) for bytes the model does not interpret."""

    def __init__(self, model):
        self.m = model
        rng = np.random.default_rng(381 + model.pb)
        rb = rng.bytes(32 * NMULT)
        self.rs = [int.from_bytes(rb[32 * j:32 * j + 32], "big") % ORDER for j in range(NMULT)]
        self.rs[2] = 1
        self.rs[12] = (-self.rs[0] - self.rs[1]) % ORDER  # r_0 G + r_1 G + r_12 G is the identity
        self.pts = [model.gen_mul(r) for r in self.rs]
        self.recs = [model.record(p)[0] for p in self.pts]
        self.out = model.outsider()
        self._sums = {}

    def member(self, x):
        """(record, flag byte, contribution to the scalar sum, explicit point to add)"""
        if isinstance(x, int):
            return self.recs[x], 0, self.rs[x], None
        if x[0] == "pt":
            return self.m.record(x[1])[0], 0, 0, x[1]
        return x[1], x[2], 0, None

    def expect(self, group):
        """(record, flag) of the group's sum"""
        if any(not isinstance(x, int) and x[0] == "raw" and x[2] == 2 for x in group):
            return bytes(self.m.pb), 2
        k = sum(self.member(x)[2] for x in group) % ORDER
        if k not in self._sums:
            self._sums[k] = self.m.gen_mul(k)
        acc = self._sums[k]
        for x in group:
            extra = self.member(x)[3]
            if extra is not None:
                acc = self.m.add(acc, extra)
        return self.m.record(acc)

    def pack(self, groups):
        """(points bytes, inf bytes, offsets) of the groups back to back"""
        pts, inf, offs = [], bytearray(), [0]
        for g in groups:
            for x in g:
                rec, fl, _, _ = self.member(x)
                pts.append(rec)
                inf.append(fl)
            offs.append(len(inf))
        return b"".join(pts), bytes(inf), np.array(offs, dtype=np.uint64)


@pytest.fixture(scope="module", params=[G1Model, G2Model], ids=["g1", "g2"])
def case(request):
    return Case(request.param)


@pytest.fixture(scope="module")
def eng():
    with E.Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    return torch


def split(out, flags, pb):
    return [(out[pb * i:pb * i + pb], flags[i]) for i in range(len(flags))]


def boundary_groups(c):
    """The lengths around the lane and tree boundaries, and the special groups; returns (groups, indices of the groups that
    only ECCX_VALIDATE_POINTS rejects)."""
    groups = [[(7 * n + 3 * i) % NMULT for i in range(n)] for n in LENGTHS]
    garbage = ("raw", b"\xff" * c.m.pb, 1)
    groups += [
        [5] * 64,                                       # 64 equal points: every tree round is a doubling
        [3, ("pt", c.m.neg(c.pts[3])), 7],              # P, -P, Q
        [0, 1, 12],                                     # sums to the identity
        [("pt", c.m.neg(c.pts[4]))] + [4],              # ... and so do a point and its negative alone
        [3, garbage, 4, garbage],                       # members flagged 1 over garbage bytes
        [garbage] * 3,                                  # ... and nothing else: the identity
        [1, 2, ("raw", c.recs[6], 2), 8],               # one member flagged 2
        [("pt", c.out), 9, ("pt", c.out)] + [10] * 70,  # a curve point outside the prime-order subgroup, twice
        [("pt", c.out), 9, ("pt", c.out)],              # ... and in a group one lane sums
        [(3 * i + 1) % NMULT for i in range(7)],        # the longest group one lane sums
        [(3 * i + 2) % NMULT for i in range(8)],        # ... and the shortest a wavefront does
    ]
    only_validated = [len(groups), len(groups) + 1]
    groups += [
        [2, ("raw", c.m.off_curve(c.pts[5]), 0), 6],    # off the curve
        [("raw", c.m.big_x(c.pts[5]), 0)] * 2 + [11],   # x >= p
    ]
    return groups, only_validated


def test_boundary_lengths_and_special_members(eng, case):
    c = case
    groups, only_validated = boundary_groups(c)
    pts, inf, offs = c.pack(groups)
    want = [c.expect(g) for g in groups]
    assert want[LENGTHS.index(0)] == (bytes(c.m.pb), 1)
    assert want[len(LENGTHS) + 2] == (bytes(c.m.pb), 1) and want[len(LENGTHS) + 3] == (bytes(c.m.pb), 1)
    got = split(*eng.point_sum(c.m.name, pts, offs, inf=inf, validate=True), c.m.pb)
    for i in only_validated:
        want[i] = (bytes(c.m.pb), 2)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(groups[i]))
    # without the validation the same groups stand, apart from the two whose members are no curve points (unspecified)
    plain = split(*eng.point_sum(c.m.name, pts, offs + 11, inf=inf), c.m.pb)  # offsets[0] != 0: only differences count
    for i, (g, w) in enumerate(zip(plain, want)):
        if i not in only_validated:
            assert g == w, i
    # inf == NULL: every member counts (the groups without flagged members)
    clean = [g for g in groups[:len(LENGTHS) + 3]]
    pts2, _, offs2 = c.pack(clean)
    assert split(*eng.point_sum(c.m.name, pts2, offs2), c.m.pb) == [c.expect(g) for g in clean]


def test_many_short_and_few_long_groups(eng, case):
    """700 groups of 1 to 3 members and 3 groups of 1500: more groups than a launch has wavefronts resident on a small
    grid's stride, and chains of 24 additions per lane"""
    c = case
    groups = [[(i + t) % NMULT for t in range(1 + i % 3)] for i in range(700)]
    groups += [[(5 * i + s) % NMULT for i in range(1500)] for s in range(3)]
    pts, inf, offs = c.pack(groups)
    got = split(*eng.point_sum(c.m.name, pts, offs), c.m.pb)
    for i, g in enumerate(groups):
        assert got[i] == c.expect(g), i


def _dev(torch, b, lead=0):
    t = torch.frombuffer(bytearray(bytes(lead) + b), dtype=torch.uint8).cuda()
    return t[lead:lead + len(b)]


def _host(out, flags, pb):
    return split(out.cpu().numpy().tobytes(), flags.cpu().numpy().tobytes(), pb)


def test_dev_form(eng, torch_mod, case):
    c, torch = case, torch_mod
    groups, only_validated = boundary_groups(c)
    groups = [g for i, g in enumerate(groups) if i not in only_validated]
    pts, inf, offs = c.pack(groups)
    want = [c.expect(g) for g in groups]
    side = torch.cuda.Stream()
    d_offs = torch.from_numpy((offs + 7).astype(np.int64)).cuda()
    d_pts, d_inf = _dev(torch, pts), _dev(torch, inf)
    torch.cuda.synchronize()
    res = eng.point_sum_t(c.m.name, d_pts, d_offs, inf=d_inf, stream=side.cuda_stream)
    side.synchronize()
    assert _host(*res, c.m.pb) == want
    # a sub-batch with its own offsets[0], records and flags at odd addresses
    lo, hi = 4, len(LENGTHS)
    a = int(offs[lo])
    for lead in (1, 3):
        res = eng.point_sum_t(c.m.name, _dev(torch, pts[c.m.pb * a:], lead), d_offs[lo:hi + 1], inf=_dev(torch, inf[a:], lead))
        torch.cuda.synchronize()
        assert _host(*res, c.m.pb) == want[lo:hi], lead
    # the same input twice gives the same bytes
    again = eng.point_sum_t(c.m.name, d_pts, d_offs, inf=d_inf)
    torch.cuda.synchronize()
    assert _host(*again, c.m.pb) == want
    # no groups
    none = eng.point_sum_t(c.m.name, d_pts, d_offs[:1])
    torch.cuda.synchronize()
    assert none[0].numel() == 0 and none[1].numel() == 0


def test_dev_form_rejects_bad_ranges_alone(eng, torch_mod, case):
    """A range that decreases, one that starts below offsets[0] and one that ends beyond the members are rejected, read
    nothing, and leave the other groups standing."""
    c, torch = case, torch_mod
    members = [j % NMULT for j in range(10)]
    pts = b"".join(c.recs[j] for j in members)
    base = 100
    #        group: 0      1 (decreases)  2          3 (below offsets[0])  4 (from below up)  5          6 (beyond)
    rel = [0, 5, 3, 8, -2, 6, 10, 11]
    d_offs = torch.tensor([base + r for r in rel], dtype=torch.int64).cuda()
    want = [c.expect(members[0:5]), (bytes(c.m.pb), 2), c.expect(members[3:8]), (bytes(c.m.pb), 2), (bytes(c.m.pb), 2),
            c.expect(members[6:10]), (bytes(c.m.pb), 2)]
    res = eng.point_sum_t(c.m.name, _dev(torch, pts), d_offs)
    torch.cuda.synchronize()
    assert _host(*res, c.m.pb) == want
    # far beyond: the records end where `members` says, whatever the offsets claim
    d_far = torch.tensor([0, 4, 1 << 40, (1 << 40) + 3, (1 << 62)], dtype=torch.int64).cuda()
    res = eng.point_sum_t(c.m.name, _dev(torch, pts), d_far)
    torch.cuda.synchronize()
    assert _host(*res, c.m.pb) == [c.expect(members[0:4])] + [(bytes(c.m.pb), 2)] * 3


def test_reserve_covers_the_dev_call(torch_mod, case):
    c, torch = case, torch_mod
    groups = [[(i + t) % NMULT for t in range(1 + i % 3)] for i in range(300)]
    pts, _, offs = c.pack(groups)
    d_pts, d_offs = _dev(torch, pts), torch.from_numpy(offs.astype(np.int64)).cuda()
    with E.Engine(0) as fresh:
        fresh.reserve(c.m.name, len(groups), var=False)
        before = fresh.device_bytes()
        assert before > 0
        big = fresh.point_sum_t(c.m.name, d_pts, d_offs)
        small = fresh.point_sum_t(c.m.name, d_pts, d_offs[:41])
        torch.cuda.synchronize()
        assert _host(*big, c.m.pb) == [c.expect(g) for g in groups]
        assert _host(*small, c.m.pb) == [c.expect(g) for g in groups[:40]]
        assert fresh.device_bytes() == before


def test_host_form_checks_offsets_and_arguments(eng, case):
    c = case
    lib, ctx = eng._lib, eng._ctx
    cid = EN.CURVE_IDS[c.m.name]
    pb = c.m.pb
    pts = c.recs[0] + c.recs[1] + c.recs[2]
    mark = b"\x5a" * (2 * pb)
    out, fl = ctypes.create_string_buffer(mark, 2 * pb), ctypes.create_string_buffer(b"\x5a\x5a", 2)
    untouched = lambda: (out.raw, fl.raw) == (mark, b"\x5a\x5a")
    err = lambda: lib.eccx_last_error(ctx).decode()

    def host(curve, n, o, members, p, opts=0, o_=out, f_=fl):
        keep = np.array(o, dtype=np.uint64) if o is not None else None
        return lib.eccx_point_sum(ctx, curve, n, keep.ctypes.data if keep is not None else None, members, p, None, o_, f_, opts)

    served = {EN.CURVE_IDS["bls12_381_g1"], EN.CURVE_IDS["bls12_381_g2"]}
    for name, other in EN.CURVE_IDS.items():
        if other not in served:
            assert host(other, 2, (0, 1, 3), 3, pts) == ERR_ARG and untouched(), name
            assert lib.eccx_point_sum_dev(ctx, other, 2, None, 3, None, None, None, None, 0, None) == ERR_ARG, name
    for bad_id in (-1, 6, 8, 10, 99):
        assert host(bad_id, 2, (0, 1, 3), 3, pts) == ERR_CURVE and untouched(), bad_id
        assert lib.eccx_point_sum_dev(ctx, bad_id, 2, None, 3, None, None, None, None, 0, None) == ERR_CURVE, bad_id
    refused = [EN.MIRROR_REFERENCE, EN.TABLE_IN_LDS, EN.SUBTRACT, EN.CHECK_SUBGROUP, EN.UNCOMPRESSED, EN.CT_SCAN, EN.ASSUME_SUBGROUP,
               EN.CT_GATHER, 1 << 3, 1 << 4, 1 << 14, 1 << 20, 1 << 31, EN.CT_SCAN | EN.VALIDATE_POINTS]
    for bad in refused:
        assert host(cid, 2, (0, 1, 3), 3, pts, bad) == ERR_ARG and "opts" in err() and untouched(), bad
        assert host(cid, 0, None, 0, None, bad) == ERR_ARG and untouched(), bad
        assert lib.eccx_point_sum_dev(ctx, cid, 2, None, 3, None, None, None, None, bad, None) == ERR_ARG and "opts" in err(), bad
    # offsets that decrease, or whose span leaves the members: refused before the device is touched
    assert host(cid, 2, (0, 2, 1), 3, pts) == ERR_ARG and "decrease" in err() and untouched()
    assert host(cid, 2, (5, 4, 6), 3, pts) == ERR_ARG and "decrease" in err() and untouched()
    assert host(cid, 2, (0, 1, 4), 3, pts) == ERR_ARG and "beyond" in err() and untouched()
    assert host(cid, 2, (7, 8, 11), 3, pts) == ERR_ARG and "beyond" in err() and untouched()
    # null buffers
    assert host(cid, 2, None, 3, pts) == ERR_ARG and "null buffer" in err() and untouched()
    assert host(cid, 2, (0, 1, 3), 3, None) == ERR_ARG and "null buffer" in err() and untouched()
    assert host(cid, 2, (0, 1, 3), 3, pts, 0, None, fl) == ERR_ARG and "null buffer" in err() and untouched()
    assert host(cid, 2, (0, 1, 3), 3, pts, 0, out, None) == ERR_ARG and "null buffer" in err() and untouched()
    assert lib.eccx_point_sum_dev(ctx, cid, 2, None, 3, None, None, None, None, 0, None) == ERR_ARG and "null buffer" in err()
    # n == 0 returns ECCX_OK whatever the pointers are
    assert host(cid, 0, None, 0, None, 0, None, None) == 0 and untouched()
    assert lib.eccx_point_sum_dev(ctx, cid, 0, None, 0, None, None, None, None, EN.VALIDATE_POINTS, None) == 0
    # no members at all: every group is empty, and points may be NULL
    assert host(cid, 2, (9, 9, 9), 0, None) == 0 and (out.raw, fl.raw) == (bytes(2 * pb), b"\1\1")
    # a good call through the raw ABI, offsets[0] != 0
    assert host(cid, 2, (7, 8, 10), 3, pts) == 0
    assert split(out.raw, fl.raw, pb) == [c.expect([0]), c.expect([1, 2])]


def test_bls_aggregate(eng, case):
    """Engine.bls_aggregate: decompress, sum, compress -- groups of compressed points against the model's sums"""
    c = case
    if c.m.pb == 192:
        compress = G2.compress
    else:
        compress = lambda p: R1.point_compress_bytes(c.m.name, c.m.record(p)[0], bytes([c.m.record(p)[1]]))
    sizes = [1, 2, 0, 64, 65, 3]
    groups, at = [], 0
    for s in sizes:
        groups.append([(at + i) % NMULT for i in range(s)])
        at += s
    groups[5] = [0, 1, 12]  # aggregates to the point at infinity
    enc = b"".join(compress(c.pts[j]) for g in groups for j in g)
    got, flags = eng.bls_aggregate(enc, sizes, curve=c.m.name)
    eb = len(compress(c.pts[0]))
    want = [c.expect(g) for g in groups]
    assert flags == bytes(w[1] for w in want) and flags[2] == 1 and flags[5] == 1
    assert got == b"".join(compress(None if w[1] else _affine(c, w[0])) for w in want)
    # one member that does not decode rejects its group alone
    bad = bytearray(enc)
    bad[eb * 1] &= 0x7f  # the compression bit of the second group's first member
    got2, flags2 = eng.bls_aggregate(bytes(bad), sizes, curve=c.m.name)
    assert flags2 == bytes([flags[0], 2]) + flags[2:]
    assert got2[:eb] == got[:eb] and got2[2 * eb:] == got[2 * eb:]


def _affine(c, rec):
    if c.m.pb == 192:
        return G2.from_record(rec)
    return int.from_bytes(rec[:48], "big"), int.from_bytes(rec[48:], "big")
