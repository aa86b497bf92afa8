"""Python model of the saturated field layer (eccoxide_amd/csrc/fe.hpp) for the eight field classes of
curve_consts.inc: the moduli and their derived constants, expected values in plain int arithmetic, limb-faithful
CLASSIFIERS of the three reductions (which only say which branch a row takes, never what it should give), and the
generators of the rows tests/test_sat_layer_cpu.py counts and tests/test_sat_layer_gpu.py runs.  No GPU, no library
under test."""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTS = os.path.join(ROOT, "eccoxide_amd", "csrc", "curve_consts.inc")
M32 = (1 << 32) - 1


class Field:
    """One class of curve_consts.inc.  kind: 'mont' (word-by-word Montgomery, R = 2^(32 L)), 'mersenne' and 'pm19'
    (plain representation, fold reductions), 'none' (CURVE448: no product on the saturated layer)."""

    def __init__(self, idx, name, p, L, FB, be, kind, consts):
        self.idx, self.name, self.p, self.L, self.FB, self.be, self.kind = idx, name, p, L, FB, be, kind
        self.consts = consts                       # the constants fe_mul_k is called with, besides R2 and ONE
        self.R = 1 << (32 * L)                     # what a limb array can hold
        self.Rw = self.R if kind == "mont" else 1  # the factor of the working form
        self.Rinv = pow(self.Rw, -1, p)
        self.ONE = self.Rw % p
        self.R2 = self.Rw * self.Rw % p
        self.N0 = (-pow(p, -1, 1 << 32)) & M32
        self.PP1 = p + 1
        self.has_product = kind != "none"

    def __repr__(self):
        return self.name

    # ---- expected values: plain integers only ----
    def add(self, a, b):
        return (a + b) % self.p

    def sub(self, a, b):
        return (a - b) % self.p

    def neg(self, a):
        return -a % self.p

    def mul(self, a, b):
        return a * b * self.Rinv % self.p

    def to_mont(self, raw):
        return raw * self.Rw % self.p

    def from_mont(self, a):
        return a * self.Rinv % self.p

    def inv(self, a):
        """fe_inv_fast in the working form: (a / Rw)^-1 Rw; 0 gives 0."""
        if a % self.p == 0:
            return 0
        return pow(a * self.Rinv, -1, self.p) * self.Rw % self.p

    # ---- limbs ----
    def pack(self, vals):
        return b"".join(v.to_bytes(4 * self.L, "little") for v in vals)

    def unpack(self, raw):
        w = 4 * self.L
        return [int.from_bytes(raw[i:i + w], "little") for i in range(0, len(raw), w)]


FIELDS = [
    Field(0, "P256", 2**256 - 2**224 + 2**192 + 2**96 - 1, 8, 32, True, "mont", ("B", "B3")),
    Field(1, "P384", 2**384 - 2**128 - 2**96 + 2**32 - 1, 12, 48, True, "mont", ("B", "B3")),
    Field(2, "P521", 2**521 - 1, 17, 66, True, "mersenne", ("B", "B3")),
    Field(3, "BLS12_381", 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab,
          12, 48, True, "mont", ("B", "B3")),
    Field(4, "ED25519", 2**255 - 19, 8, 32, False, "pm19", ("D2",)),
    Field(5, "P256K1", 2**256 - 2**32 - 977, 8, 32, True, "mont", ("B", "B3")),
    Field(6, "CURVE448", 2**448 - 2**224 - 1, 14, 56, False, "none", ()),
    Field(7, "JUBJUB", 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001, 8, 32, True, "mont", ("D2",)),
]
BY_NAME = {f.name: f for f in FIELDS}
NAMES = [f.name for f in FIELDS]
PRODUCT_NAMES = [f.name for f in FIELDS if f.has_product]


def parse_consts(name):
    """The digits of struct `name` in curve_consts.inc: scalars and limb arrays as integers."""
    with open(CONSTS) as fh:
        txt = fh.read()
    body = txt[txt.index("struct %s {" % name):]
    body = body[: body.index("\n};")]
    out = {}
    for key in ("L", "FB", "MERSENNE", "PM19", "PBITS"):
        out[key] = int(re.search(r"int %s = (\d+);" % key, body).group(1))
    out["N0"] = int(re.search(r"uint32_t N0 = (\w+?)u;", body).group(1), 16)
    out["IO_BE"] = re.search(r"bool IO_BE = true;", body) is not None
    for m in re.finditer(r"uint32_t (\w+)\[(\d+)\] = \{([^}]*)\}", body):
        vals = [int(v.strip().rstrip("u"), 16) for v in m.group(3).split(",")]
        assert len(vals) == int(m.group(2))
        out[m.group(1)] = sum(v << (32 * i) for i, v in enumerate(vals))
    return out


# ---- classifiers: the three reductions restated limb for limb.  They say which branch a row takes; no expected value
# ---- of any test comes from them.
def mont_t(f, a, b):
    """The value (carry : t) that fe_mul_impl hands to cond_sub_p: (a b + m p) / R with one reduction digit per word."""
    acc = a * b
    for i in range(f.L):
        m = (((acc >> (32 * i)) & M32) * f.N0) & M32
        acc += (m * f.p) << (32 * i)
    assert acc & (f.R - 1) == 0
    return acc >> (32 * f.L)


def pm19_fold(a, b):
    """fe_mul_pm19: (u, top) with u the value that enters cond_sub_p and top the folded carry word."""
    t = a * b
    lo, hi = t & (2**256 - 1), t >> 256
    acc = lo + 38 * hi
    c, u = acc >> 256, acc & (2**256 - 1)
    assert c < 2**31
    top = ((c << 1) & M32) | (u >> 255)
    u &= 2**255 - 1
    u += (top * 19) & M32
    assert u < 2**256
    return u, top


def mersenne_fold(f, a, b):
    """fe_mul_mersenne: (s, top) with s the value that enters cond_sub_p and top the bit the second fold adds back."""
    k = f.p.bit_length()
    t = a * b
    assert t < 1 << (64 * f.L)
    s = (t & f.p) + ((t >> k) & (f.R - 1))
    assert s < f.R
    top = s >> k
    s = (s & f.p) + top
    assert s < f.R
    return s, top


def entering(f, a, b):
    """The integer that enters the product's closing cond_sub_p."""
    if f.kind == "mont":
        return mont_t(f, a, b)
    if f.kind == "pm19":
        return pm19_fold(a, b)[0]
    return mersenne_fold(f, a, b)[0]


def band(f, t):
    """0: t < p (kept), 1: p <= t < R (decided by the borrow alone), 2: t >= R (decided by the carry word)."""
    return 0 if t < f.p else (1 if t < f.R else 2)


def top_reachable(f):
    """Whether a sum or a Montgomery t of canonical operands can reach R at all: only where 2p > R."""
    return 2 * f.p > f.R


# ---- square roots (Tonelli-Shanks; JUBJUB's p - 1 has 2-adicity 32) ----
def sqrt_mod(v, p):
    v %= p
    if v == 0:
        return 0
    if pow(v, (p - 1) // 2, p) != 1:
        return None
    q, s = p - 1, 0
    while q % 2 == 0:
        q //= 2
        s += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(v, q, p), pow(v, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % p
            i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    assert r * r % p == v
    return r


# ---- rows ----
def _dedup(vals, p):
    out, seen = [], set()
    for v in vals:
        if 0 <= v < p and v not in seen:
            seen.add(v)
            out.append(v)
    return out


def edge_values(f):
    """Canonical values at which a carry chain, a reduction digit or a fold is at an edge."""
    p, L, R = f.p, f.L, f.R
    vals = [0, 1, 2, 3, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2]
    vals += [R % p, R * R % p, -R % p, pow(R, -1, p)]
    for i in range(1, L):                                    # every 32-bit boundary
        vals += [1 << (32 * i), (1 << (32 * i)) - 1, p - (1 << (32 * i))]
    vals += [1 << (p.bit_length() - 1), (1 << (p.bit_length() - 1)) - 1]
    for i in range(1, L):                                    # p with the limbs below i cleared
        vals.append((p >> (32 * i)) << (32 * i))
    for i in range(L):                                       # p - 1 with a run of limbs flipped
        for run in sorted({1, 2, 3, L // 2}):
            if i + run <= L:
                vals.append((p - 1) ^ (((1 << (32 * run)) - 1) << (32 * i)))
    return _dedup(vals, p)


def noncanonical_values(f):
    """Raw values at or above p that an unchecked load (fe_load_* without fe_is_canonical) hands on, and the two
    all-ones patterns."""
    p, wire = f.p, 1 << (8 * f.FB)
    vals = [v for v in (p, p + 1, p + 18, p + 19, 2 * p, 2 * p + 1) if v < wire]
    vals += [wire - 1, f.R - 1]
    if f.name == "P521":
        vals += [k * p for k in (1, 2, 64, 127)] + [2**528 - 1]
    if f.name == "ED25519":
        vals += [p + j for j in range(20)] + [2**255 - 1, 2**255, 2**256 - 1]
    if f.name == "JUBJUB":
        vals += [2 * p, 2 * p + 1, 2**256 - 1]
    out = []
    for v in vals:
        assert p <= v < f.R
        if v not in out:
            out.append(v)
    return out


def interleave(edges, rnd):
    """Edge rows and random rows in one list, spread evenly so that they share wavefronts."""
    out, j = [], 0
    for i, e in enumerate(edges):
        out.append(e)
        while j < len(rnd) and (j + 1) * len(edges) <= (i + 1) * len(rnd):
            out.append(rnd[j])
            j += 1
    return out + list(rnd[j:])


def _odd_len(rows, filler):
    """No batch is a multiple of the workgroup (256): the last turn of the grid-stride loop is a partial one."""
    rows = list(rows)
    while len(rows) % 256 == 0 or len(rows) % 64 == 0:
        rows.append(filler)
    return rows


N_RANDOM = 2000
_cache = {}


def _memo(fn):
    def wrapped(f):
        key = (fn.__name__, f.name)
        if key not in _cache:
            _cache[key] = fn(f)
        return list(_cache[key])
    wrapped.__name__ = fn.__name__
    wrapped.__doc__ = fn.__doc__
    return wrapped


@_memo
def tiny_residue_pairs(f):
    """(a, r Rw / a): products whose residue r is below 64.  u or s then sits just above 0 or just above p (2^255 - 19:
    the closing subtraction fires; Montgomery: t = r or t = r + p, the band the borrow alone decides)."""
    rng = random.Random("tiny " + f.name)
    out = []
    for r in range(64):
        for _ in range(16):
            a = rng.randrange(1, f.p)
            out.append((a, r * f.Rw * pow(a, -1, f.p) % f.p))
    return out


@_memo
def pair_rows(f):
    """Rows of the binary arithmetic ops: the all-pairs product of the edge set, sums crafted to land in [p, p + 16),
    tiny-residue products (classes with a product), interleaved with 2000 random pairs."""
    rng = random.Random("pairs " + f.name)
    e = edge_values(f)
    edges = [(a, b) for a in e for b in e]
    for j in range(16):
        if f.p + j < f.R:
            for _ in range(4):
                a = rng.randrange(j + 1, f.p)
                edges.append((a, f.p + j - a))
    if f.has_product:
        edges += tiny_residue_pairs(f)
    rnd = [(rng.randrange(f.p), rng.randrange(f.p)) for _ in range(N_RANDOM)]
    return _odd_len(interleave(edges, rnd), (1, 2))


@_memo
def unary_rows(f):
    """Canonical rows of the unary ops (neg, from_mont, inv, mul_k): the edge set among 2000 random values."""
    rng = random.Random("unary " + f.name)
    return _odd_len(interleave(edge_values(f), [rng.randrange(f.p) for _ in range(N_RANDOM)]), 5)


@_memo
def sqr_rows(f):
    """fe_sqr's own rows: squares land differently from products, so the middle band is reached by construction: square
    roots a of r Rw for small r and for r up to R - p, so that a^2 / Rw = r (mod p) and the value entering cond_sub_p is r
    or r + p.  Both roots are kept; which band a row takes is for the classifier to say."""
    rng = random.Random("sqr " + f.name)
    targets = list(range(256))
    span = min(f.R - f.p, f.p)
    targets += [rng.randrange(span) for _ in range(256)]
    crafted = []
    for r in targets:
        a = sqrt_mod(r * f.Rw, f.p)
        if a is not None:
            crafted += [a, f.p - a] if a else [0]
    edges = edge_values(f) + _dedup(crafted, f.p)
    return _odd_len(interleave(edges, [rng.randrange(f.p) for _ in range(N_RANDOM)]), 7)


@_memo
def raw_rows(f):
    """Rows of the ops that take any value (fe_to_mont, fe_is_canonical, fe_is_zero, fe_eq, fe_all_zero): the canonical
    unary rows, the non-canonical values of an unchecked load, and random values below 2^(8 FB)."""
    rng = random.Random("raw " + f.name)
    extra = noncanonical_values(f) + [rng.getrandbits(8 * f.FB) for _ in range(200)]
    # values whose working form is tiny: fe_to_mont's t is then r + p, in the band the borrow alone decides, also where
    # R^2 mod p is so small (P384, P256K1) that no other row gets a t above p
    extra += [r * f.Rinv % f.p for r in range(1, 33)]
    return _odd_len(interleave(extra, unary_rows(f)), 9)


def constants(f):
    """name -> value of the constants fe_mul_k is tested with: R2 and ONE derived here, the curve's from the file."""
    if not f.has_product:
        return {}
    d = parse_consts(f.name)
    out = {"R2": f.R2, "ONE": f.ONE}
    for k in f.consts:
        out[k] = d[k]
    return out
