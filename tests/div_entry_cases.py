"""Hand-built tapes and rows for the division subroutine's level-6 entries (jit.cpp op_div /
div_routine, MH_JIT_STAGE=6), shared by tests/test_jit_div_entry.py (host emulator) and
tests/test_gpu_jit_div_entry.py (MI355X).

Columns x, y, w, s.

Raw srem entry (layer A): `srem(x, y)` as a values tape, as the Bool tape
`w < 2^255 and srem(x, y) <s K`, with 1 to 7 limbs demanded (`srem(x, y) & mask`), and next to a
called urem (`srem(x, y) ^ urem(x, y)`).  One wave per crafted lane among random lanes that are
decided (HOT): the wave is HOT when the crafted lane is decided by a margin the estimate's error
cannot cross, COLD when it is undecided by such a margin, EDGE when it sits on a threshold (values
only).  The estimate e of |x| / |y| is within 0.71 thr of the quotient, thr = (e + 1) 2^-20
(div_small_quotient's proof), so a fraction of 4 thr or 1 - 4 thr is decided and one of 0.05 thr or
1 - 0.05 thr is not, whatever the roundings.

Run-time width dispatch (layer B): udiv / urem / sdiv / srem of x by `lshr(y, s)`, a divisor whose
width only the rows know (and sdiv / srem by its negation).  Waves: every lane at one ny in {2, 3, 5, 7} (DISPATCH: the wave enters
variant ny), with a short and a full x; one lane narrower, one lane wider, one lane y = 0 (LEGACY:
the dispatch leaves the wave to the legacy code)."""
import random

from mythril_amd.tape import Op, TapeSet
from tests.div_cases import KILL, M, PASS, neg

HOT, COLD, EDGE = "hot", "cold", "edge"
DISPATCH, LEGACY = "dispatch", "legacy"
K_SLT = 1 << 200
NYS = (2, 3, 5, 7)
B_OPS = (("udiv", Op.BVUDIV), ("urem", Op.BVUREM), ("sdiv", Op.BVSDIV), ("srem", Op.BVSREM))


def build():
    """(tape set, {name: tape index})."""
    ts = TapeSet()
    b = ts.builder()
    x, y, w, s = b.var("x"), b.var("y"), b.var("w"), b.var("s")
    guard = b.op(Op.BVULT, w, b.const(1 << 255, 256))
    idx = {}

    def add(name, root):
        idx[name] = len(ts.tapes)
        ts.add(b.finish(root))

    r = b.op(Op.BVSREM, x, y)
    add("srem_v", r)
    add("srem_b", b.op(Op.AND, guard, b.op(Op.BVSLT, r, b.const(K_SLT, 256))))
    add("srem_low_v", b.op(Op.BVAND, r, b.const(0xFFFFFFFF, 256)))
    for bits in (64, 96, 128, 160, 192, 224):   # top demanded limb 1..6: the hot chain's other exits
        add("srem_%d_v" % bits, b.op(Op.BVAND, r, b.const((1 << bits) - 1, 256)))
    add("srem_urem_v", b.op(Op.BVXOR, r, b.op(Op.BVUREM, x, y)))
    ys = b.op(Op.BVLSHR, y, s)
    for name, op in B_OPS:
        add("w_%s_v" % name, b.op(op, x, ys))
    yn = b.op(Op.BVSUB, b.const(0, 256), ys)   # a negative divisor of short magnitude
    add("wn_sdiv_v", b.op(Op.BVSDIV, x, yn))
    add("wn_srem_v", b.op(Op.BVSREM, x, yn))
    add("w_urem_b", b.op(Op.AND, guard, b.op(Op.BVULT, b.op(Op.BVUREM, x, ys),
                                            b.const(1 << 60, 256))))
    return ts, idx


A_TAPES = ("srem_v", "srem_b", "srem_low_v", "srem_64_v", "srem_96_v", "srem_128_v", "srem_160_v",
           "srem_192_v", "srem_224_v", "srem_urem_v")
B_TAPES = tuple("w_%s_v" % n for n, _ in B_OPS) + ("wn_sdiv_v", "wn_srem_v", "w_urem_b")


# ---- layer A rows ---------------------------------------------------------------------------
def _signed(mag, negative):
    return neg(mag) if negative else mag


def _ymag(rng):
    """|y| with a nonzero top limb (of |y| and of |y| - 1) that leaves room for c < 2^10."""
    return rng.randrange(1 << 226, 1 << 244)


def _at(ym, c, num, den):
    """|x| = c |y| + |y| num / den (a fraction num / den of the way to the next multiple)."""
    return c * ym + ym * num // den


def _thr(c):
    """thr of a quotient in [c, c + 1), as (numerator, denominator)."""
    return (c + 1), 1 << 20


def hot_lane(rng):
    ym = _ymag(rng)
    c = rng.choice([0, 1, 2, 3, rng.randrange(1 << 10)])
    xm = _at(ym, c, rng.randrange(100, 900), 1000)
    return [_signed(xm, rng.random() < 0.5), _signed(ym, rng.random() < 0.5)]


def crafted_a(seed):
    """[(label, x, y, kind)] for the raw srem entry."""
    rng = random.Random(seed)
    out = []

    def put(label, x, y, kind):
        out.append((label, x & M, y & M, kind))

    for sx in (False, True):
        for sy in (False, True):
            ym = _ymag(rng)
            put("signs %d%d" % (sx, sy), _signed(_at(ym, 5, 1, 2), sx), _signed(ym, sy), HOT)
    put("x = -2^255, y = 1", 1 << 255, 1, COLD)
    put("x = -2^255, y = -1", 1 << 255, M, COLD)
    put("x = -2^255, y = -2^255", 1 << 255, 1 << 255, COLD)
    for sx in (False, True):
        ym = _ymag(rng)
        put("|x| < |y|", _signed(ym - 1 - rng.randrange(ym >> 3), sx), _signed(ym, not sx), HOT)
        put("x tiny", _signed(5, sx), _signed(ym, sx), HOT)
        put("c = 1", _signed(_at(ym, 1, 1, 2), sx), _signed(ym, not sx), HOT)
        put("c = 2^10 - 1", _signed(_at(ym, 1023, 1, 2), sx), _signed(ym, sx), HOT)
        put("c = 2^10", _signed(_at(ym, 1024, 1, 2), sx), _signed(ym, sx), COLD)
        yl = rng.randrange(1 << 226, 1 << 240)   # room for the larger quotient
        put("c = 5000", _signed(_at(yl, 5000, 1, 2), sx), _signed(yl, not sx), COLD)
        for k in (1, 2, 77, 1023):
            put("x = %d y" % k, _signed(k * ym, sx), _signed(ym, sx ^ (k & 1 == 0)), COLD)
        put("x = 0", 0, _signed(ym, sx), HOT)
        for c in (1, 40, 1000):
            tn, td = _thr(c)
            for label, num, den, kind in (
                    ("0.05 thr above", tn, 20 * td, COLD), ("4 thr above", 4 * tn, td, HOT),
                    ("thr above", tn, td, EDGE), ("0.05 thr below", td * 20 - tn, 20 * td, COLD),
                    ("4 thr below", td - 4 * tn, td, HOT), ("thr below", td - tn, td, EDGE)):
                put("c = %d, %s" % (c, label), _signed(_at(ym, c, num, den), sx),
                    _signed(ym, rng.random() < 0.5), kind)
        # top limb of y ^ sy zero; y = 0
        ys = rng.getrandbits(224) | 1
        put("short y", _signed(rng.getrandbits(255), sx), _signed(ys, sx), COLD)
        put("|y| = 2^224 (y ^ sy is short when y is negative)",
            _signed(rng.getrandbits(255), not sx), _signed(1 << 224, sx), COLD)
        put("y = 0", _signed(rng.getrandbits(255), sx), 0, COLD)
        # the borrow runs through every limb: y's low limbs all ones, x's zero below the top
        put("borrow through", _signed(0x7A000000 << 224, sx), _signed((1 << 250) - 1, not sx), HOT)
        put("borrow through, same signs", _signed(0x7A000000 << 224, sx),
            _signed((1 << 250) - 1, sx), HOT)
        # m != 0 with P = 0
        put("m != 0, P = 0", _signed(5 + rng.getrandbits(100), sx), _signed(_ymag(rng), not sx), HOT)
    return out


def waves_a(seed):
    """[(kind, 64 rows [x, y, w, s], crafted lane or None, label)]."""
    rng = random.Random(seed ^ 0xA11)

    def filler():
        return hot_lane(rng) + [KILL if rng.random() < 0.125 else PASS, 0]

    out = [(HOT, [filler() for _ in range(64)], None, "random")]
    for i, (label, x, y, kind) in enumerate(crafted_a(seed)):
        rows = [filler() for _ in range(64)]
        lane = (17 * i + 3) % 64
        rows[lane] = [x, y, PASS, 0]
        out.append((kind, rows, lane, label))
    return out


# ---- layer B rows ---------------------------------------------------------------------------
def _b_lane(rng, ny, x_bits):
    """x of x_bits bits over a divisor lshr(y, s) whose limb ny - 1 is its top nonzero limb."""
    y = rng.getrandbits(256) | 1 << 255
    s = 32 * (8 - ny) + rng.randrange(16)
    x = rng.getrandbits(x_bits) | 1 << (x_bits - 1)
    if x_bits == 255 and rng.random() < 0.5:
        x = neg(x)   # a full-width dividend of either sign (its magnitude is as wide)
    return [x, y, KILL if rng.random() < 0.125 else PASS, s]


def waves_b(seed):
    """[(kind, 64 rows, ny of the wave, label)]: x is positive wherever it is short, so the signed
    kinds see the same widths; a full-width x has either sign, and the wn_ tapes negate the
    divisor, so the signed tails run after a dispatched variant with negative operands."""
    rng = random.Random(seed ^ 0xB22)
    out = []
    for ny in NYS:
        for label, xb in (("x full", 255), ("x short", 32 * ny + 48)):
            xb = min(xb, 255)
            out.append((DISPATCH, [_b_lane(rng, ny, xb) for _ in range(64)], ny,
                        "ny = %d, %s" % (ny, label)))
        for label, fix in (("one lane narrower", lambda r: r.__setitem__(3, r[3] + 32 + 5)),
                           ("one lane wider", lambda r: r.__setitem__(3, r[3] - 32)),
                           ("one lane y = 0", lambda r: r.__setitem__(1, 0))):
            rows = [_b_lane(rng, ny, 255) for _ in range(64)]
            r = rows[(7 * ny + 11) % 32]   # inside the partial copy of the wave (flatten)
            fix(r)
            r[2] = PASS
            out.append((LEGACY, rows, ny, "ny = %d, %s" % (ny, label)))
    # a per-lane mix of widths, one-limb and zero divisors among them
    rows = []
    for _ in range(64):
        r = _b_lane(rng, rng.choice((1, 2, 3, 4, 5, 6, 7, 8)), rng.choice((64, 160, 255)))
        if rng.random() < 0.1:
            r[3] = 256 + rng.randrange(64)   # shifted out: y = 0
        rows.append(r)
    out.append((LEGACY, rows, 0, "mixed widths"))
    return out


def flatten(ws, last=37):
    """(rows, kinds): the waves in order, then the first one again cut to a partial wave."""
    ws = list(ws) + [(ws[0][0], ws[0][1][:last], ws[0][2], "partial")]
    return [r for w in ws for r in w[1]], [w[0] for w in ws]


def gpu_rows():
    """A few hundred rows for the whole tape set: the crafted layer-A lanes packed among decided
    ones, the layer-B waves of ny = 3 and 5 and the mixed wave; the last wave is partial."""
    rng = random.Random(99)
    rows = []
    for label, x, y, kind in crafted_a(5):
        rows.append([x, y, PASS, 0])
        rows.append(hot_lane(rng) + [KILL if len(rows) % 7 == 0 else PASS, 0])
    while len(rows) % 64:
        rows.append(hot_lane(rng) + [PASS, 0])
    rows += [hot_lane(rng) + [PASS, 0] for _ in range(64)]   # one hot wave
    for w in waves_b(6):
        if w[2] in (0, 3, 5):
            rows += w[1]
    rows += waves_b(6)[0][1][:41]
    return rows
