"""Hand-built tapes and rows for the division subroutine's width-specialised variants (jit.cpp
op_div / div_routine, MH_JIT_STAGE=5), shared by tests/test_jit_div_width.py (host emulator) and
tests/test_gpu_jit_div_width.py (MI355X).

Columns x, y, w.  Every (divisor, dividend) shape comes, for each of udiv / urem / sdiv / srem /
smod, as a values tape `op(a, b)` and as a Bool tape `w < 2^255 and op(a, b) < K` behind the cheap
guard conjunct.  Divisors: low(y, 32 k) for k = 1..7, y & C160, the constants C32, C160, C224, and
two negative constants (-1, -C160) whose magnitudes the signed kinds divide by.  Dividends: x,
low(x, 160), low(x, 96).

Rows come in waves of 64 with a partial last wave.  A crafted lane is alone in its wave among
random lanes whose divisors fill their declared width, so no other lane's fallback recomputes it:
the wave is HOT when the crafted lane's divisor fills its width too (or is a constant, or the
shape is one limb wide), SHORT when its top declared limb is zero -- the wave the variant sends to
the legacy code."""
import random
from fractions import Fraction

from mythril_amd.tape import Op, TapeSet
from tests.div_cases import C32, C160, KILL, M, M32, OPS, PASS, neg

C224 = 0x9B05688C2B3E6C1F1F83D9ABFB41BD6B5BE0CD19137E2179510E527F
HOT, SHORT = "hot", "short"

# name -> (how, parameter): low(y, bits), y & mask, a pool constant
DIVISORS = {"y%d" % (32 * k): ("low", 32 * k) for k in range(1, 8)}
DIVISORS.update({"and160": ("and", C160), "c32": ("const", C32), "c160": ("const", C160),
                 "c224": ("const", C224), "cm1": ("const", M), "cn160": ("const", neg(C160))})
DIVIDENDS = {"x": 256, "x160": 160, "x96": 96}
DIGITS = (0, 1, 1 << 31, M32)


def limbs(v):
    return (max(v, 1).bit_length() + 31) // 32


def is_signed(div, dividend, op):
    """Whether the site keeps the signed kind: a dividend known non-negative over a divisor known
    non-negative is the unsigned kind."""
    how, p = DIVISORS[div]
    return op[0] == "s" and (dividend == "x" or (how == "const" and bool(p >> 255)))


def eff_y(div, yraw, signed=False):
    """The divisor the tape sees (its magnitude for a signed kind)."""
    how, p = DIVISORS[div]
    v = yraw & ((1 << p) - 1) if how == "low" else yraw & p if how == "and" else p
    return neg(v) if signed and v >> 255 else v


def declared_ny(div, signed):
    """Limbs of the divisor not known zero at the site, as op_div counts them."""
    how, p = DIVISORS[div]
    if how == "low":
        return p // 32
    if how == "and":
        return limbs(p)
    return limbs(neg(p) if signed and p >> 255 else p)


def variant(div, dividend, op):
    """True when the default level calls a variant for this shape: a called (path-0) site with
    ny <= 7 and nx >= ny (a full-width x keeps nx = 8 under a signed kind)."""
    how, p = DIVISORS[div]
    if op == "sdiv" and dividend == "x" and how == "const" and p >> 255:
        return False    # full-width operands: the small-quotient path, its cold side the legacy call
    nx = DIVIDENDS[dividend] // 32
    ny = declared_ny(div, is_signed(div, dividend, op))
    return ny <= 7 and nx >= ny


def build(divisors=None):
    """(tape set, {name: (tape index, divisor, dividend, op)}); names are
    "<dividend>_<divisor>_<op>_v" (values) and "..._b" (Bool)."""
    ts = TapeSet()
    b = ts.builder()
    x, y, w = b.var("x"), b.var("y"), b.var("w")
    guard = b.op(Op.BVULT, w, b.const(1 << 255, 256))
    c = lambda v: b.const(v, 256)

    def low(v, bits):
        return b.op(Op.ZEXT, b.op(Op.EXTRACT, v, imm0=bits - 1, imm1=0), imm0=256 - bits)

    idx = {}
    for dn in (divisors or DIVISORS):
        how, p = DIVISORS[dn]
        q = low(y, p) if how == "low" else b.op(Op.BVAND, y, c(p)) if how == "and" else c(p)
        for xn, bits in DIVIDENDS.items():
            a = x if bits == 256 else low(x, bits)
            for name, op in OPS:
                d = b.op(op, a, q)
                idx["%s_%s_%s_v" % (xn, dn, name)] = (len(ts.tapes), dn, xn, name)
                ts.add(b.finish(d))
                k = c(500) if name in ("udiv", "sdiv") else c(1 << 254)
                idx["%s_%s_%s_b" % (xn, dn, name)] = (len(ts.tapes), dn, xn, name)
                ts.add(b.finish(b.op(Op.AND, guard, b.op(Op.BVULT, d, k))))
    return ts, idx


def _raw_y(rng, div, yv):
    """A column value the shape reduces to yv (garbage in the bits it cuts)."""
    how, p = DIVISORS[div]
    g = rng.getrandbits(256)
    if how == "low":
        return yv | (g >> p << p)
    if how == "and":
        assert yv & ~p == 0
        return yv | (g & ~p & M)
    return g


def _full_y(rng, div):
    """A divisor of the shape whose top declared limb is nonzero."""
    how, p = DIVISORS[div]
    if how == "const":
        return p
    mask = p if how == "and" else (1 << p) - 1
    while True:
        v = rng.getrandbits(256) & mask
        if v >> (32 * (limbs(mask) - 1)):
            return v


def crafted(seed, div, dividend, signed):
    """[(label, x, y raw, short)]: the rows the variants' steps can go wrong on, for one shape.
    x = q y + r with r in {0, 1, y - 1} and each of the digits 0, 1, 2^31, 2^32 - 1 at every
    digit position the widths allow; x < y, x = y, x = 0, y = 1, y = 0; a divisor whose top
    declared limb is zero; for the signed kinds, dividends of both signs and -2^255."""
    rng = random.Random(seed)
    how, p = DIVISORS[div]
    full = DIVIDENDS[dividend]
    xmax = (1 << (full - (1 if signed and dividend == "x" else 0))) - 1
    ny = declared_ny(div, signed)
    out = []

    def put(label, xm, yv, short=False):
        assert 0 <= xm <= xmax or (signed and xm == 1 << 255), label
        if signed and dividend == "x" and len(out) % 2:
            xm = neg(xm)                      # both signs of x
        xr = xm | (rng.getrandbits(256) >> full << full)
        out.append((label, xr & M, _raw_y(rng, div, yv) & M, short))

    ys = [_full_y(rng, div)]
    if how == "low":
        ys += [(1 << p) - 1, 1 << (p - 32), (1 << (p - 32)) + 1]
    elif how == "and":
        top = p >> 128
        ys += [p, (top & -top) << 128]
    n = 0
    for j in range(limbs(xmax // min(eff_y(div, v, signed) for v in ys))):
        for d in DIGITS:    # the divisors and the remainders take turns
            for turn in range(len(ys)):   # the first divisor that leaves the digit room
                yv = ys[(n + n // 4 + turn) % len(ys)]
                ym = eff_y(div, yv, signed)
                qmax = xmax // ym
                q = rng.randrange(qmax + 1)
                q = (q & ~(M32 << (32 * j))) | (d << (32 * j))
                if q > qmax:
                    q &= (1 << (32 * (j + 1))) - 1   # the digit on top
                if q >> (32 * (j + 1)) == 0 and (q | 1 << (32 * (j + 1))) <= qmax:
                    q |= 1 << (32 * (j + 1))         # ... or under a digit, so that a 0 counts
                r = (0, 1, ym - 1)[n % 3]
                if q * ym + r > xmax:
                    r = 0
                if q * ym + r <= xmax and (d or q >> (32 * (j + 1))):
                    put("digit %d = %#x" % (j, d), q * ym + r, yv)
                    break
            n += 1
    # the estimate reaches the 2^32 clamp: digit 2^32 - 1 with everything below it at its maximum
    for yv in ys:
        ym = eff_y(div, yv, signed)
        for j in sorted({0, limbs(xmax // ym) - 2}):
            if j >= 0 and (ym << (32 * (j + 1))) - 1 <= xmax:
                put("clamp at %d" % j, (ym << (32 * (j + 1))) - 1, yv)
    for yv in ys[:2]:
        ym = eff_y(div, yv, signed)
        put("x < y", min(ym - 1, xmax), yv)
        if ym <= xmax:
            put("x = y", ym, yv)
        put("x = 0", 0, yv)
    if how != "const":
        put("y = 1", rng.randrange(xmax + 1), 1, short=ny > 1)
        put("y = 0", rng.randrange(xmax + 1), 0, short=ny > 1)
        if ny > 1:
            yv = rng.getrandbits(32 * (ny - 1)) & (p if how == "and" else M) | 1
            put("short divisor", rng.randrange(xmax + 1), yv, short=True)
    if signed and dividend == "x":
        out.append(("-2^255", 1 << 255, _raw_y(rng, div, ys[0]) & M, False))
    return out


def waves(seed, div, dividend, signed):
    """[(kind, 64 rows, crafted lane or None, label)]: a wave of random lanes, then one wave per
    crafted row with that row alone in it."""
    rng = random.Random(seed ^ 0x5EED)

    def filler():
        xr = rng.getrandbits(256)
        if signed and dividend == "x" and rng.random() < 0.5:
            xr = neg(xr >> 1)
        return [xr, _raw_y(rng, div, _full_y(rng, div)) & M, KILL if rng.random() < 0.125 else PASS]

    out = [(HOT, [filler() for _ in range(64)], None, "random")]
    for i, (label, xr, yr, short) in enumerate(crafted(seed, div, dividend, signed)):
        rows = [filler() for _ in range(64)]
        lane = (17 * i + 3) % 64
        rows[lane] = [xr, yr, PASS]
        out.append((SHORT if short else HOT, rows, lane, label))
    return out


def flatten(ws, last=37):
    """(rows, kinds): the waves in order, then the first one again cut to a partial wave."""
    ws = list(ws) + [(HOT, ws[0][1][:last], None, "partial")]
    return [r for w in ws for r in w[1]], [w[0] for w in ws]


def digit_facts(xm, ym, ny):
    """What the long division of xm by ym (magnitudes, ym >= 2^(32 (ny - 1))) meets: the set of
    (position, digit), whether an estimate reaches the 2^32 clamp, and whether a remainder has
    limb j + ny nonzero before step j."""
    digits, clamp, borrow_limb = set(), False, False
    r = xm
    for j in range(limbs(max(xm // ym, 1)) - 1, -1, -1):
        yj = ym << (32 * j)
        if r >> (32 * (j + ny)):
            borrow_limb = True
        d = r // yj
        assert d <= M32
        if float(Fraction(r, yj)) >= 2.0 ** 32:
            clamp = True
        digits.add((j, d))
        r -= d * yj
    return digits, clamp, borrow_limb


def gpu_rows(per_shape=14):
    """A few hundred rows for the whole tape set: per divisor shape crafted lanes of the
    full-width dividend (unsigned and signed, the short divisors among them), packed; then
    random rows.  The last wave is partial."""
    rng = random.Random(77)
    rows = []
    for i, div in enumerate(DIVISORS):
        for signed in (False, True):
            cr = crafted(100 + i, div, "x", signed)
            rng.shuffle(cr)
            keep = [c for c in cr if c[3]][:2] + [c for c in cr if not c[3]]
            rows += [[c[1], c[2], PASS] for c in keep[:per_shape]]
    while len(rows) % 64 != 41:
        rows.append([rng.getrandbits(rng.choice([256, 160, 96])), rng.getrandbits(256),
                     KILL if len(rows) % 7 == 0 else PASS])
    return rows
