"""Hand-built division tapes and rows for the tape JIT's inline division paths (jit.cpp op_div,
MH_JIT_DIV), shared by tests/test_jit_div_inline.py (host emulator) and
tests/test_gpu_jit_div_inline.py (MI355X).

Columns x, y, w.  Every operand shape comes, for each of udiv / urem / sdiv / srem / smod, as a
values tape `op(a, b)` and as a Bool tape `w < 2^255 and op(a, b) < K`: the guard is the cheap
first conjunct, so w = 2^256 - 1 makes a lane dead before the division runs.  SHAPES gives, per
shape, which inline path the default level takes for each op (0: the call, 1: short dividend,
3: small quotient, "fold": no code at all).

Rows come in waves of 64 (the last wave of a set is partial).  A wave is HOT when every live lane
is decided by the inline path, COLD when one lane -- alone in its wave -- is not, and DEAD when
that one lane is killed by the guard (hot for the Bool tape, cold for the values tape)."""
import random

from mythril_amd.tape import Op, TapeSet

M = (1 << 256) - 1
M32 = 0xFFFFFFFF
PASS, KILL = 0, M
HOT, COLD, DEAD = "hot", "cold", "dead"

OPS = (("udiv", Op.BVUDIV), ("urem", Op.BVUREM), ("sdiv", Op.BVSDIV), ("srem", Op.BVSREM),
       ("smod", Op.BVSMOD))
C32 = 0x9E3779B9
C160 = 0xC2B2AE3D27D4EB4F165667B19E3779B97F4A7C15
CFULL = 0x1F83D9ABFB41BD6B5BE0CD19137E2179510E527FADE682D19B05688C2B3E6C1F  # top limb < 2^31

# shape -> path per op at the default level (the short-divisor long division is not built: the
# shapes that would select it call the subroutine at every level)
_P1 = dict(udiv=1, urem=1, sdiv=1, srem=1, smod=0)
_CALL = dict(udiv=0, urem=0, sdiv=0, srem=0, smod=0)
SHAPES = {
    "var_var": dict(udiv=3, urem=0, sdiv=3, srem=0, smod=0),
    "c32_var": _P1,
    "x160_var": _P1,
    "x160_cfull": dict(udiv="fold", urem="fold", sdiv="fold", srem="fold", smod="fold"),
    "var_c160": _CALL,
    "var_y160": _CALL,
    "var_and160": _CALL,
    "var_y128": _CALL,
    "x160_y32": _CALL,
    "var_c32": _CALL,
    "var_y8": _CALL,
    # the estimate of x / x is 1 to a rounding: never clear of an integer, the call always runs
    "x_x": _CALL,
}


def build():
    """(tape set, {name: (tape index, [path of each division site])}); names are
    "<shape>_<op>_v" (values) and "<shape>_<op>_b" (Bool), plus the two-division tapes."""
    ts = TapeSet()
    b = ts.builder()
    x, y, w = b.var("x"), b.var("y"), b.var("w")
    guard = b.op(Op.BVULT, w, b.const(1 << 255, 256))
    c = lambda v: b.const(v, 256)

    def low(v, bits):
        return b.op(Op.ZEXT, b.op(Op.EXTRACT, v, imm0=bits - 1, imm1=0), imm0=256 - bits)

    operands = {
        "var_var": (x, y),
        "c32_var": (c(C32), y),
        "x160_var": (low(x, 160), y),
        "x160_cfull": (low(x, 160), c(CFULL)),
        "var_c160": (x, c(C160)),
        "var_y160": (x, low(y, 160)),
        "var_and160": (x, b.op(Op.BVAND, y, c(C160))),
        "var_y128": (x, low(y, 128)),
        "x160_y32": (low(x, 160), low(y, 32)),
        "var_c32": (x, c(C32)),
        "var_y8": (x, low(y, 8)),
        "x_x": (x, x),
    }
    idx = {}

    def add(name, root, paths):
        idx[name] = (len(ts.tapes), paths)
        ts.add(b.finish(root))

    for shape, (p, q) in operands.items():
        for name, op in OPS:
            d = b.op(op, p, q)
            path = [SHAPES[shape][name]]
            add("%s_%s_v" % (shape, name), d, path)
            k = c(500) if name in ("udiv", "sdiv") else c(1 << 254)
            add("%s_%s_b" % (shape, name), b.op(Op.AND, guard, b.op(Op.BVULT, d, k)), path)
    # two divisions sharing an operand, one inline and one called: a result waiting in the
    # subroutine's registers survives the next site
    add("two_p1_call_v", b.op(Op.BVXOR, b.op(Op.BVUDIV, low(x, 160), y), b.op(Op.BVUREM, x, y)),
        [1, 0])
    add("two_p3_call_v", b.op(Op.BVXOR, b.op(Op.BVUDIV, x, y), b.op(Op.BVUREM, x, y)), [3, 0])
    add("two_call_p3_v", b.op(Op.BVADD, b.op(Op.BVSREM, x, y), b.op(Op.BVSDIV, x, y)), [0, 3])
    add("two_p1_p3_b", b.op(Op.AND, guard, b.op(Op.BVULT, b.op(Op.BVUREM, c(C32), y),
                                                 b.op(Op.BVUDIV, x, y))), [1, 3])
    # only the low limb of the quotient is demanded
    add("lowlimb_udiv_v", b.op(Op.BVAND, b.op(Op.BVUDIV, x, y), c(M32)), [3])
    add("lowlimb_sdiv_v", b.op(Op.BVAND, b.op(Op.BVSDIV, x, y), c(M32)), [3])
    return ts, idx


def neg(v):
    return (-v) & M


def _full_y(rng):
    """A divisor whose top limb, and the top limb of its complement, are far from zero."""
    return (rng.randrange(0x00010000, 0x7FFF0000) << 224) | rng.getrandbits(224)


def _mid(rng, yv, q):
    """x = q y + r with r / y in [0.25, 0.75]: the estimate's fraction is far from an integer."""
    return q * yv + yv // 4 + rng.randrange(yv // 2)


def path1_waves(seed, signed):
    """[(kind, 64 rows[, crafted lane])] for a short dividend over a full-width column y: the divisor's top limb
    is nonzero in hot waves (for the signed kinds also not 2^32 - 1, whose complement's top limb
    is zero); a cold wave has one lane with y < 2^224, y = 0, or (signed) y >= -2^224."""
    rng = random.Random(seed)

    def hot_row():
        yv = _full_y(rng)
        if signed and rng.random() < 0.5:
            yv = neg(yv)
        return [rng.getrandbits(256), yv, PASS]

    waves = [(HOT, [hot_row() for _ in range(64)])]
    edge = [hot_row() for _ in range(64)]
    edge[0][1] = 1 << 224                     # the smallest divisor with a nonzero top limb
    edge[1][1] = M32 << 224 if not signed else (0x7FFFFFFF << 224) | 5
    edge[2][1] = (1 << 255) if signed else M  # -2^255: its complement's top limb is 2^31 - 1
    edge[3][0] = M                            # x's low bits all ones
    edge[4][0] = 0
    edge[5][1] = neg((1 << 224) + 1) if signed else (1 << 224) + 1
    waves.append((HOT, edge))
    bad = [(1 << 224) - 1, 0, 1, rng.getrandbits(100)]
    if signed:
        bad += [M, neg(1 << 224), neg(rng.getrandbits(200) + 1)]   # y7 = 2^32 - 1
    for i, yv in enumerate(bad):
        for kind in (COLD, DEAD):
            rows = [hot_row() for _ in range(64)]
            lane = (11 * i + 5) % 64
            rows[lane][1] = yv
            rows[lane][2] = KILL if kind == DEAD else PASS
            waves.append((kind, rows, lane))
    return waves


def path3_waves(seed, signed):
    """[(kind, 64 rows[, crafted lane])] for udiv / sdiv of two full-width columns: hot waves keep every lane's
    quotient below 2^10 with the estimate's fraction clear of an integer, or x < y with the
    fraction clear of 1; a cold wave has one lane that is not (see the labels below)."""
    rng = random.Random(seed)

    def signs(xv, yv):
        if signed:
            s = rng.randrange(4)
            return (neg(xv) if s & 1 else xv), (neg(yv) if s & 2 else yv)
        return xv, yv

    def hot_row(q=None):
        yv = _full_y(rng) >> (rng.choice([0, 0, 3, 9]) if q is None else 10)
        yv |= 1 << 224
        if q is None:
            q = rng.choice([0, 0, 1, 2, 5, rng.randrange(1 << rng.randrange(1, 7))])
        xv = _mid(rng, yv, q)
        while xv >> (255 if signed else 256):
            q //= 2
            xv = _mid(rng, yv, q)
        xv, yv = signs(xv, yv)
        return [xv, yv, PASS]

    waves = [(HOT, [hot_row() for _ in range(64)])]
    # quotients up to 1023, x far below y, and fractions just inside the band on both sides: the
    # band is thr = (e + 1) 2^-20 around every integer and the estimate is within 0.6 thr of the
    # true ratio (jit.cpp div_small_quotient), so a true fraction of 2 thr is decided and one of
    # 0.3 thr is not
    edge = [hot_row() for _ in range(64)]
    for i, q in enumerate((1023, 1023, 1000, 512, 1, 3, 100)):
        yv = (rng.randrange(0x00000400, 0x001F0000) << 224) | rng.getrandbits(224)
        r_in = (yv * 2 * (q + 2)) >> 20
        xv = q * yv + (r_in if i % 2 == 0 else yv - r_in)
        edge[i][0], edge[i][1] = signs(xv, yv)
    edge[10][0], edge[10][1] = signs(0, _full_y(rng))
    edge[11][0], edge[11][1] = signs(12345, _full_y(rng))         # x7 = x6 = 0: e = 0
    yv = _full_y(rng)
    edge[12][0], edge[12][1] = signs(yv >> 40, yv)                # e = 2^-40
    waves.append((HOT, edge))
    if signed:
        # the six low limbs of a negative operand all zero: the complement's window is one short
        # of |v|'s, a 2^-32 relative move
        lowz = [hot_row() for _ in range(64)]
        for i in range(0, 64, 2):
            wy = rng.randrange(1 << 40, 1 << 54)
            q = rng.randrange(1, 200)
            wx = q * wy + wy // 2
            lowz[i][0], lowz[i][1] = neg(wx << 192), neg(wy << 192) if i % 4 else wy << 192
        waves.append((HOT, lowz))
    yv = _full_y(rng) >> 11 | (1 << 224)
    thr_out = lambda q: (yv * 3 * (q + 1)) // (10 << 20)          # 0.3 thr
    cold = [
        ("k y", 7 * yv, yv), ("k y - 1", 7 * yv - 1, yv), ("k y + y - 1", 8 * yv - 1, yv),
        ("y - 1", yv - 1, yv), ("x = y", yv, yv),
        ("q = 1024", 1024 * yv + yv // 2, yv), ("q = 1023, fraction 1", 1024 * yv - 1, yv),
        ("just outside, low", 37 * yv + thr_out(37), yv),
        ("just outside, high", 38 * yv - thr_out(37), yv),
        ("y7 = 0", rng.getrandbits(250), (1 << 224) - 1), ("y = 0", rng.getrandbits(250), 0),
        ("y = 1", rng.getrandbits(250), 1),
    ]
    if signed:
        cold += [("-2^255 / -1", 1 << 255, M), ("-2^255 / 1", 1 << 255, 1),
                 ("y = -2^224", 5 << 230, neg(1 << 224)),
                 ("-k y", neg(9 * yv), yv), ("k y / -y", 9 * yv, neg(yv))]
    for i, (_, xv, yv_) in enumerate(cold):
        for kind in (COLD, DEAD):
            rows = [hot_row() for _ in range(64)]
            lane = (13 * i + 3) % 64
            rows[lane] = [xv & M, yv_ & M, KILL if kind == DEAD else PASS]
            waves.append((kind, rows, lane))
    return waves


def general_rows(seed, n=229):
    """Rows for every shape, called or inline: digits on integer boundaries for divisors of
    every width the shapes produce (x = k y - 1, k y, k y + y - 1 with k at each digit position),
    zero and all-ones operands, the signed corners."""
    rng = random.Random(seed)
    rows = []
    for wy in (8, 32, 128, 160, 200, 256):
        for _ in range(6):
            yv = rng.getrandbits(wy) | 1 << (wy - 1)
            kbits = rng.choice([1, 10, 32, 33, 64, 96, 128, 160])
            k = rng.getrandbits(max(1, min(kbits, 256 - wy))) | 1
            for xv in (k * yv - 1, k * yv, k * yv + yv - 1):
                if xv <= M:
                    rows.append([xv, yv | (rng.getrandbits(256) << wy & M), PASS])
    for xv in (0, 1, M, 1 << 255, (1 << 255) - 1, neg(5)):
        for yv in (0, 1, M, 1 << 255, 3, neg(3)):
            rows.append([xv, yv, PASS])
    while len(rows) < n:
        rows.append([rng.getrandbits(rng.choice([256, 256, 160, 64])),
                     rng.getrandbits(rng.choice([256, 256, 200, 33])),
                     KILL if len(rows) % 5 == 0 else PASS])
    return rows[:n]


def flatten(waves, last=37):
    """(rows, kinds): the waves in order, then the first (hot) wave again cut to `last` rows, a
    partial wave."""
    waves = list(waves)
    assert waves[0][0] == HOT
    waves.append((HOT, waves[0][1][:last]))
    rows = [r for w in waves for r in w[1]]
    return rows, [w[0] for w in waves]


def gpu_rows():
    """A few hundred rows that take every path, unsigned and signed: per path a hot wave, the
    wave of edge rows that stay hot, and the crafted lanes of the cold waves packed into waves
    of their own; then the general rows.  The last wave is partial."""
    rows = []
    for signed in (False, True):
        for waves in (path1_waves(3, signed), path3_waves(4, signed)):
            rows += waves[0][1] + waves[1][1]
            rows += [w[1][w[2]] for w in waves if w[0] == COLD]
            rows += waves[0][1][:64 - len(rows) % 64 if len(rows) % 64 else 0]
    rows += general_rows(5, 101)
    return rows
