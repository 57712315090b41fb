"""Hand-built tapes and rows for the staged conjuncts of the tape JIT (jit.cpp emit_staged),
shared by tests/test_jit_staged.py (host emulator) and tests/test_gpu_jit_staged.py (MI355X).

Every tape is a root conjunction over the columns x, y, z, w whose first conjunct, `w < 2^255`,
is a guard the rows switch on and off (w = 0 passes, w = 2^256 - 1 kills the row); the conjunct
under test follows it.  Row sets are 64 rows, one wave."""
import random

from mythril_amd.tape import Op, TapeSet

M = (1 << 256) - 1
M32 = 0xFFFFFFFF
LOW = (1 << 224) - 1      # limbs 0..6
PASS, KILL = 0, M         # values of w for the guard


def top(t7: int, low: int = 0) -> int:
    """A 256-bit value with limb 7 = t7 and limbs 0..6 = low."""
    return ((t7 & M32) << 224) | (low & LOW)


def build():
    """(tape set, {name: tape index})."""
    ts = TapeSet()
    b = ts.builder()
    x, y, z, w = b.var("x"), b.var("y"), b.var("z"), b.var("w")
    guard = b.op(Op.BVULT, w, b.const(1 << 255, 256))
    idx = {}

    def add(name, conj, *more):
        root = b.op(Op.AND, guard, conj)
        for c in more:
            root = b.op(Op.AND, root, c)
        idx[name] = len(ts.tapes)
        ts.add(b.finish(root))

    k1 = b.const(0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95, 256)
    # == over a multiplication cone
    add("eq_mul", b.op(Op.EQ, b.op(Op.BVMUL, x, y), z))
    # ordered compares over a logic / constant-shift cone: A = (x ^ (y << 8)) | (y >> 252),
    # B = z & ~(y << 4); y = 0 gives A = x, B = z
    def logic_a():
        return b.op(Op.BVOR, b.op(Op.BVXOR, x, b.op(Op.BVSHL, y, b.const(8, 256))),
                    b.op(Op.BVLSHR, y, b.const(252, 256)))

    def logic_b():
        return b.op(Op.BVAND, z, b.op(Op.BVNOT, b.op(Op.BVSHL, y, b.const(4, 256))))

    for name, op in (("ult", Op.BVULT), ("ule", Op.BVULE), ("ugt", Op.BVUGT), ("uge", Op.BVUGE),
                     ("slt", Op.BVSLT), ("sle", Op.BVSLE), ("sgt", Op.BVSGT), ("sge", Op.BVSGE)):
        add("logic_" + name, b.op(op, logic_a(), logic_b()))
    # carry slack
    add("add_ult", b.op(Op.BVULT, b.op(Op.BVADD, x, y), z))
    add("sub_uge", b.op(Op.BVUGE, b.op(Op.BVSUB, x, y), z))
    add("add_slt", b.op(Op.BVSLT, b.op(Op.BVADD, x, y), z))
    add("chain3_ult", b.op(Op.BVULT, b.op(Op.BVADD, b.op(Op.BVSUB, b.op(Op.BVADD, x, y), k1), k1),
                           z))
    add("chain3_sge", b.op(Op.BVSGE, b.op(Op.BVSUB, b.op(Op.BVADD, b.op(Op.BVADD, x, y), k1), k1),
                           z))
    add("both_sides", b.op(Op.BVULE, b.op(Op.BVADD, x, y), b.op(Op.BVADD, z, b.const(0, 256))),
        b.op(Op.BVUGT, b.op(Op.BVADD, x, k1), b.op(Op.BVSUB, z, y)))
    add("ite_sums", b.op(Op.BVULT, b.op(Op.ITE, b.op(Op.EQ, b.op(Op.BVAND, x, b.const(1, 256)),
                                                    b.const(0, 256)),
                                        b.op(Op.BVADD, x, y), b.op(Op.BVSUB, x, y)), z))
    add("sum_and", b.op(Op.BVULT, b.op(Op.BVAND, b.op(Op.BVADD, x, y),
                                       b.const(M ^ (0xFF << 248), 256)), z))
    # a node (the product) used by the staged conjunct and by a later one
    prod = b.op(Op.BVMUL, x, y)
    shared = b.op(Op.BVADD, b.op(Op.BVXOR, b.op(Op.BVADD, prod, z), b.op(Op.BVSHL, z,
                                                                       b.const(40, 256))), x)
    add("shared", b.op(Op.EQ, shared, z), b.op(Op.BVULT, b.op(Op.BVXOR, prod, x), z))
    add("shared_ord", b.op(Op.BVULT, shared, z), b.op(Op.BVUGE, b.op(Op.BVXOR, prod, x), y))
    return ts, idx


def rows_eq_mul():
    """{case: 64 rows} for eq_mul: (a) no row with equal low limbs, (b) one row with equal low
    limbs and unequal high limbs, (c) one row equal in every limb, (d) the row with equal low
    limbs killed by the guard."""
    rng = random.Random(11)
    base = []
    for _ in range(64):
        xv, yv = rng.getrandbits(256), rng.getrandbits(256)
        p = (xv * yv) & M
        base.append([xv, yv, p ^ (1 + rng.getrandbits(31)) ^ (rng.getrandbits(200) << 32), PASS])
    out = {"a": [list(r) for r in base]}
    for case in "bcd":
        rows = [list(r) for r in base]
        xv, yv = rows[17][0], rows[17][1]
        p = (xv * yv) & M
        rows[17][2] = p if case == "c" else p ^ (1 << 200)
        rows[17][3] = KILL if case == "d" else PASS
        out[case] = rows
    return out


def rows_ordered():
    """64 rows for the logic_* tapes (y = 0: A = x, B = z, except the random tail): top limbs
    equal with the lower limbs deciding either way, equal operands, the signed boundary."""
    rng = random.Random(12)
    rows = []
    for t7 in (0, 1, 0x7FFFFFFF, 0x80000000, M32, 0x12345678):
        lo = rng.getrandbits(224)
        rows.append([top(t7, lo), 0, top(t7, lo + 1), PASS])   # lower limbs: A < B
        rows.append([top(t7, lo + 1), 0, top(t7, lo), PASS])   # A > B
        rows.append([top(t7, lo), 0, top(t7, lo), PASS])       # equal (< against <=)
        rows.append([top(t7, 1 << 200), 0, top(t7, 1), PASS])  # decided by limb 6
    for a7, b7 in ((0x7FFFFFFF, 0x80000000), (0x80000000, 0x7FFFFFFF), (0, M32), (M32, 0),
                   (0x7FFFFFFF, 0x7FFFFFFE), (0x80000000, 0x80000001)):
        rows.append([top(a7, rng.getrandbits(224)), 0, top(b7, rng.getrandbits(224)), PASS])
        rows.append([top(a7, 0), 0, top(b7, LOW), PASS])
    rows.append([top(5, 7), 0, top(5, 7), KILL])               # equal, but killed by the guard
    while len(rows) < 64:
        rows.append([rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(256), PASS])
    return rows


def rows_decided():
    """64 rows in which the top limbs of A and B differ (y = 0) -- no staged ordered compare of
    the logic_* tapes needs its fallback: the signed boundary and the ends of the range first."""
    rng = random.Random(13)
    rows = []
    for a7, b7 in ((0x7FFFFFFF, 0x80000000), (0x80000000, 0x7FFFFFFF), (0, M32), (M32, 0),
                   (0x7FFFFFFF, 0x7FFFFFFE), (0x80000000, 0x80000001), (0, 1), (M32, M32 - 1)):
        rows.append([top(a7, rng.getrandbits(224)), 0, top(b7, rng.getrandbits(224)), PASS])
        rows.append([top(a7, 0), 0, top(b7, LOW), PASS])
    while len(rows) < 64:
        a, c = rng.getrandbits(256), rng.getrandbits(256)
        if (a >> 224) != (c >> 224):
            rows.append([a, 0, c, PASS])
    return rows


def rows_carry(sub: bool):
    """64 rows for the carry-slack tapes: the top-limb sum (difference) of x and y lands exactly
    on z's top limb, 1..3 off either way, on 0xFFFFFFFF or 0 -- each with and without a carry
    (borrow) out of limb 6, z's lower limbs at both ends -- and far apart."""
    rng = random.Random(14 + sub)
    rows = []

    def xy(s7, carry):
        """x, y whose top limbs sum (x - y: differ) to s7 mod 2^32, lower limbs (not) carrying."""
        x7 = rng.getrandbits(32)
        y7 = (x7 - s7) & M32 if sub else (s7 - x7) & M32
        if sub:
            xl, yl = (0, LOW) if carry else (LOW, 0)       # borrow: x_low < y_low
        else:
            xl, yl = (LOW, 1) if carry else (5, 7)
        return top(x7, xl), top(y7, yl)

    for delta in (-3, -2, -1, 0, 1, 2, 3):
        for carry in (0, 1):
            for zl in (0, LOW):
                s7 = rng.getrandbits(32) | 0x100
                xv, yv = xy(s7, carry)
                rows.append([xv, yv, top(s7 + delta, zl), PASS])
    for s7 in (M32, 0):
        for carry in (0, 1):
            for z7 in (0, M32, 1, 0x80000000):
                xv, yv = xy(s7, carry)
                rows.append([xv, yv, top(z7, rng.getrandbits(224)), PASS])
    for s7, z7 in ((0x7FFFFFFF, 0x80000000), (0x80000000, 0x7FFFFFFF), (0x7FFFFFFF, 0x7FFFFFFF),
                   (0x80000000, 0x80000000)):
        for carry in (0, 1):
            xv, yv = xy(s7, carry)
            rows.append([xv, yv, top(z7, 1 << 100), PASS])
    xv, yv = xy(77, 1)
    rows.append([xv, yv, top(77, 0), KILL])
    while len(rows) < 64:
        rows.append([rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(256), PASS])
    return rows[:64]


def rows_far():
    """64 rows whose top limbs keep x + y, x - y and z far from each other and from a wrap."""
    rng = random.Random(16)
    rows = []
    for _ in range(64):
        xv = top(0x60000000 + rng.getrandbits(24), rng.getrandbits(224))
        yv = top(0x10000000 + rng.getrandbits(24), rng.getrandbits(224))
        zv = top(rng.choice([0x20000000, 0x7F000000]) + rng.getrandbits(20), rng.getrandbits(224))
        rows.append([xv, yv, zv, PASS])
    return rows


def rows_wrap(sub: bool):
    """Hazard rows where the open-carry top limb of x + y (x - y) sits on or next to the wrap
    (0xFFFFFFFF, 0xFFFFFFFE, 0, 1), with and without the carry (borrow) that takes it across,
    against a z far from both ends."""
    rng = random.Random(18 + sub)
    rows = []
    for s7 in (M32, M32 - 1, 0, 1, 0x7FFFFFFF, 0x80000000):
        for carry in (0, 1):
            for z7 in (0x40000000, 0x80000000, 0xC0000000, 0x00001000):
                x7 = 0x30000000 + rng.getrandbits(24)
                y7 = (x7 - s7) & M32 if sub else (s7 - x7) & M32
                if sub:
                    xl, yl = (0, LOW) if carry else (LOW, 0)
                else:
                    xl, yl = (LOW, 1) if carry else (5, 7)
                rows.append([top(x7, xl), top(y7, yl), top(z7, rng.getrandbits(224)), PASS])
    return rows


def hazard_rows():
    """Every crafted row of the carry-slack sets: a test puts each alone into a wave of rows_far,
    so that no other lane's fallback hides what the decision makes of it."""
    return rows_carry(False) + rows_carry(True) + rows_wrap(False) + rows_wrap(True)


def gpu_rows():
    """256 rows, four waves, for the GPU test."""
    return rows_decided() + rows_ordered() + rows_carry(False) + (rows_wrap(True) + rows_far())[:64]
