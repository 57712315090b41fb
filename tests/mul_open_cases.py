"""Hand-built tapes and rows for the open top-limb products of the tape JIT (jit.cpp op_mul_open,
emit_staged layer 4), shared by tests/test_jit_mul_open.py (host emulator) and
tests/test_gpu_jit_mul_open.py (MI355X).

A staged ordered compare may read a product through T = (C_7 + floor(C_6 / 2^32)) mod 2^32 -- C_k
the sum of column k's terms -- instead of its true limb 7 = T + e, 0 <= e <= hi.  open_T and
open_hi restate the emitter's rule in Python integers.

Every tape is `guard & cmp(L(x, y), R(z))` over columns x, y, z, w of a 4- or 7-column set; the
guard `w < 2^255` passes on every row here.  L holds the product; R(z) is z, or z times an odd
constant where the compare has a product on both sides, so a row can put R's value anywhere.  A
crafted row takes a pair (x, y), computes L with Python integers and sets R to L with its top limb
moved next to T, T + e and T + hi.  Each crafted row is one lane of a wave whose other 63 rows are
random (their top limbs are far apart: decidable), as tests/conj_cases.py near_tie_rows does."""
import random

from mythril_amd.tape import Op, TapeSet

M = (1 << 256) - 1
M32 = 0xFFFFFFFF
LOW = (1 << 224) - 1      # limbs 0..6
PASS = 0                  # w of every row: the guard holds

KINDS = [("ult", Op.BVULT), ("ule", Op.BVULE), ("ugt", Op.BVUGT), ("uge", Op.BVUGE),
         ("slt", Op.BVSLT), ("sle", Op.BVSLE), ("sgt", Op.BVSGT), ("sge", Op.BVSGE)]

K_RANDOM = 0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95
K_ODD = 0xC2B2AE3D27D4EB4F165667B19E3779B97F4A7C15F39CC0605CEDC8341082276B
K_ADD = 0x6A09E667F3BCC908BB67AE8584CAA73B3C6EF372FE94F82BA54FF53A5F1D36F1
# the pool-constant shapes a product meets: 0, 1, all ones, 160 bits, 32 bits, a full word
CONSTS = [("k0", 0), ("k1", 1), ("kones", M), ("k160", (1 << 160) - 1 - (0xABCDEF << 64)),
          ("k32", 0xDEADBEEF), ("kfull", K_RANDOM)]
# column indices of x, y, z, w
LAYOUT = {4: (0, 1, 2, 3), 7: (5, 1, 6, 3)}


def limbs(v: int):
    return [(v >> (32 * k)) & M32 for k in range(8)]


def top(t7: int, low: int = 0) -> int:
    return ((t7 & M32) << 224) | (low & LOW)


# -- the rule, restated --------------------------------------------------------------------------
def open_T(a: int, b: int) -> int:
    """The inexact top limb of a * b the open product computes."""
    x, y = limbs(a), limbs(b)
    c6 = sum(x[i] * y[6 - i] for i in range(7))
    c7 = sum(x[i] * y[7 - i] for i in range(8))
    return (c7 + (c6 >> 32)) & M32


def open_e(a: int, b: int) -> int:
    """True limb 7 of a * b minus open_T, mod 2^32."""
    return ((((a * b) & M) >> 224) - open_T(a, b)) & M32


def open_hi(ka, kb) -> int:
    """The slack bound of jit.cpp open_mul_slack.  ka, kb: eight limbs each, an int for a limb
    known at compile time, None for a variable one."""
    def mx(l):
        return M32 if l is None else l

    def col(k):
        return sum(mx(ka[i]) * mx(kb[k - i]) for i in range(k + 1)
                   if ka[i] != 0 and kb[k - i] != 0)

    cm = 0
    for k in range(6):
        cm = (cm + col(k)) >> 32
    return (min(M32, col(6)) + cm) >> 32


VAR = [None] * 8


# -- tapes ---------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, tape, lhs, rhs_k, prod, hi):
        self.name = name
        self.tape = tape      # index in the set
        self.lhs = lhs        # L(x, y) in Python integers
        self.rhs_k = rhs_k    # R(z) = z * rhs_k (1: R(z) = z)
        self.prod = prod      # (x, y) -> the open product's factors, or None
        self.hi = hi          # slack of the whole side L (products' hi plus the chain's)


def build(n_cols: int):
    """(tape set, [Case]): the tapes whose product may be open."""
    ts = TapeSet()
    b = ts.builder()
    cols = [b.var("c%d" % i) for i in range(n_cols)]
    x, y, z, w = (cols[i] for i in LAYOUT[n_cols])
    guard = b.op(Op.BVULT, w, b.const(1 << 255, 256))
    cases = []

    def add(name, op, lnode, lhs, prod, hi, rnode=None, rhs_k=1):
        root = b.op(Op.AND, guard, b.op(op, lnode, z if rnode is None else rnode))
        cases.append(Case(name, len(ts.tapes), lhs, rhs_k, prod, hi))
        ts.add(b.finish(root))

    hv = open_hi(VAR, VAR)
    # variable x variable under each of the eight compares
    for name, op in KINDS:
        add("vv_" + name, op, b.op(Op.BVMUL, x, y), lambda p, q: p * q & M, lambda p, q: (p, q), hv)
    add("sq", Op.BVULT, b.op(Op.BVMUL, x, x), lambda p, q: p * p & M, lambda p, q: (p, p), hv)
    # variable x each constant shape
    for i, (cname, k) in enumerate(CONSTS):
        add("c_" + cname, KINDS[(3 * i + 1) % 8][1], b.op(Op.BVMUL, x, b.const(k, 256)),
            lambda p, q, k=k: p * k & M, lambda p, q, k=k: (p, k), open_hi(VAR, limbs(k)))
    # a product inside an add / sub / rsub chain
    ka = b.const(K_ADD, 256)
    add("chain_add_sub", Op.BVULT, b.op(Op.BVSUB, b.op(Op.BVADD, b.op(Op.BVMUL, x, y), x), ka),
        lambda p, q: (p * q + p - K_ADD) & M, lambda p, q: (p, q), hv + 2)
    add("chain_rsub", Op.BVSGE, b.op(Op.BVSUB, ka, b.op(Op.BVMUL, x, y)),
        lambda p, q: (K_ADD - p * q) & M, lambda p, q: (p, q), hv + 1)
    add("chain_sub_prod", Op.BVUGT, b.op(Op.BVSUB, x, b.op(Op.BVMUL, x, y)),
        lambda p, q: (p - p * q) & M, lambda p, q: (p, q), hv + 1)
    # two products on opposite sides
    ko = b.const(K_ODD, 256)
    add("both_sides_ule", Op.BVULE, b.op(Op.BVMUL, x, y), lambda p, q: p * q & M,
        lambda p, q: (p, q), hv + open_hi(VAR, limbs(K_ODD)), b.op(Op.BVMUL, z, ko), K_ODD)
    add("both_sides_slt", Op.BVSLT, b.op(Op.BVMUL, x, y), lambda p, q: p * q & M,
        lambda p, q: (p, q), hv + open_hi(VAR, limbs(K_ODD)), b.op(Op.BVMUL, z, ko), K_ODD)
    # a product in one ite arm: the arms' slacks differ
    cond = b.op(Op.EQ, b.op(Op.BVAND, x, b.const(1, 256)), b.const(0, 256))
    add("ite_arm", Op.BVULT, b.op(Op.ITE, cond, b.op(Op.BVMUL, x, y), b.op(Op.BVADD, x, y)),
        lambda p, q: (p * q if p % 2 == 0 else p + q) & M, lambda p, q: (p, q), hv)
    add("ite_arm_sgt", Op.BVSGT, b.op(Op.ITE, cond, b.op(Op.BVSUB, y, x), b.op(Op.BVMUL, x, y)),
        lambda p, q: (q - p if p % 2 == 0 else p * q) & M, lambda p, q: (p, q), hv)
    # an exact product under an open one
    add("nested", Op.BVUGE, b.op(Op.BVMUL, b.op(Op.BVMUL, x, y), y),
        lambda p, q: p * q * q & M, lambda p, q: (p * q & M, q), hv)
    # a sum of products past the decision's D > 64 cut-off: comes out unstaged
    terms = [b.op(Op.BVMUL, x, y), b.op(Op.BVMUL, x, x), b.op(Op.BVMUL, y, y)]
    pys = [lambda p, q: p * q, lambda p, q: p * p, lambda p, q: q * q]
    for i in range(8):      # 11 products of variable factors: 11 * 6 + 10 > 64
        k = (K_RANDOM * (2 * i + 3) ^ K_ODD >> i) & M
        terms.append(b.op(Op.BVMUL, b.op(Op.BVXOR, x, b.const(k, 256)), y))
        pys.append(lambda p, q, k=k: (p ^ k) * q)
    s = terms[0]
    for t in terms[1:]:
        s = b.op(Op.BVADD, s, t)
    add("cutoff_sum", Op.BVULT, s, lambda p, q: sum(f(p, q) for f in pys) & M,
        lambda p, q: (p, q), 11 * hv + 10)
    return ts, cases


def build_exact(n_cols: int):
    """(tape set, names): products that must stay exact -- a product feeding a logic op, a shift,
    a division, another product or ==, and one with a second user outside the staged cone.  The
    JIT's text for this set at level 4 equals level 3's."""
    ts = TapeSet()
    b = ts.builder()
    cols = [b.var("c%d" % i) for i in range(n_cols)]
    x, y, z, w = (cols[i] for i in LAYOUT[n_cols])
    guard = b.op(Op.BVULT, w, b.const(1 << 255, 256))
    names = []

    def add(name, conj, *more):
        root = b.op(Op.AND, guard, conj)
        for c in more:
            root = b.op(Op.AND, root, c)
        names.append(name)
        ts.add(b.finish(root))

    p = b.op(Op.BVMUL, x, y)
    add("logic", b.op(Op.BVULT, b.op(Op.BVAND, p, b.const(M ^ (0xFF << 248), 256)), z))
    add("xor", b.op(Op.BVSGT, b.op(Op.BVXOR, p, x), z))
    add("shift", b.op(Op.BVULE, b.op(Op.BVLSHR, p, b.const(8, 256)), z))
    add("shl", b.op(Op.BVUGE, b.op(Op.BVSHL, p, b.const(40, 256)), z))
    add("div", b.op(Op.BVULT, b.op(Op.BVUDIV, p, b.op(Op.BVOR, z, b.const(1 << 200, 256))), x))
    add("mul_eq", b.op(Op.EQ, b.op(Op.BVMUL, p, z), x))
    add("eq", b.op(Op.EQ, p, z))
    add("second_user", b.op(Op.BVULT, p, z), b.op(Op.BVUGE, b.op(Op.BVXOR, p, x), y))
    return ts, names


# -- rows ----------------------------------------------------------------------------------------
def inv(k: int) -> int:
    return pow(k, -1, 1 << 256)


def operand_pairs(case, rng: random.Random, n_search: int = 300):
    """(x, y) pairs for a case: all limbs 0xFFFFFFFF, pairs with e = 0, one pair per other value
    of e a search finds, and pairs whose product's top limb sits on the unsigned and the signed
    wrap (x = target / y for an odd y)."""
    pairs = [(M, M), (3, 5), (top(0x12345678, 0), 9), (M, 1), (M - 1, M)]
    if case.prod is not None:
        seen = {open_e(*case.prod(p, q)) for p, q in pairs}
        for _ in range(n_search):
            r = rng.random()
            if r < 0.3:
                p, q = rng.getrandbits(256), rng.getrandbits(256)
            elif r < 0.6:   # limbs at the ends of their range: large carries
                p = sum(rng.choice([0, 1, M32, M32 - 1, rng.getrandbits(32)]) << (32 * k)
                        for k in range(8))
                q = sum(rng.choice([M32, M32, M32 - 1, rng.getrandbits(32)]) << (32 * k)
                        for k in range(8))
            else:
                p, q = M - rng.getrandbits(40), M - rng.getrandbits(rng.choice([8, 40, 200]))
            e = open_e(*case.prod(p, q))
            if e not in seen:
                seen.add(e)
                pairs.append((p, q))
    for t7 in (0, 2, M32, M32 - 2, 0x7FFFFFFF, 0x80000000, 0x80000003):
        q = rng.getrandbits(256) | 1
        pairs.append((top(t7, rng.getrandbits(224)) * inv(q) & M, q))
    return pairs


def crafted_rows(case, pair, n_cols: int, points="all"):
    """Rows for one (x, y): R's value is L's with its top limb at T - 1, T, T + e, T + e + 1,
    T + hi, T + hi + 1 (T = true limb 7 of L minus the product's e: what the slice computes when
    nothing else is open), and next to L itself."""
    p, q = pair
    lv = case.lhs(p, q)
    l7, low = lv >> 224, lv & LOW
    e = open_e(*case.prod(p, q)) if case.prod is not None else 0
    t = (l7 - e) & M32
    targets = [top(t + d, low) for d in (-1, 0, e, e + 1, case.hi, case.hi + 1)]
    targets += [(lv - 1) & M, (lv + 1) & M, top(l7 - 1, low)]
    if points == "few":
        targets = [top(t, low), lv, top(t + e + 1, low)]
    rows, seen = [], set()
    for tv in targets:
        if tv in seen:
            continue
        seen.add(tv)
        row = [0] * n_cols
        ix, iy, iz, iw = LAYOUT[n_cols]
        row[ix], row[iy], row[iw] = p, q, PASS
        row[iz] = tv * inv(case.rhs_k) & M
        rows.append(row)
    return rows


def decidable_rows(rng: random.Random, n_cols: int, n: int):
    """Random rows: the compared top limbs are far apart and far from a wrap but for a chance of
    about 2^-24 per row; the guard passes."""
    rows = []
    for _ in range(n):
        row = [rng.getrandbits(256) for _ in range(n_cols)]
        row[LAYOUT[n_cols][3]] = PASS
        rows.append(row)
    return rows


def waves_of(crafted, rng: random.Random, n_cols: int):
    """One wave of 64 rows per crafted row, the crafted row in a random lane; then one wave of
    decidable rows only.  Returns (rows, index of each crafted row)."""
    rows, at = [], []
    for row in crafted:
        wave = decidable_rows(rng, n_cols, 64)
        lane = rng.randrange(64)
        wave[lane] = [v if i in LAYOUT[n_cols] else wave[lane][i] for i, v in enumerate(row)]
        at.append(len(rows) + lane)
        rows += wave
    rows += decidable_rows(rng, n_cols, 64)
    return rows, at


def case_rows(case, n_cols: int, seed: int = 0):
    """(rows, crafted lanes) of a case for the emulator test."""
    rng = random.Random(0x0FE40000 + 131 * case.tape + n_cols + seed)
    crafted = []
    for pair in operand_pairs(case, rng):
        crafted += crafted_rows(case, pair, n_cols)
    return waves_of(crafted, rng, n_cols)


def gpu_rows(cases, n_cols: int, lanes_per_case: int = 6):
    """One row set for every tape of the set: a few crafted lanes per case (all limbs ones and a
    pair on the wrap; on T, on L and one past T + e), each alone in its wave, and a partial last
    wave of decidable rows."""
    rng = random.Random(0x0FE50000 + n_cols)
    crafted = []
    for case in cases:
        pairs = operand_pairs(case, rng, n_search=0)
        mine = []
        for pair in (pairs[0], pairs[-1], pairs[-3]):
            mine += crafted_rows(case, pair, n_cols, points="few")
        crafted += mine[:lanes_per_case]
    rows, at = waves_of(crafted, rng, n_cols)
    return rows[:len(rows) - 23], at
