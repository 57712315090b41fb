"""Random root conjunctions of 256-bit compares for the count path of the tape JIT (jit.cpp
schedule_conjuncts, plan_stages, emit_staged, stage_decide), shared by tests/test_jit_conj.py
(host emulator) and tests/test_gpu_jit_conj.py (MI355X).  Everything is drawn from one
random.Random(seed), so both see the same tapes and rows.

Two families over 256-bit columns c0..c{n-1}, Bool roots:

random_set: 24 tapes, each an AND chain of 1..6 compares (either nesting, a literal true now and
then, a conjunct under NOT now and then) whose sides are cones of depth <= 3, add/sub chains of up
to 40 terms or constants, with sub-cones shared between the conjuncts of a tape; about 200 rows
whose columns share a top limb within +-2, share limb 0, take edge values or are random.

near_tie_set: 8 tapes `guard & cmp(A, W) [& one more compare]`, A a cone over every column but the
last and W the last column plus an offset, A and W added as value tapes too.  near_tie_rows makes
waves of 64 random rows with one crafted lane each, in which W = A + d7 2^224 + lo: the compared
top limbs on, next to and just outside every slack window the decision can have, in a lane no
other lane's fallback recomputes."""
import random

import numpy as np

from mythril_amd.tape import Op, TapeSet
from oracle import ctape
from tests.fuzz import interesting

M = (1 << 256) - 1
M32 = 0xFFFFFFFF
LOW = (1 << 224) - 1      # limbs 0..6
N_TAPES = 24              # of a random set
N_TIES = 8                # conjunctions of a near-tie set
COMPARES = [Op.EQ, Op.BVULT, Op.BVULE, Op.BVUGT, Op.BVUGE, Op.BVSLT, Op.BVSLE, Op.BVSGT, Op.BVSGE]
SHIFTS = [0, 1, 4, 8, 31, 32, 33, 64, 100, 224, 252, 255]
EXT_WIDTHS = [8, 32, 64, 160, 224]
CHAIN_LENGTHS = [1, 3, 8, 20, 31, 32, 33, 40]
TOP7 = [0, 1, 2, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF]
D7 = [0] + [s * d for d in (1, 2, 3, 4, 9, 32, 33, 34, 64, 65, 66) for s in (1, -1)]
TIE_PAIRS = [(d7, sign) for d7 in D7 for sign in (0, 1, -1)]   # (top-limb distance, sign of lo)


class ConjGen:
    def __init__(self, rng: random.Random, n_cols: int, rows=None):
        self.rng = rng
        self.rows = rows  # conjunctions prefer conjuncts that hold on some of them, not on all
        self.ts = TapeSet()
        self.b = self.ts.builder()
        self.cols = [self.b.var("c%d" % i) for i in range(n_cols)]
        self.pool = []    # sub-cones of the tape being built, for later conjuncts to reuse

    # -- operands -------------------------------------------------------------------------------
    def const_value(self) -> int:
        rng = self.rng
        r = rng.random()
        if r < 0.35:
            return interesting(rng, 256)
        if r < 0.75:
            return (rng.choice(TOP7) << 224) | rng.getrandbits(224)
        return rng.getrandbits(256)

    def const(self):
        return self.b.const(self.const_value(), 256)

    def leaf(self, cols):
        return self.rng.choice(cols)

    def chain(self, cols):
        """An add/sub chain over leaves (a constant now and then); a quarter are leaf - chain."""
        b, rng = self.b, self.rng
        x = self.leaf(cols)
        for _ in range(rng.choice(CHAIN_LENGTHS)):
            y = self.const() if rng.random() < 0.15 else self.leaf(cols)
            x = b.op(rng.choice([Op.BVADD, Op.BVSUB]), x, y)
        if rng.random() < 0.25:
            x = b.op(Op.BVSUB, self.leaf(cols), x)
        return x

    def cone(self, depth, cols, unsliceable=True):
        b, rng = self.b, self.rng
        if depth <= 0 or rng.random() < 0.12:
            return self.leaf(cols) if rng.random() < 0.85 else self.const()
        if self.pool and rng.random() < 0.15:
            return rng.choice(self.pool)
        d = depth - 1
        sub = lambda: self.cone(d, cols, unsliceable)
        r = rng.random()
        if unsliceable and r < 0.05:
            c = rng.choice(["udiv", "urem", "shlv", "lshrv"])
            op = {"udiv": Op.BVUDIV, "urem": Op.BVUREM, "shlv": Op.BVSHL, "lshrv": Op.BVLSHR}[c]
            x = b.op(op, sub(), sub())
        else:
            c = rng.choice(["add", "add", "sub", "sub", "rsub", "and", "or", "xor", "mul", "not",
                            "neg", "shl", "lshr", "ite", "zext", "sext"])
            if c in ("add", "sub", "and", "or", "xor", "mul"):
                op = {"add": Op.BVADD, "sub": Op.BVSUB, "and": Op.BVAND, "or": Op.BVOR,
                      "xor": Op.BVXOR, "mul": Op.BVMUL}[c]
                y = self.const() if rng.random() < 0.2 else sub()
                x = b.op(op, sub(), y)
            elif c == "rsub":        # constant - cone
                x = b.op(Op.BVSUB, self.const(), sub())
            elif c in ("not", "neg"):
                x = b.op(Op.BVNOT if c == "not" else Op.BVNEG, sub())
            elif c in ("shl", "lshr"):
                k = rng.choice(SHIFTS + [rng.randrange(256)])
                x = b.op(Op.BVSHL if c == "shl" else Op.BVLSHR, sub(), b.const(k, 256))
            elif c == "ite":
                cond = b.op(rng.choice(COMPARES), sub(), self.const() if rng.random() < 0.3
                            else sub())
                x = b.op(Op.ITE, cond, sub(), sub())
            else:
                w = rng.choice(EXT_WIDTHS)
                low = b.op(Op.EXTRACT, sub(), imm0=w - 1, imm1=0)
                x = b.op(Op.ZEXT if c == "zext" else Op.SEXT, low, imm0=256 - w)
        self.pool.append(x)
        return x

    def side(self, cols, const=True, chain=0.15):
        """(a compare's operand, whether it is a constant)."""
        rng = self.rng
        r = rng.random()
        if const and r < 0.30:
            return self.const(), True
        if r < 0.30 + chain:
            return self.chain(cols), False
        return self.cone(rng.randint(1, 3), cols), False

    def compare(self, cols):
        b, rng = self.b, self.rng
        op = rng.choice(COMPARES)
        a, ac = self.side(cols)
        # a chain against a chain more often than chance: both sides' slacks add up (D near 64)
        long_a = self.b.nodes[a][0] in (Op.BVADD, Op.BVSUB) and rng.random() < 0.5
        c, _ = self.side(cols, const=not ac and not long_a, chain=0.6 if long_a else 0.15)
        if op == Op.EQ and rng.random() < 0.5:
            # an == that holds on some rows: one side is the other under a condition
            cond = b.op(rng.choice(COMPARES), self.cone(1, cols), self.cone(1, cols))
            x = c if ac else a
            y = b.op(Op.ITE, cond, x, self.cone(2, cols))
            a, c = (x, y) if rng.random() < 0.5 else (y, x)
        return b.op(op, a, c)

    def conjunct(self):
        """A compare over every column, under NOT now and then; one that is constant over the
        rows is drawn again (up to three times) two times in three."""
        b, rng = self.b, self.rng
        for _ in range(4):
            c = self.compare(self.cols)
            if rng.random() < 0.1:
                c = b.op(Op.NOT, c)
            if self.rows is None or rng.random() < 0.33:
                break
            bits = tape_bits(self.ts, b.finish(c), self.rows)
            if 0 < int(bits.sum()) < len(self.rows):
                break
        return c

    # -- tapes ----------------------------------------------------------------------------------
    def nest(self, items):
        """AND of the items in order: left-nested, right-nested or split at random."""
        b, rng = self.b, self.rng
        mode = rng.choice(["left", "right", "mixed"])

        def rec(xs):
            if len(xs) == 1:
                return xs[0]
            k = {"left": len(xs) - 1, "right": 1}.get(mode) or rng.randrange(1, len(xs))
            return b.op(Op.AND, rec(xs[:k]), rec(xs[k:]))

        return rec(items)

    def conjunction(self):
        b, rng = self.b, self.rng
        self.pool = []
        items = []
        for _ in range(rng.randint(1, 6)):
            items.append(self.conjunct())
        if rng.random() < 0.15:
            items.insert(rng.randrange(len(items) + 1), b.true())
        return self.ts.add(b.finish(self.nest(items)))

    def near_tie(self):
        """(tape, A's value tape, W's value tape)."""
        b, rng, ts = self.b, self.rng, self.ts
        self.pool = []
        inner, last = self.cols[:-1], self.cols[-1]
        if rng.random() < 0.4:
            a = self.chain(inner)
        else:
            a = self.cone(rng.randint(1, 3), inner, unsliceable=False)
        form = rng.randrange(4)
        w = [last, b.op(Op.BVADD, last, self.const()), b.op(Op.BVSUB, last, self.const()),
             b.op(Op.BVADD, last, self.cols[0])][form]
        op = rng.choice(COMPARES)
        cmp_ = b.op(op, a, w) if rng.random() < 0.5 else b.op(op, w, a)
        guard = b.op(Op.BVULT, self.cols[0], b.const(3 << 254, 256))
        items = [guard, cmp_]
        if rng.random() < 0.5:
            items.append(self.compare(self.cols))
        rng.shuffle(items)
        t = ts.add(b.finish(self.nest(items)))
        return t, ts.add(b.finish(a)), ts.add(b.finish(w))


# -- rows ---------------------------------------------------------------------------------------
def random_rows(rng: random.Random, n_cols: int, n_rows: int):
    rows = []
    for _ in range(n_rows):
        kind = rng.randrange(4)
        if kind == 0:       # every column's top limb within +-2 of one value
            t7 = rng.choice(TOP7 + [rng.getrandbits(32)] * 4)
            row = [(((t7 + rng.randint(-2, 2)) & M32) << 224)
                   | rng.choice([0, 1, LOW, rng.getrandbits(224)]) for _ in range(n_cols)]
        elif kind == 1:     # one limb 0
            l0 = rng.getrandbits(32)
            row = [(rng.getrandbits(256) & ~M32) | l0 for _ in range(n_cols)]
        elif kind == 2:
            row = [interesting(rng, 256) for _ in range(n_cols)]
        else:
            row = [rng.getrandbits(256) for _ in range(n_cols)]
        rows.append(row)
    return rows


def random_set(seed: int, n_cols: int):
    """(tape set of N_TAPES conjunctions, rows)."""
    rng = random.Random(0xC0170000 + seed)
    rows = random_rows(rng, n_cols, 197 + rng.randrange(10))
    g = ConjGen(rng, n_cols, rows)
    for _ in range(N_TAPES):
        g.conjunction()
    return g.ts, rows


def near_tie_set(seed: int, n_cols: int):
    """(tape set, [(tape, A_tape, W_tape)] of its N_TIES conjunctions)."""
    rng = random.Random(0x71E50000 + seed)
    g = ConjGen(rng, n_cols)
    return g.ts, [g.near_tie() for _ in range(N_TIES)]


def near_tie_rows(ts, triple, rng: random.Random, pairs=TIE_PAIRS):
    """One wave of 64 random rows per (d7, sign of lo) of `pairs`; one random lane of each wave is
    crafted so that W = A + d7 2^224 + lo and the guard holds."""
    _, ta, tw = triple
    n = ts.n_vars
    rows = []
    for d7, sign in pairs:
        wave = [[rng.getrandbits(256) for _ in range(n)] for _ in range(64)]
        row = wave[rng.randrange(64)]
        row[0] &= M >> 1
        mag = rng.randint(1, 3) if rng.random() < 0.5 else rng.getrandbits(200) | 1
        row[-1] = 0
        a = ctape.evaluate(ts, ta, row) & M
        off = ctape.evaluate(ts, tw, row) & M     # W = last column + off
        row[-1] = (a + (d7 << 224) + sign * mag - off) & M
        assert (ctape.evaluate(ts, tw, row) - a) & M == ((d7 << 224) + sign * mag) & M
        rows += wave
    return rows


def near_tie_case(seed: int, n_cols: int):
    """(tape set, triples, rows, first row of each triple's waves): every (d7, sign) pair at least
    once per set, dealt over the set's conjunctions; each gets W = A (the one row an == holds on)
    and nine other pairs."""
    ts, triples = near_tie_set(seed, n_cols)
    rng = random.Random(0x71E60000 + seed)
    pairs = [p for p in TIE_PAIRS if p != (0, 0)]
    rng.shuffle(pairs)
    pairs += pairs[:(-len(pairs)) % len(triples)]
    rows, first = [], []
    for i, tr in enumerate(triples):
        first.append(len(rows))
        rows += near_tie_rows(ts, tr, rng, [(0, 0)] + pairs[i::len(triples)])
    return ts, triples, rows, first


# -- the oracle ---------------------------------------------------------------------------------
def soa_of(rows, n_vars):
    """[n_vars, 8, rows] u32 limbs of rows of column values."""
    buf = b"".join(v.to_bytes(32, "little") for r in rows for v in r)
    a = np.frombuffer(buf, dtype="<u4").reshape(len(rows), n_vars, 8)
    return np.ascontiguousarray(a.transpose(1, 2, 0))


def root_bits(ts, tape: int, rows):
    """Whether the C oracle's root is not 0, on every row (int64 array): the root bit of a Bool
    tape, and what the count path counts for a value tape."""
    return tape_bits(ts, ts.tapes[tape], rows)


def tape_bits(ts, tape, rows):
    """root_bits of a tape over the set's columns and constants that need not be in the set."""
    lib = ctape.lib()
    nodes = np.ascontiguousarray(tape.nodes)
    consts = np.ascontiguousarray(ts.pool.to_array())
    buf = b"".join(v.to_bytes(32, "little") for r in rows for v in r)
    a = np.frombuffer(buf, dtype="<u4").reshape(len(rows), ts.n_vars * 8)
    out = np.zeros(34, dtype=np.uint32)
    bits = np.zeros(len(rows), dtype=np.int64)
    args = (nodes.ctypes.data, len(nodes), consts.ctypes.data, len(ts.pool.values))
    stride = a.strides[0]
    for r in range(len(rows)):
        if lib.ct_eval(*args, a.ctypes.data + r * stride, ts.n_vars, out.ctypes.data) != 0:
            raise ValueError("malformed tape")
        bits[r] = out.any()
    return bits
