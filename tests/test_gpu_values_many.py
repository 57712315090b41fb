"""Root values of MANY tapes per launch (mh_eval_values_many, the path behind Model.eval batches
and Sieve.eval_tapeset) against the Python oracle, bit for bit, tape by tape.

The other values checks (test_gpu_parity, test_gpu_native, test_gpu_interp_core) run one tape per
launch; the launches that put several tapes through one workgroup are otherwise checked through
hit counts and first hits only.  Here the workgroup loop of sieve_body (csrc/sieve_kernels.hip:
chunk formation by ballot, s_meta, the LDS staging of the slot words, the prefetch of the next
tape's first window, the register planes successive tapes share, the grid-y split of the id list
and the values_out indexing) has its 256-bit results compared with oracle.smt_eval.evaluate.

Two things about the launch shape decide what a list exercises (sieve_kernels.hip launch_block):
one row is one row block, so grid y = min(ids of the launch, 256) -- a list of up to 256 ids of a
variant gives every id a workgroup of its own, and only beyond that does a workgroup walk several
tapes (ids * y / 256 .. ids * (y + 1) / 256 of the launch's ascending list).  `deep()` below
builds the lists whose LAST workgroup walks exactly a chosen sequence of tapes.

Kernel variants.  The set has 6 columns, more than the 4 the kernel preloads, so NO column is
pinned (compile.cpp:164, capi.cpp make_params n_pre) and every read of a column is a D_LOADVAR
(compile.cpp:615-621), which fold_constants never folds (compile.cpp:1036) and which is a
complex op (dev_isa.h:90-95, compile.cpp:1104: F_CPLX).  A tape that reads no column has only
constant operands and folds to one LOADC / TRUE / FALSE (compile.cpp:1041-1066) unless it holds a
keccak (never folded, compile.cpp:1036: F_KECCAK), so a tape without a complex op is a single
constant load and sits in the smallest register class.  The variants (9 registers, asm only) = 4
and (15 registers, asm only) = 8 therefore cannot occur in a 6-column set; the fixture asserts
the other ten exactly, and a second, 3-column set (`pinned`) puts variants 4 and 8 (and 0)
through the same multi-tape checks.
"""
import random
import threading

import numpy as np
import pytest

from mythril_amd import native
from mythril_amd.tape import Op, TapeSet
from oracle import smt_eval as E
from tests.fuzz import TapeFuzzer, assignment_soa, soa_row, tree_tape

pytestmark = pytest.mark.gpu

N_COLS = 6
LDS_SLOTS = 2048   # sieve_kernels.hip kLdsInsns
CHUNK = 64         # sieve_kernels.hip kChunk
GRID_Y = 256       # launch_block: the cap of grid y for a one-row run
F_KECCAK, F_EVM, F_CPLX = 2, 4, 8  # dev_isa.h
REACHABLE = {0, 1, 2, 3, 5, 6, 7, 9, 10, 11}  # module docstring


def variant_of(x):  # csrc/kernels.h variant_of
    nr = 0 if x["n_regs"] <= 7 else 1 if x["n_regs"] <= 9 else 2
    f = x["features"]
    return nr * 4 + (3 if f & F_EVM else 2 if f & F_KECCAK else 1 if f & F_CPLX else 0)


# ---- the tapes ---------------------------------------------------------------------------------
def _zext256(b, leaf):
    return b.op(Op.ZEXT, leaf, imm0=192)


def wrap_keccak(b, leaf):
    return b.op(Op.EXTRACT, b.op(Op.KECCAK, leaf), imm0=70, imm1=7)


def wrap_byte(b, leaf):
    return b.op(Op.EXTRACT, b.op(Op.EVM_BYTE, b.const(27, 256), _zext256(b, leaf)),
                imm0=63, imm1=0)


def wrap_signext(b, leaf):
    return b.op(Op.EXTRACT, b.op(Op.EVM_SIGNEXTEND, b.const(3, 256), _zext256(b, leaf)),
                imm0=90, imm1=27)


def wrap_exp(b, leaf):
    return b.op(Op.EXTRACT, b.op(Op.EVM_EXP, _zext256(b, leaf), b.const(3, 256)),
                imm0=191, imm1=128)


def wrap_ovfl(b, leaf):  # an overflow predicate: a C++-path op beside the column loads
    return b.op(Op.ITE, b.op(Op.BVMUL_NOOVFL_U, leaf, leaf), leaf, b.op(Op.BVNOT, leaf))


WRAPS = [None, wrap_ovfl, wrap_keccak, wrap_byte, wrap_signext, wrap_exp]
# leaves of a wide_tape per register class: k + 1 registers, so 7 | 8, 9 | 10, 15 are the edges
# of the classes (kernels.h nr_class; tests/emu.py Emulator.eval returns the n_regs)
WIDE_LEAVES = (4, 6, 7, 8, 9, 14)


def wide_tape(ts, b, k, salt, n_cols=N_COLS, wrap=None, compare=True):
    """k 64-bit slices of the columns, each used twice -- in a sum and, last first, in a chain of
    products / xors / differences -- so all k stay live: k + 1 registers, about 16 slots a leaf.
    `wrap(b, leaf)` replaces leaf 0 with a 64-bit term of its own (a keccak, an EVM helper);
    compare=False leaves the 64-bit value itself as the root."""
    leaves = []
    for i in range(k):
        lo = (7 * i + salt) % 192
        leaf = b.op(Op.EXTRACT, b.var("v%d" % ((i + salt) % n_cols), 256), imm0=lo + 63, imm1=lo)
        leaves.append(wrap(b, leaf) if wrap is not None and i == 0 else leaf)
    s = leaves[0]
    for x in leaves[1:]:
        s = b.op(Op.BVADD, s, x)
    p = leaves[-1]
    for i, x in enumerate(reversed(leaves[:-1])):
        p = b.op((Op.BVMUL, Op.BVXOR, Op.BVSUB)[i % 3], p, x)
    root = b.op(Op.BVXOR, s, p)
    return ts.add(b.finish(b.op(Op.BVULT, root, b.const(1 << 62, 64)) if compare else root))


def chain(b, rng, xs, n, newest):
    """((c1 & c2) & c3) ... & newest, as a path condition grows: n conjuncts true on almost every
    row (an inline 256-bit constant each), so the walk reaches the tape's last window."""
    acc = None
    for _ in range(n):
        x, y = rng.sample(xs, 2)
        # (no sub-term shared between conjuncts: shared sums would stay live in registers)
        c = b.op(Op.NOT, b.op(Op.EQ, b.op(Op.BVADD, x, b.const(rng.getrandbits(256), 256)), y))
        acc = c if acc is None else b.op(Op.AND, acc, c)
    return b.op(Op.AND, acc, newest)


def build_tapes(n_cols=N_COLS, seed=0x7A9E5):
    """The module's tape set: fuzzed tapes (keccak and the EVM helpers on) of every root sort,
    wide tapes per register class with each complex-op kind at leaf 0, 66 small ones of one
    variant (64 consecutive ones exceed the LDS chunk), a tree_tape, constant tapes, hand-written
    tapes over columns 4 and 5, and two conjunction chains longer than the LDS chunk that sit
    inside their variant's id range."""
    rng = random.Random(seed)
    ts = TapeSet()
    fz = TapeFuzzer(rng, ts, n_vars=n_cols, allow_keccak=True, allow_evm=True, max_depth=3)
    b = fz.b
    xs = [b.var("v%d" % i, 256) for i in range(n_cols)]
    add = lambda root: ts.add(b.finish(root))  # noqa: E731
    makers = []
    for i in range(36):  # fuzzed: Bool roots and bit-vector roots of widths 1, 8, 255, 256, ...
        def fuzzed(i=i):
            fz.max_depth = 1 + i % 3
            kind = i % 6
            if kind == 0:
                return fz.tape(root_bool=True)
            w = (1, 8, 255, 256, rng.choice([7, 33, 64, 160]))[kind - 1]
            return add(fz.bv(w, fz.max_depth))
        makers.append(fuzzed)
    for ki, k in enumerate(WIDE_LEAVES):  # each register class x each complex-op kind
        for wi, wrap in enumerate(WRAPS):
            for rep in range(2):  # a Bool root and a 64-bit one
                makers.append(lambda k=k, wrap=wrap, s=31 * ki + 5 * wi + rep, rep=rep:
                              wide_tape(ts, b, k, s, n_cols=n_cols, wrap=wrap, compare=bool(rep)))
    for i in range(66):  # one variant, 40-odd slots each: a 64-tape chunk is cut by words
        makers.append(lambda i=i: wide_tape(ts, b, 3, 3 * i + 1, n_cols=n_cols,
                                            compare=bool(i % 2)))
    consts = [lambda: add(b.const(rng.getrandbits(256), 256)),
              lambda: add(b.const(0xA5, 8)),
              lambda: add(b.op(Op.AND, b.true(), b.op(Op.NOT, b.false()))),
              lambda: add(b.op(Op.BVMUL, b.const(rng.getrandbits(255), 255),
                               b.const(rng.getrandbits(255), 255))),
              lambda: add(b.op(Op.BVULT, b.const(3, 1), b.const(0, 1)))]
    makers += consts
    hand = [lambda: add(xs[5]),                                            # a column is the root
            lambda: add(b.op(Op.EQ, xs[4], xs[5])),
            lambda: add(b.op(Op.EXTRACT, xs[5], imm0=255, imm1=255)),      # width 1
            lambda: add(b.op(Op.EXTRACT, xs[4], imm0=15, imm1=8)),         # width 8
            lambda: add(b.op(Op.EXTRACT, b.op(Op.BVADD, xs[4], xs[0]), imm0=254, imm1=0)),
            lambda: add(b.op(Op.ITE, b.op(Op.BVULT, xs[4], xs[5]), xs[0], b.op(Op.BVNOT, xs[3]))),
            lambda: add(b.op(Op.KECCAK, b.op(Op.CONCAT, xs[4], xs[5]))),
            lambda: add(b.op(Op.EVM_ADDMOD, xs[4], xs[5], xs[2], imm0=1)),
            lambda: add(b.op(Op.NOT, b.op(Op.BVSLT, xs[5], xs[4]))),
            lambda: add(chain(b, rng, xs, 12, b.op(Op.BVULT, xs[1], b.const(1 << 255, 256)))),
            lambda: tree_tape(ts, b, 5, 9, n_cols=n_cols)]
    makers += hand
    rng.shuffle(makers)
    always = b.op(Op.NOT, b.op(Op.BVULT, xs[2], b.const(0, 256)))
    half = b.op(Op.BVULT, xs[5], b.const(1 << 255, 256))
    # early in the id order: tapes of their variant before, between and after them, and 64
    # consecutive ones of that variant after the second
    makers.insert(len(makers) // 10, lambda: add(chain(b, rng, xs, 300, always)))
    makers.insert(len(makers) // 5, lambda: add(chain(b, rng, xs, 262, half)))
    for m in makers:
        m()
    return ts


def build_pinned_tapes(seed=0x91A7):
    """A 3-column set (every column pinned): the asm-only kernel of each register class,
    variants 0, 4 and 8, which a 6-column set cannot reach."""
    rng = random.Random(seed)
    ts = TapeSet()
    b = ts.builder()
    xs = [b.var("v%d" % i, 256) for i in range(3)]
    makers = []
    for i in range(8):
        makers.append(lambda i=i: tree_tape(ts, b, 5, 11 * i, compare=bool(i % 2)))      # 8 regs
        makers.append(lambda i=i: tree_tape(ts, b, 7, 13 * i + 2, compare=bool(i % 2)))  # 10
        makers.append(lambda i=i: ts.add(b.finish(
            b.op(Op.BVULT, xs[i % 3], b.const(1 << (8 * i + 3), 256)))))
        makers.append(lambda i=i: ts.add(b.finish(
            b.op(Op.BVXOR, xs[i % 3], b.op(Op.BVADD, xs[(i + 1) % 3], b.const(i, 256))))))
    rng.shuffle(makers)
    for m in makers:
        m()
    return ts


# ---- a compiled set, its row buffers and the memoised oracle -----------------------------------
def compile_on_a_new_thread(ctx, ts):
    """compile_tape tries first the attempt (columns held or not, cheap sub-terms duplicated)
    that fitted the last tape compiled on its thread (compile.cpp compile_tape, `hint`), so the
    registers a tape gets depend on what the thread compiled before.  A new thread starts from
    the first attempt: the set's variants are then the same after any other test."""
    box = {}

    def work():
        try:
            box["ct"] = ctx.compile(ts)
        except BaseException as e:  # noqa: BLE001 - handed to the caller below
            box["err"] = e

    th = threading.Thread(target=work)
    th.start()
    th.join()
    if "err" in box:
        raise box["err"]
    return box["ct"]


class World:
    def __init__(self, ctx, ts, soas):
        self.ctx, self.ts = ctx, ts
        self.ct = compile_on_a_new_thread(ctx, ts)
        self.info = self.ct.info()
        self.n = len(ts.tapes)
        self.variant = [variant_of(x) for x in self.info]
        self.ids_of = {}
        for t, v in enumerate(self.variant):
            self.ids_of.setdefault(v, []).append(t)  # ascending
        self.soa = dict(soas)
        self.buf = {}
        for k, soa in self.soa.items():
            self.buf[k] = ctx.assignments(ts.n_vars, soa.shape[2])
            self.buf[k].upload(soa)
        self._memo = {}
        self._tables = {}
        self._single = {}

    def close(self):
        for a in self.buf.values():
            a.close()
        self.ct.close()

    def want(self, t, buf, row):
        """The oracle's root value of tape t at (buffer, row): computed once, never changed."""
        key = (t, buf, row)
        if key not in self._memo:
            self._memo[key] = int(E.evaluate(self.ts.tapes[t].nodes, self.ts.pool.values,
                                             soa_row(self.soa[buf], row)))
        return self._memo[key]

    def table(self, buf, row):
        """u32 [n_tapes, 8]: the oracle's values of every tape at (buffer, row)."""
        if (buf, row) not in self._tables:
            tab = np.zeros((self.n, 8), dtype=np.uint32)
            for t in range(self.n):
                x = self.want(t, buf, row)
                for k in range(8):
                    tab[t, k] = (x >> (32 * k)) & 0xFFFFFFFF
            tab.setflags(write=False)
            self._tables[buf, row] = tab
        return self._tables[buf, row]

    def single(self, buf):
        """u32 [n_tapes, 8, rows]: mh_eval_values, one tape per launch, over the whole buffer."""
        if buf not in self._single:
            self._single[buf] = np.stack([native.eval_values(self.ctx, self.ct, t, self.buf[buf])
                                          for t in range(self.n)])
        return self._single[buf]

    def check(self, ids, buf, row):
        """eval_values_many(ids) at (buffer, row) equals the oracle position by position, in as
        many launches as the list has variants (include/mythril_hip.h)."""
        ids = np.asarray(ids, dtype=np.uint32)
        before = native.eval_launches(self.ctx)
        got = native.eval_values_many(self.ctx, self.ct, ids, self.buf[buf], row)
        launches = native.eval_launches(self.ctx) - before
        want = self.table(buf, row)[ids]
        bad = np.nonzero((got != want).any(axis=1))[0]
        if bad.size:
            i = int(bad[0])
            t = int(ids[i])
            raise AssertionError(
                "%d of %d positions differ at (%s, row %d); first: position %d, tape %d "
                "(variant %d, %d slots): got %s, oracle %s"
                % (bad.size, len(ids), buf, row, i, t, self.variant[t], self.info[t]["n_insns"],
                   [hex(int(x)) for x in got[i]], [hex(int(x)) for x in want[i]]))
        assert launches == len({self.variant[int(t)] for t in ids}), launches
        return got


def deep(seq, slices=None):
    """A list whose launch's LAST workgroup walks exactly `seq` (ascending distinct ids of one
    variant): 256 * s ids (s >= len(seq), default len(seq)), the first id repeated, so grid y is
    at its cap and every y-slice holds s ids; the last slice is seq[0] x (s - len + 1), seq[1:]."""
    s = len(seq) if slices is None else slices
    assert s >= len(seq) >= 1 and list(seq) == sorted(set(seq))
    return [seq[0]] * (GRID_Y * s - (len(seq) - 1)) + list(seq[1:])


KEYS = [("A", 0), ("A", 1), ("A", 63), ("A", 64), ("A", 69), ("B", 0)]
FEW = [("A", 0), ("A", 69), ("B", 0)]


def row_buffers(n_cols, seed):
    rng = random.Random(seed)
    return {"A": assignment_soa(rng, n_cols, 70),   # edge-biased values
            "B": assignment_soa(rng, n_cols, 1)}    # the product's shape: one row


@pytest.fixture(scope="module")
def world(gpu_ctx):
    w = World(gpu_ctx, build_tapes(), row_buffers(N_COLS, 0xB0F))
    info = w.info
    assert 150 <= w.n <= 200 and w.ts.n_vars == N_COLS
    # every variant a 6-column set can reach (module docstring), at least twice each
    assert set(w.ids_of) == REACHABLE, sorted(w.ids_of)
    assert all(len(v) >= 2 for v in w.ids_of.values()), {k: len(v) for k, v in w.ids_of.items()}
    assert {v // 4 for v in w.ids_of} == {0, 1, 2} and {v % 4 for v in w.ids_of} == {0, 1, 2, 3}
    widths = {t.nodes[-1]["width"] for t in w.ts.tapes}
    assert {0, 1, 8, 255, 256} <= {int(x) for x in widths}  # Bool roots are width 0
    assert any(64 < x["n_insns"] <= LDS_SLOTS for x in info)  # changes window inside the LDS chunk
    w.big = [t for t in range(w.n) if info[t]["n_insns"] > LDS_SLOTS]  # streamed from memory
    assert len(w.big) >= 2 and len({w.variant[t] for t in w.big}) == 1
    ids = w.ids_of[w.variant[w.big[0]]]
    assert all(ids[0] < t < ids[-1] for t in w.big)  # tapes of the variant before and after
    # a run of 64 consecutive tapes of one variant, none of them streamed, over the LDS chunk:
    # the chunk is cut by words there, not by the 64-tape count
    w.cut = None
    for v, ids in sorted(w.ids_of.items()):
        for i in range(len(ids) - CHUNK + 1):
            run = ids[i:i + CHUNK]
            if (all(info[t]["n_insns"] <= LDS_SLOTS for t in run)
                    and sum(info[t]["n_insns"] for t in run) > LDS_SLOTS and w.cut is None):
                w.cut = run
    assert w.cut is not None
    yield w
    w.close()


@pytest.fixture(scope="module")
def pinned(gpu_ctx):
    w = World(gpu_ctx, build_pinned_tapes(), row_buffers(3, 0xB10))
    assert set(w.ids_of) == {0, 4, 8}, sorted(w.ids_of)
    assert all(len(v) >= 8 for v in w.ids_of.values())
    yield w
    w.close()


def root_width(tape):
    return int(tape.nodes[-1]["width"])


# ---- all tapes, ascending ----------------------------------------------------------------------
@pytest.mark.parametrize("buf,row", KEYS)
def test_all_tapes_ascending(world, buf, row):
    got = world.check(range(world.n), buf, row)
    # the batched path agrees with the single-tape one
    assert np.array_equal(got, world.single(buf)[:, :, row])
    assert got.any(axis=1).sum() > world.n // 4  # the rows do not make everything zero


@pytest.mark.parametrize("buf,row", FEW)
def test_whole_buckets_in_one_workgroup(world, buf, row):
    """Every variant's whole id list walked by ONE workgroup (deep): chunks of 64 tapes and
    chunks cut by words, the streamed tapes between staged ones, every tape after its
    predecessor in the bucket -- each launch alone, then all ten in one call."""
    for v, ids in sorted(world.ids_of.items()):
        world.check(deep(ids), buf, row)
    world.check([t for _, ids in sorted(world.ids_of.items()) for t in deep(ids)], buf, row)


@pytest.mark.parametrize("buf,row", FEW)
def test_pinned_columns_set(pinned, buf, row):
    """Variants 0, 4 and 8 (asm-only kernels; columns preloaded): ascending, unordered, repeated
    and whole buckets in one workgroup."""
    w = pinned
    got = w.check(range(w.n), buf, row)
    assert np.array_equal(got, w.single(buf)[:, :, row])
    rng = random.Random(5)
    w.check(list(reversed(range(w.n))), buf, row)
    w.check(rng.sample(range(w.n), w.n), buf, row)
    for ids in w.ids_of.values():
        w.check(deep(ids), buf, row)
        w.check(rng.sample(deep(ids), GRID_Y * len(ids)), buf, row)
        w.check(rng.choices(ids, k=300), buf, row)


# ---- order and repetition (mh_eval_values_many sorts each variant's ids for the kernel) ---------
def order_cases(w):
    rng = random.Random(0x0DE5)
    n = w.n
    cases = {"reversed": list(reversed(range(n)))}
    for i in range(3):
        cases["shuffle%d" % i] = rng.sample(range(n), n)
    # [a, c, b] with a < b < c inside one variant, for every variant with three tapes, and the
    # same three where one workgroup walks them
    for v, ids in sorted(w.ids_of.items()):
        if len(ids) >= 3:
            a, b, c = ids[0], ids[len(ids) // 2], ids[-1]
            cases["triple_v%d" % v] = [a, c, b]
            cases["triple_deep_v%d" % v] = [a, c, b] + [a] * (3 * GRID_Y - 3)
    cases["twice"] = [t for t in range(n) for _ in (0, 1)]
    cases["twice_shuffled"] = rng.sample(cases["twice"], 2 * n)
    for t in (w.big[0], w.ids_of[11][0], w.ids_of[0][0], w.ids_of[6][-1]):
        cases["x130_t%d" % t] = [t] * 130
    # round-robin over the variants: no two neighbours of the list share a launch
    lists = [list(ids) for _, ids in sorted(w.ids_of.items())]
    inter = []
    while any(lists):
        for ids in lists:
            if ids:
                inter.append(ids.pop(rng.randrange(len(ids))))
    cases["interleaved"] = inter
    # every variant's whole bucket in one workgroup, the list handed over shuffled
    d = [t for _, ids in sorted(w.ids_of.items()) for t in deep(ids)]
    cases["deep_shuffled"] = rng.sample(d, len(d))
    return cases


def test_order_and_repetition(world):
    cases = order_cases(world)
    assert sorted(cases["interleaved"]) == list(range(world.n))
    for name, ids in cases.items():
        for buf, row in (FEW if len(ids) > 4 * world.n else KEYS):
            try:
                world.check(ids, buf, row)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e)) from None


# ---- lengths -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 129, 257, 300])
def test_lengths(world, n):
    """n ids of one variant (the largest of each register class), repeated where the variant has
    fewer: the odd/even pad of the result block, the 64-tape chunk edge, and grid y at its cap of
    256 with several ids per y-slice."""
    rng = random.Random(n)
    for cls in range(3):
        ids = max((ids for v, ids in world.ids_of.items() if v // 4 == cls), key=len)
        picks = rng.choices(ids, k=n) if n > len(ids) else rng.sample(ids, n)
        for buf, row in (("A", 64), ("B", 0)):
            world.check(picks, buf, row)
            world.check(sorted(picks), buf, row)


# ---- neighbours --------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [0, 1, 2])
def test_neighbours(world, cls):
    """A tape's value does not depend on what ran before or after it in the workgroup (stale
    registers, the prefetched window of the next tape, s_rb of a Bool / bit-vector neighbour):
    up to 8 tapes of one variant of the register class, every ordered pair and sampled triples as
    short lists, and -- a short list gives each id its own workgroup -- every pair and the
    triples again as the tapes ONE workgroup walks back to back (deep)."""
    w = world
    rng = random.Random(0x4E1 + cls)
    cands = [ids for v, ids in sorted(w.ids_of.items()) if v // 4 == cls and len(ids) >= 8]
    ids = max(cands, key=lambda ids: len({root_width(w.ts.tapes[t]) == 0 for t in ids}))
    small = [t for t in ids if w.info[t]["n_insns"] <= LDS_SLOTS]
    sub = sorted(rng.sample(small, 8))
    assert len({root_width(w.ts.tapes[t]) == 0 for t in sub}) == 2  # Bool and bit-vector roots
    triples = [rng.sample(sub, 3) for _ in range(24)]
    for buf, row in (("A", 63), ("B", 0)):
        for p in sub:
            for t in sub:
                w.check([p, t], buf, row)
        for tr in triples:
            w.check(tr, buf, row)
        for i, p in enumerate(sub):
            for t in sub[i + 1:]:
                w.check(deep([p, t]), buf, row)
        for tr in triples:
            w.check(deep(sorted(tr)), buf, row)
            w.check(deep(sorted(tr), 4), buf, row)  # after a repeat of the first tape


# ---- chunk cuts --------------------------------------------------------------------------------
def test_chunk_cuts(world):
    """One workgroup walks the contiguous tapes of a variant that end one tape before, at and one
    after the point where the running slot count passes the LDS chunk (2048 slots); and lists in
    which a tape larger than the chunk (streamed from memory) is first, in the middle and last."""
    w = world
    run, total, cut = w.cut, 0, None
    for i, t in enumerate(run):
        total += w.info[t]["n_insns"]
        if total > LDS_SLOTS:
            cut = i  # run[:cut + 1] is the first prefix over the chunk
            break
    assert cut is not None and 2 <= cut < CHUNK - 1
    lists = [run[:cut], run[:cut + 1], run[:cut + 2], run]
    ids = w.ids_of[w.variant[w.big[0]]]
    for big in w.big:
        i = ids.index(big)
        before, after = ids[max(0, i - 3):i], ids[i + 1:i + 4]
        after = [t for t in after if t not in w.big]
        before = [t for t in before if t not in w.big]
        assert before and after
        lists += [[big] + after, before + [big] + after, before + [big]]
    lists.append(sorted(set(w.big + ids[:2] + ids[-2:])))  # both streamed tapes in one walk
    for seq in lists:
        for buf, row in FEW:
            w.check(deep(seq), buf, row)
            w.check(deep(seq, len(seq) + 1), buf, row)


# ---- row windows of mh_eval_values -------------------------------------------------------------
WINDOWS = [(0, 1), (1, 63), (3, 64), (0, 65), (5, 257), (9, 4096), (7, 4097)]


def test_row_windows_of_eval_values(world, gpu_ctx):
    """(row_first, row_count) across the one-wave and 256-thread workgroup forms, partial last
    waves and row_first != 0: each window equals the same rows of the whole-buffer call, and the
    oracle on its first and last rows and a seeded sample of 100."""
    w = world
    rows = 4200
    soa = assignment_soa(random.Random(0x4200), N_COLS, rows)
    a = gpu_ctx.assignments(N_COLS, rows)
    try:
        a.upload(soa)
        tapes = []
        for v in (1, 7, 10):  # one per register class; keccak and EVM helpers among them
            tapes.append(next(t for t in w.ids_of[v] if 8 < w.info[t]["n_insns"] <= 512))
        memo = {}
        for t in tapes:
            whole = native.eval_values(gpu_ctx, w.ct, t, a)
            assert whole.shape == (8, rows)
            for first, count in WINDOWS:
                got = native.eval_values(gpu_ctx, w.ct, t, a, first, count)
                assert np.array_equal(got, whole[:, first:first + count]), (t, first, count)
                rng = random.Random(first * 10007 + count)
                pick = {0, count - 1} | set(rng.sample(range(count), min(count, 100)))
                ints = native.limbs_to_ints(got[:, sorted(pick)])
                for r, x in zip(sorted(pick), ints):
                    if (t, first + r) not in memo:
                        memo[t, first + r] = int(E.evaluate(w.ts.tapes[t].nodes, w.ts.pool.values,
                                                            soa_row(soa, first + r)))
                    assert x == memo[t, first + r], (t, first, count, r)
    finally:
        a.close()


# ---- refusals ----------------------------------------------------------------------------------
def test_refusals_before_any_launch(world, gpu_ctx):
    w = world
    a = w.buf["A"]
    other = native.Context(0)
    foreign = other.assignments(N_COLS, 70)
    try:
        before = native.eval_launches(gpu_ctx)

        def refused(ids, assign, row):
            with pytest.raises(native.SieveError) as e:
                native.eval_values_many(gpu_ctx, w.ct, ids, assign, row)
            assert e.value.code == native.MH_E_INVALID

        refused([0, w.n], a, 0)          # an id >= n_tapes
        refused([w.n + 7], a, 0)
        refused([0, 1], a, 70)           # a row >= capacity
        refused([0, 1], w.buf["B"], 1)
        refused([0, 1], foreign, 0)      # an assignment buffer of another context
        # n == 0 with null pointers is MH_OK
        assert gpu_ctx.lib.mh_eval_values_many(gpu_ctx.h, w.ct.h, None, 0, a.h, 0,
                                               None) == native.MH_OK
        assert native.eval_values_many(gpu_ctx, w.ct, [], a, 0).shape == (0, 8)
        assert native.eval_launches(gpu_ctx) == before
    finally:
        foreign.close()
        other.close()
    w.check([0, 1], "A", 0)  # and the context still serves
