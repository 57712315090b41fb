"""Tapes that need more live values than the interpreter has registers (tests/test_spill_host.py,
tests/test_gpu_spill.py, scripts/spill_cost.py).

``fan(k, chain)``: k values, each a chain of add / multiply steps over the columns x0, x1, all
live until they are combined twice: S = v_0 ^ .. ^ v_{k-1}, then t = the sum, over i from k - 1
down to 0, of v_i * (S + (i + 1)); the root is ULT(t, x0).  Every v_i is live from its definition
to its term of the sum, so the tape needs about k + 3 registers: k = 12 is the largest fan that
fits the 15 registers, k = 13 the smallest that spills.

``fuzz_tape(seed)``: a random DAG over every op class whose nodes are picked again as operands
long after they were made, so many values are live at once.
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np

from mythril_amd.tape import NODE_DTYPE, Op, Tape, TapeSet

M256 = (1 << 256) - 1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "mythril_amd", "csrc")
SPILL_EMU_LIB = os.path.join(NATIVE, "libmh_spill_emu.so")


def build_spill_emulator() -> str:
    """Build the host emulator that compiles with spilling (tests/native/spill_emu.cpp + the tape
    compiler), unless it is newer than its sources."""
    srcs = [os.path.join(NATIVE, "spill_emu.cpp"), os.path.join(CSRC, "compile.cpp")]
    deps = srcs + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(SPILL_EMU_LIB) and all(
            os.path.getmtime(SPILL_EMU_LIB) >= os.path.getmtime(d) for d in deps):
        return SPILL_EMU_LIB
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I/opt/rocm/include",
           "-o", SPILL_EMU_LIB] + srcs
    subprocess.run(cmd, check=True, capture_output=True)
    return SPILL_EMU_LIB


class SpillEmulator:
    """ctypes wrapper of tests/native/spill_emu.cpp: eval() and words() as tests/emu.py's
    Emulator has them, and spills(), the slots per tape."""

    def __init__(self, path=None):
        self.lib = C.CDLL(path or build_spill_emulator())

    @staticmethod
    def _flat(ts):
        nodes, offs, consts = ts.flatten()
        return (np.ascontiguousarray(nodes, dtype=NODE_DTYPE),
                np.ascontiguousarray(offs, dtype=np.uint64),
                np.ascontiguousarray(consts, dtype=np.uint32))

    def _call(self, name, ts, *tail):
        from tests.emu import EmuError

        nodes, offs, consts = self._flat(ts)
        err = C.create_string_buffer(512)
        f = getattr(self.lib, name)
        f.restype = C.c_int32
        r = f(C.c_void_p(nodes.ctypes.data), C.c_void_p(offs.ctypes.data), C.c_uint32(len(ts.tapes)),
              C.c_void_p(consts.ctypes.data), C.c_uint32(len(ts.pool.values)),
              C.c_uint32(ts.n_vars), *tail, err, C.c_int(512))
        if r != 0:
            raise EmuError(r, err.value.decode())

    def eval(self, ts, tape: int, soa_rows: np.ndarray):
        """soa_rows: [n_vars, 8, rows] u32.  Returns (list of root ints, n_regs)."""
        a = np.ascontiguousarray(soa_rows, dtype=np.uint32)
        rows = a.shape[2]
        out = np.zeros((8, rows), dtype=np.uint32)
        n_regs = C.c_uint32()
        self._call("spill_emu_eval", ts, C.c_uint32(tape), C.c_void_p(a.ctypes.data),
                   C.c_uint64(rows), C.c_void_p(out.ctypes.data), C.byref(n_regs))
        vals = [sum(int(out[k, j]) << (32 * k) for k in range(8)) for j in range(rows)]
        return vals, n_regs.value

    def words(self, ts) -> np.ndarray:
        cap = 1 << 21
        out = np.zeros(cap, dtype=np.uint32)
        nw = C.c_uint64()
        self._call("spill_emu_words", ts, C.c_void_p(out.ctypes.data), C.c_uint64(cap),
                   C.byref(nw))
        assert nw.value <= cap
        return out[:int(nw.value)].copy()

    def spills(self, ts) -> np.ndarray:
        out = np.zeros(max(len(ts.tapes), 1), dtype=np.uint32)
        self._call("spill_emu_tape_spills", ts, C.c_void_p(out.ctypes.data))
        return out[:len(ts.tapes)]


def fan_nodes(b, k: int, chain: int, var=None):
    """(t, root) node ids of the fan in builder ``b`` (columns x0, x1; ``var`` makes them,
    default ``b.var``)."""
    var = var or b.var
    x = [var("x0", 256), var("x1", 256)]
    vs = []
    for i in range(k):
        a = x[i % 2]
        for j in range(chain):
            a = b.op(Op.BVMUL, b.op(Op.BVADD, a, b.const(3 + 7 * i + j, 256)), x[(i + j) % 2])
        vs.append(a)
    s = vs[0]
    for v in vs[1:]:
        s = b.op(Op.BVXOR, s, v)
    t = None
    for i in reversed(range(k)):
        term = b.op(Op.BVMUL, vs[i], b.op(Op.BVADD, s, b.const(i + 1, 256)))
        t = term if t is None else b.op(Op.BVADD, t, term)
    return t, b.op(Op.BVULT, t, x[0])


def fan(k: int, chain: int = 1, value: bool = False) -> TapeSet:
    """The fan as a one-tape set; ``value``: the root is t itself (256 bits), not ULT(t, x0)."""
    ts = TapeSet(["x0", "x1"])
    b = ts.builder()
    t, root = fan_nodes(b, k, chain)
    ts.add(b.finish(t if value else root))
    return ts


def edge_rows(n_cols: int, n: int, seed: int):
    """n rows of n_cols 256-bit values: all zero, all ones, then random (some narrow)."""
    rng = random.Random(seed)
    rows = [[0] * n_cols, [M256] * n_cols]
    while len(rows) < n:
        rows.append([rng.getrandbits(rng.choice((256, 256, 256, 64, 8))) for _ in range(n_cols)])
    return rows[:n]


def soa(rows, n_cols: int) -> np.ndarray:
    out = np.zeros((max(n_cols, 1), 8, len(rows)), dtype=np.uint32)
    for j, row in enumerate(rows):
        for i, v in enumerate(row):
            for k in range(8):
                out[i, k, j] = (v >> (32 * k)) & 0xFFFFFFFF
    return out


_BIN = [Op.BVADD, Op.BVSUB, Op.BVMUL, Op.BVAND, Op.BVOR, Op.BVXOR]
_DIV = [Op.BVUDIV, Op.BVUREM, Op.BVSDIV, Op.BVSREM, Op.BVSMOD]
_SHIFT = [Op.BVSHL, Op.BVLSHR, Op.BVASHR]
_CMP = [Op.EQ, Op.BVULT, Op.BVULE, Op.BVUGT, Op.BVUGE, Op.BVSLT, Op.BVSLE, Op.BVSGT, Op.BVSGE]
_OVFL = [Op.BVADD_NOOVFL_U, Op.BVMUL_NOOVFL_U, Op.BVSUB_NOUDFL_U]


def fuzz_into(b, names, seed: int, n_ops: int, window: int, mix: bool = False):
    """A random DAG of about n_ops operations in builder ``b`` over the columns ``names``;
    operands come from the last ``window`` words made (a wide window keeps many values live) or,
    now and then, from anywhere.  Returns the Bool root: a chain of compares, mostly ANDs, so the
    short-circuit order applies too; ``mix``: that chain OR a compare about half of all rows
    satisfy, so uniform random rows run the whole tape and count some hits."""
    rng = random.Random(seed)
    words = [b.var(n, 256) for n in names]
    bools = []

    def word():
        if rng.random() < 0.15:
            return rng.choice(words)
        return rng.choice(words[-window:])

    def const():
        return b.const(rng.getrandbits(rng.choice((256, 64, 8, 3))), 256)

    for _ in range(n_ops):
        r = rng.random()
        x = word()
        y = const() if rng.random() < 0.25 else word()
        if r < 0.42:
            z = b.op(rng.choice(_BIN), x, y)
        elif r < 0.50:
            z = b.op(rng.choice(_DIV), x, y)
        elif r < 0.57:
            z = b.op(rng.choice(_SHIFT), x, y if rng.random() < 0.7 else
                     b.const(rng.randrange(0, 300), 256))
        elif r < 0.69:
            bools.append(b.op(rng.choice(_CMP), x, y))
            continue
        elif r < 0.74:
            bools.append(b.op(rng.choice(_OVFL), x, y))
            continue
        elif r < 0.84 and bools:
            z = b.op(Op.ITE, rng.choice(bools[-6:]), x, y)
        elif r < 0.87:
            z = b.op(Op.KECCAK, b.op(Op.CONCAT, x, y) if rng.random() < 0.5 else x)
        elif r < 0.94:
            lo = rng.randrange(0, 200)
            hi = rng.randrange(lo, 256)
            part = b.op(Op.EXTRACT, x, imm0=hi, imm1=lo)
            rest = b.op(Op.EXTRACT, y, imm0=255 - (hi - lo + 1), imm1=0) if hi - lo < 255 else None
            z = part if rest is None else b.op(Op.CONCAT, part, rest)
            if b.width(z) != 256:
                z = b.op(Op.ZEXT, z, imm0=256 - b.width(z))
        elif r < 0.97:
            z = b.op(Op.BVNOT if rng.random() < 0.5 else Op.BVNEG, x)
        else:
            z = b.op(rng.choice((Op.EVM_ADDMOD, Op.EVM_MULMOD)), x, y, word(),
                     imm0=rng.randrange(2))
        words.append(z)
    # fold what is left live into the conjuncts, so the whole DAG is reachable
    acc = words[-1]
    for w in words[-window:-1]:
        acc = b.op(Op.BVXOR, acc, w)
    bools.append(b.op(Op.BVULT, acc, b.const(M256 - (M256 >> 3), 256)))
    root = bools[0]
    for c in bools[1:]:
        root = b.op(Op.AND if rng.random() < 0.8 else Op.OR, root, c)
    if mix:
        root = b.op(Op.OR, root, b.op(Op.BVULT, acc, b.const(1 << 255, 256)))
    return root


def fuzz_params(seed: int):
    """(columns, operations, operand window) of fuzz tape ``seed``: two thirds of the seeds draw
    a window of 14..30 words, which alone exceeds the 15 registers less the pinned columns; the
    rest a window of 3..8, where the operands picked from anywhere (15 %) decide; 2..9 columns,
    so that tapes over more than four columns (D_LOADVAR, held columns) occur."""
    rng = random.Random(seed * 7919 + 13)
    n_cols = rng.randrange(2, 10)
    n_ops = rng.randrange(40, 240)
    window = rng.randrange(14, 31) if seed % 3 else rng.randrange(3, 9)
    return n_cols, n_ops, window


def fuzz_tape(seed: int) -> TapeSet:
    n_cols, n_ops, window = fuzz_params(seed)
    names = ["c%d" % i for i in range(n_cols)]
    ts = TapeSet(names)
    b = ts.builder()
    ts.add(b.finish(fuzz_into(b, names, seed, n_ops, window)))
    return ts


MIXED_COLUMNS = ["x0", "x1", "c2", "c3", "c4", "c5", "c6", "c7", "c8"]
# fuzz seeds of the mixed set below (each spills over four, six and nine columns)
MIXED_SEEDS = (2, 4, 5, 7, 8, 10, 11, 13, 14, 16, 17, 19, 20, 22, 23, 26)
# per column count of mixed_set: the tapes that fit the registers (tests/test_spill_host.py
# checks it on the host; over more than four columns no column is pinned, which leaves the
# fan k = 13 the registers it needs)
MIXED_FIT = {4: [], 6: [0], 9: [0]}


def mixed_set(n_cols: int = 4, plain: bool = False) -> TapeSet:
    """The GPU parity set: fans k = 13, 24, 40 (chain 1) and 16 fuzz tapes that spill, half of
    them with the ``mix`` root.  Over four columns every column is pinned in a register and all
    19 tapes spill; over six or nine (more than the pinned ones) every column is a D_LOADVAR.
    ``plain`` puts one more tape that does not spill (fan k = 5) in the middle."""
    names = MIXED_COLUMNS[:n_cols]
    ts = TapeSet(names)
    b = ts.builder()
    for k in (13, 24, 40):
        ts.add(b.finish(fan_nodes(b, k, 1)[1]))
    for i, seed in enumerate(MIXED_SEEDS):
        if plain and i == 5:
            ts.add(b.finish(fan_nodes(b, 5, 1)[1]))
        _, n_ops, window = fuzz_params(seed)
        ts.add(b.finish(fuzz_into(b, names, seed, n_ops, window, mix=i % 2 == 1)))
    return ts


# ---- the emitted code, word by word (tests/test_spill_host.py, scripts/spill_cost.py)
def _ops():
    """Op numbers of dev_isa.h's enum mh_dop."""
    import re
    text = open(os.path.join(CSRC, "dev_isa.h")).read()
    body = text[text.index("enum mh_dop"):]
    body = body[body.index("{") + 1:body.index("};")]
    body = re.sub(r"//[^\n]*", "", body)
    ops, nxt = {}, 0
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        if "=" in item:
            name, val = (x.strip() for x in item.split("="))
            nxt = ops[val] if val in ops else int(val, 0)
        else:
            name = item
        ops[name] = nxt
        nxt += 1
    return ops


OPS = _ops()
AUX_MAX = (1 << 14) - 1
WINDOW = 64


def _has_const(w1: int) -> bool:
    """Whether the instruction is followed by four slots of inline constant (exec.h step())."""
    op = w1 & 0xFF
    if op >= OPS["D_FIRST_COMPLEX"]:
        return bool(w1 >> 31)
    if OPS["D_ADD_RX"] <= op <= OPS["D_SGE_CX"]:
        op = OPS["D_ADD_R"] + (op - OPS["D_ADD_RX"])
    op = {OPS["D_MUL_RX"]: OPS["D_MUL_R"], OPS["D_MUL_CX"]: OPS["D_MUL_C"],
          OPS["D_LOADC_X"]: OPS["D_LOADC"]}.get(op, op)
    if OPS["D_ADD_R"] <= op <= OPS["D_SGE_C"]:
        return bool((op - OPS["D_ADD_R"]) & 1)
    if OPS["D_UDIV_R"] <= op <= OPS["D_SMOD_C"]:
        return bool((op - OPS["D_UDIV_R"]) & 1)
    return op in (OPS["D_MUL_C"], OPS["D_LOADC"])


def spill_ops(words):
    """[(slot index, op name, spill slot, w0)] of the D_SPILL / D_FILL of a one-tape word list,
    in tape order."""
    out, s = [], 0
    n = len(words) // 2
    while True:
        assert s < n, "tape ran past its slots"
        w0, w1 = int(words[2 * s]), int(words[2 * s + 1])
        op = w1 & 0xFF
        if op == OPS["D_END"]:
            return out
        if op == OPS["D_WINDOW"]:
            s = (s // WINDOW + 1) * WINDOW
            continue
        if op in (OPS["D_SPILL"], OPS["D_FILL"]):
            out.append((s, "D_SPILL" if op == OPS["D_SPILL"] else "D_FILL",
                        (w1 >> 17) & AUX_MAX, w0))
        s += 5 if _has_const(w1) else 1
