"""Certification of sieve witnesses against the ORIGINAL constraints.

A sieve witness is a row of the lowered query's columns (lower.py, csrc/query.cpp).  The
congruence, cell and injectivity conjuncts that make such a row a model are conjuncts of the
lowered *query*, not part of any term's *value*: a row that violates one the lowering dropped
still evaluates every stated constraint to true through ``Model.eval_many``, which lowers the
term again with the same lowering and the same frozen schema.

This module evaluates the un-lowered terms under the EXTENSIONAL meaning of the model instead —
the concrete tables ``Model[decl]`` shows a caller and ``plugin.witness_pins`` pins for z3:
arrays are (finite table, else value), functions are tables with a default rule, and ``select``
is a lookup by the *value* of its index.  What ``oracle/term_eval.py`` computes on the CPU, on the
device: a term becomes a device term that depends on the term only (``ext_lower``: stores become
``ite``, ``K(v)`` becomes ``v``, a select of a free array and a function application become
``Op.LOOKUP`` of a table id), the model becomes one table set (``native.Tables``) and one row,
and every constraint is a tape of its own, so a LASER child query reuses its parent's compiled
tapes (the ctx's by-content tape cache) and only the tables and the row change per witness.

Nothing here imports ``lower.Lowering`` or reaches csrc/query.cpp: independence from the lowering
and the guide is the point.  The evaluator (the interpreter's ops) is shared with the search; the
oracle parity suite pins it.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import native
from .lower import (KECCAK_ALIGN, KECCAK_SHIFT, _memo, _walk, is_keccak,
                    node_columns, var_names)
from .tape import ARITY, BOOL, F_ARRAY, F_HOST, Op, TapeBuilder, TapeError

SLICE = 256
M256 = (1 << 256) - 1


class CertifyUnsupported(TapeError):
    """The term uses an array / function construct the certifier does not model (what lower.py
    refuses, or a lookup key above 768 bits): the witness stays uncertified."""


@dataclass(frozen=True)
class KeccakRule:
    """A function's default outside its table: ``H(x) = base + ((keccak256(x) >> 139) << 6)``
    (lower.py: what a lowered keccak application evaluates to away from the stated pairs)."""

    base: int = 0


class Verdict(int):
    """certify()'s answer: truthy when every constraint holds.  ``failing`` lists the indices of
    the constraints that do not; ``reason`` says why a model was rejected before evaluation."""

    failing: Tuple[int, ...] = ()
    reason: str = ""

    def __new__(cls, ok: bool, failing: Sequence[int] = (), reason: str = ""):
        v = super().__new__(cls, 1 if ok else 0)
        v.failing = tuple(failing)
        v.reason = reason
        return v

    def __repr__(self) -> str:
        return "Verdict(%s, failing=%r%s)" % (bool(self), list(self.failing),
                                              ", %s" % self.reason if self.reason else "")


TABLES_PER_SYMBOL = 8  # 256-bit slices of a symbol's range (tape.MAX_WIDTH = 1088 bits: 5)


def array_table(aid: int) -> int:
    """The first table id of array symbol `aid` (slice j of its range is table id + j): ids
    depend on the symbol only, so a lowered term names the same tables under every model."""
    return 2 * TABLES_PER_SYMBOL * aid


def function_table(fid: int) -> int:
    return 2 * TABLES_PER_SYMBOL * fid + TABLES_PER_SYMBOL


def _slices(width: int) -> List[Tuple[int, int]]:
    """(low bit, bits) of the 256-bit slices of a `width`-bit range."""
    return [(lo, min(SLICE, width - lo)) for lo in range(0, width, SLICE)]


def base_column(fname: str) -> str:
    """The column holding a keccak function's interval base (KeccakRule.base)."""
    return "%s[H]" % fname


def rule_column(fname: str) -> str:
    """The 1-bit column that says whether `fname` misses to the keccak rule (1) or to the
    table's else value (0)."""
    return "%s[H?]" % fname


@dataclass
class ExtModel:
    """An extensional model, plain data:

    scalars    {name: int}                          a missing name reads 0
    arrays     {name: ({key: value}, else value)}   a missing array reads 0 everywhere
    functions  {name: ({arg: value}, default)}      default: an int or a KeccakRule
    """

    scalars: Dict[str, int] = field(default_factory=dict)
    arrays: Dict[str, Tuple[dict, int]] = field(default_factory=dict)
    functions: Dict[str, Tuple[dict, Union[int, KeccakRule]]] = field(default_factory=dict)
    rejected: str = ""  # from_model: why the Model denotes no model at all (injectivity)

    # -- what the device is given ---------------------------------------------------------
    def row(self) -> Dict[str, int]:
        """Column values: the scalars plus each function's rule columns."""
        row = dict(self.scalars)
        for f, (_, dflt) in self.functions.items():
            if isinstance(dflt, KeccakRule):
                row[base_column(f)] = dflt.base & M256
                row[rule_column(f)] = 1
        return row

    def tables(self, b: TapeBuilder, ids: Sequence[int]) -> List[Tuple[dict, int, int]]:
        """[(table, else value, key bits)] of the tables `ids` (array_table / function_table ids
        plus the slice), in that order: only what the tapes at hand look up is ever packed, so a
        symbol the session declared elsewhere costs nothing and cannot fail the upload."""
        sym = b.symbols
        out: List[Tuple[dict, int, int]] = []
        for tid in ids:
            s, j = divmod(tid, TABLES_PER_SYMBOL)
            if s % 2 == 0:
                name = sym.array_names[s // 2]
                _, dom, rng = sym.arrays[name]
                tab, els = self.arrays.get(name, ({}, 0))
            else:
                name = sym.function_names[s // 2]
                _, dom, rng = sym.functions[name]
                tab, els = self.functions.get(name, ({}, 0))
                if isinstance(els, KeccakRule):
                    els = 0
            lo, sw = _slices(rng)[j]  # a range above 256 bits: one table per slice
            m = (1 << sw) - 1
            out.append(({k: (v >> lo) & m for k, v in tab.items()}, (els >> lo) & m, dom))
        return out

    # -- from a sieve Model ---------------------------------------------------------------
    @classmethod
    def from_model(cls, model, terms: Sequence[int] = ()) -> "ExtModel":
        """The interpretation `model` (model.Model) documents and shows its callers: scalars from
        its variable columns; arrays and tabled functions from ``Model.tables`` (one device batch
        for every symbol's read indices); a keccak function as its stated pairs over its kread
        applications, missing to ``H``; an inverse ``keccak256_N-1`` as the forward table
        reversed, extended by value -> argument for every forward application under `terms`.
        Two arguments with one image leave ``rejected`` set: the row denotes no model."""
        sc = model.schema
        ext = cls()
        for name, v in model.values.items():  # (a symbol only an index term reads is no column)
            c = sc.columns.get(name)
            if c is None or c.kind == "var":
                ext.scalars[name] = v
        sym = model.ctx.b.symbols
        tabs = model.tables()
        for name, got in tabs.items():
            if name in sc.keccak or got is None:
                continue
            if name in sym.arrays:
                ext.arrays[name] = (dict(got[0]), got[1])
            else:
                ext.functions[name] = (dict(got[0]), got[1])
        for f, km in sc.keccak.items():
            tab = dict(tabs[f][0]) if tabs.get(f) is not None else {}
            tab.update(km.pairs)
            ext.functions[f] = (tab, KeccakRule(km.base))
        ext._inverses(model, terms)
        return ext

    def _inverses(self, model, terms: Sequence[int]) -> None:
        b = model.ctx.b
        sym = b.symbols
        inv = [f for f in sym.functions if f.endswith("-1") and f[:-2] in sym.functions]
        if not inv:
            return
        fwd_ids = {sym.functions[f[:-2]][0]: f for f in inv}
        apps = [n for n in _walk(b, terms, host_only=True)
                if b.nodes[n][0] == Op.UF and b.nodes[n][5] in fwd_ids]
        pairs: Dict[str, Dict[int, int]] = {f: {} for f in inv}
        clash = ""

        def put(f, value, arg):
            nonlocal clash
            old = pairs[f].setdefault(value, arg)
            if old != arg and not clash:
                clash = "%s maps %#x and %#x to %#x" % (f[:-2], old, arg, value)

        for f in inv:  # the forward table reversed
            for arg, value in self.functions.get(f[:-2], ({}, 0))[0].items():
                put(f, value, arg)
        if apps:  # ... and every forward application the terms hold, at its argument's value
            ask: List[int] = []
            for n in apps:
                ask += [b.nodes[n][2], n]
            vals = certify_values(model.sieve, b, ask, self)
            for i, n in enumerate(apps):
                put(fwd_ids[b.nodes[n][5]], vals[2 * i + 1], vals[2 * i])
        for f in inv:
            self.functions[f] = (pairs[f], 0)
        self.rejected = clash


# ---- extensional lowering ----------------------------------------------------------------------
def _eq(b: TapeBuilder, x: int, y: int) -> int:
    """x == y for lowered bit-vector terms of any width (above 256 bits: slice by slice)."""
    from .model import Slicer

    if b.widths[x] <= SLICE:
        return b.op(Op.EQ, x, y)
    sl = Slicer(b)
    acc = None
    for p, q in zip(sl.slices(x), sl.slices(y)):
        e = b.op(Op.EQ, p, q)
        acc = e if acc is None else b.op(Op.AND, acc, e)
    return acc


def _lookup(b: TapeBuilder, first: int, key: int, width: int) -> int:
    """The `width`-bit value of the symbol whose tables start at id `first`, at `key`: one lookup
    per 256-bit slice of the range, concatenated."""
    acc = None
    for j, (_, sw) in enumerate(_slices(width)):
        part = b.lookup(first + j, key, sw)
        acc = part if acc is None else b.op(Op.CONCAT, part, acc)
    return acc


def _select(b: TapeBuilder, memo: Dict[int, int], arr: int, idx: int) -> int:
    """select(arr, idx) with `idx` lowered: the store chain as ite over its keys, down to a
    lookup of the free array's table or K's value."""
    chain = []
    nodes = b.nodes
    while nodes[arr][0] == Op.STORE:
        chain.append(arr)
        arr = nodes[arr][2]
    op, w, a, _, _, i0, _ = nodes[arr]
    if op == Op.ARRAY:
        acc = _lookup(b, array_table(i0), idx, w)
    elif op == Op.CONST_ARRAY:
        acc = memo.get(a, a)
    else:
        raise CertifyUnsupported("array term %s is not a store chain" % Op(op).name)
    for st in reversed(chain):
        k, v = nodes[st][3], nodes[st][4]
        acc = b.op(Op.ITE, _eq(b, idx, memo.get(k, k)), memo.get(v, v), acc)
    return acc


def _apply(b: TapeBuilder, fid: int, x: int, w: int) -> int:
    """f(x) with `x` lowered: the function's table; a keccak function (256-bit range, whole
    bytes in) misses to H when the row's rule column says so."""
    name = b.symbols.function_names[fid]
    tid = function_table(fid)
    val = _lookup(b, tid, x, w)
    if not (is_keccak(name) and w == 256 and b.widths[x] % 8 == 0):
        return val
    h = b.op(Op.KECCAK, x)
    h = b.op(Op.BVLSHR, h, b.const(KECCAK_SHIFT, 256))
    h = b.op(Op.BVSHL, h, b.const(KECCAK_ALIGN, 256))
    h = b.op(Op.BVADD, h, b.var(base_column(name), 256))
    rule = b.op(Op.EQ, b.var(rule_column(name), 1), b.const(1, 1))
    miss = b.op(Op.AND, rule, b.op(Op.NOT, b.lookup(tid, x, w, hit=True)))
    return b.op(Op.ITE, miss, h, val)


def ext_lower(b: TapeBuilder, node: int) -> int:
    """The extensional device term of `node`: no array, store, select or function application is
    left; it depends on the term alone (never on a witness) and is memoised per node on the
    builder."""
    memo: Dict[int, int] = _memo(b, "_ext_lowered")
    got = memo.get(node)
    if got is not None:
        return got
    nodes, flags = b.nodes, b.flags
    if not flags[node] & F_HOST:
        if flags[node] & F_ARRAY:
            raise CertifyUnsupported("array-sorted term used as a value")
        return node
    try:
        for n in _walk(b, [node], host_only=True):
            if n in memo:
                continue
            op, w, a, bb, c, i0, i1 = nodes[n]
            if flags[n] & F_ARRAY:
                if op not in (Op.ARRAY, Op.CONST_ARRAY, Op.STORE):
                    raise CertifyUnsupported("%s over arrays" % Op(op).name)
                continue  # read through _select
            if op == Op.SELECT:
                memo[n] = _select(b, memo, a, memo.get(bb, bb))
                continue
            if op == Op.UF:
                memo[n] = _apply(b, i0, memo.get(a, a), w)
                continue
            kids = (a, bb, c)[:ARITY[op]]
            if any(flags[x] & F_ARRAY for x in kids):
                raise CertifyUnsupported("%s over arrays" % Op(op).name)
            low = [memo.get(x, x) for x in kids]
            if op == Op.EQ and b.widths[a] > SLICE:
                memo[n] = _eq(b, low[0], low[1])
            elif low == list(kids):
                memo[n] = n
            else:
                memo[n] = b.op(Op(op), *low, imm0=i0, imm1=i1)
    except CertifyUnsupported:
        raise
    except TapeError as e:  # a key above 768 bits, a wide operator the Slicer does not cut
        raise CertifyUnsupported(str(e)) from e
    return memo[node]


# ---- evaluation --------------------------------------------------------------------------------
PAD_COLUMNS = 64  # a certification tape set's column count is padded to a power of two from here,
                  # so a child query's new columns leave its parent's tapes' cache keys alone


def _columns(b: TapeBuilder, roots: Sequence[int]) -> List[str]:
    cols = node_columns(b, roots)
    names = var_names(b)
    used = sorted({v for r in roots for v in cols[r]})  # creation order: a parent's stay first
    out = [names[v] for v in used]
    n = PAD_COLUMNS
    while n < len(out):
        n *= 2
    return out + ["__pad%d" % i for i in range(n - len(out))]


def _table_refs(b: TapeBuilder, root: int) -> Tuple[int, ...]:
    """The table ids the lowered term `root` looks up, in the order a walk meets them (memoised
    per root on the builder: a child query walks only its new conjuncts)."""
    memo: Dict[int, Tuple[int, ...]] = _memo(b, "_ext_table_refs")
    got = memo.get(root)
    if got is None:
        nodes = b.nodes
        got = memo[root] = tuple(dict.fromkeys(
            nodes[n][5] for n in _walk(b, [root]) if nodes[n][0] == Op.LOOKUP))
    return got


def _local_tables(b: TapeBuilder, ts, flat: Sequence[int]) -> List[int]:
    """Renumber the tapes' lookups to the tables they use, 0.. in order of first use over the
    tapes (a parent query's conjuncts come first, so a child's tapes of them keep their words),
    and return those tables' ids."""
    ids = list(dict.fromkeys(t for r in flat for t in _table_refs(b, r)))
    local = {t: i for i, t in enumerate(ids)}
    for tape in ts.tapes:
        is_lk = tape.nodes["op"] == int(Op.LOOKUP)
        if is_lk.any():
            tape.nodes["imm0"][is_lk] = [local[int(t)] for t in tape.nodes["imm0"][is_lk]]
    return ids


def certify_values(sieve, b: TapeBuilder, terms: Sequence[int], ext: ExtModel) -> List[int]:
    """The values of `terms` (nodes of `b`, un-lowered) under `ext`, evaluated on the device:
    one tape per term, one table upload, one launch per register class.  Bool terms give 0 / 1."""
    from .model import Slicer
    from .sieve import local_tapeset

    if not terms:
        return []
    flat: List[int] = []
    spans = []
    try:
        for t in terms:
            r = ext_lower(b, t)
            if b.widths[r] <= SLICE:
                spans.append((len(flat), 1))
                flat.append(r)
            else:
                sl = Slicer(b).slices(r)
                spans.append((len(flat), len(sl)))
                flat.extend(sl)
    except CertifyUnsupported:
        raise
    except TapeError as e:
        raise CertifyUnsupported(str(e)) from e
    columns = _columns(b, flat)
    row = ext.row()
    ts = local_tapeset(b, flat, columns)
    table_ids = _local_tables(b, ts, flat)
    ct = sieve.compile(ts)
    assign = tables = None
    try:
        assign = sieve.ctx.assignments(len(columns), 1)
        soa = np.zeros((len(columns), 8, 1), dtype=np.uint32)
        for i, c in enumerate(columns):
            v = row.get(c, 0)
            if v:
                soa[i, :, 0] = [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]
        assign.upload(soa)
        tables = native.tables_create(sieve.ctx, ext.tables(b, table_ids))
        out = native.eval_values_tables(sieve.ctx, ct, tables, list(range(len(flat))), assign, 0, 1)
    finally:
        if tables is not None:
            tables.close()
        if assign is not None:
            assign.close()
        ct.close()
    vals = [sum(int(out[i, k, 0]) << (32 * k) for k in range(8)) for i in range(len(flat))]
    return [sum(vals[at + j] << (SLICE * j) for j in range(k)) for at, k in spans]


def _nodes(terms) -> List[int]:
    return [t if isinstance(t, int) else t.node for t in terms]


def certify(model, terms, ext: Optional[ExtModel] = None) -> Verdict:
    """Does `model` (a sieve Model, or the ExtModel given) satisfy every constraint of `terms`
    (Bool terms of the model's context, or their nodes) as they are stated?  Raises
    CertifyUnsupported for a term outside what the certifier models."""
    nodes = _nodes(terms)
    if ext is None:
        ext = ExtModel.from_model(model, nodes)
    if ext.rejected:
        return Verdict(False, (), ext.rejected)
    b = model.ctx.b
    if any(b.widths[n] != BOOL for n in nodes):
        raise CertifyUnsupported("certify takes Bool constraints")
    vals = certify_values(model.sieve, b, nodes, ext)
    failing = [i for i, v in enumerate(vals) if not v]
    return Verdict(not failing, failing)
