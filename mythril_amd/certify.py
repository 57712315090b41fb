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

from collections import OrderedDict
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
        ext = cls.from_tables(model, model.tables())
        ext._inverses(model, terms)
        return ext

    @classmethod
    def from_tables(cls, model, tabs: dict) -> "ExtModel":
        """from_model without the inverses, over ``model.tables()`` already answered (`tabs`)."""
        sc = model.schema
        ext = cls()
        for name, v in model.values.items():  # (a symbol only an index term reads is no column)
            c = sc.columns.get(name)
            if c is None or c.kind == "var":
                ext.scalars[name] = v
        sym = model.ctx.b.symbols
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
        return ext

    def _inverses(self, model, terms: Sequence[int]) -> None:
        asked = self._inverse_ask(model, terms)
        if asked is not None:
            ask = asked[3]
            vals = certify_values(model.sieve, model.ctx.b, ask, self) if ask else []
            self._inverse_answer(model, asked, vals)

    @staticmethod
    def _inverse_ask(model, terms: Sequence[int]):
        """None when the context has no keccak inverse; else (the inverses, forward function id
        -> inverse, the forward applications under `terms`, the terms whose values under this
        model ``_inverse_answer`` needs: each application's argument, then the application)."""
        b = model.ctx.b
        sym = b.symbols
        inv = [f for f in sym.functions if f.endswith("-1") and f[:-2] in sym.functions]
        if not inv:
            return None
        fwd_ids = {sym.functions[f[:-2]][0]: f for f in inv}
        apps = [n for n in _walk(b, terms, host_only=True)
                if b.nodes[n][0] == Op.UF and b.nodes[n][5] in fwd_ids]
        ask: List[int] = []
        for n in apps:
            ask += [b.nodes[n][2], n]
        return inv, fwd_ids, apps, ask

    def _inverse_answer(self, model, asked, vals: Sequence[int]) -> None:
        b = model.ctx.b
        inv, fwd_ids, apps, _ = asked
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
        # ... and every forward application the terms hold, at its argument's value
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


# ---- resident, batched certification -----------------------------------------------------------
CHUNK_ROOTS = 32    # constraints per chunk, in path order: the caching unit
CHUNK_CACHE = 256   # chunks a Certifier keeps compiled (least recently used closed first)


class _Chunk:
    """Up to CHUNK_ROOTS consecutive constraints of a path, compiled: the tape set of their
    ext-lowered roots (a term above 256 bits whole, with its slices), the tape set's own column
    list and its own local table numbering -- what certify_values builds per call, kept."""

    def __init__(self, b: TapeBuilder, ct, columns: List[str], table_ids: List[int],
                 spans: List[Tuple[int, int]], n_flat: int):
        self.b = b  # (held: the key's node ids are this builder's)
        self.ct = ct
        self.columns = columns
        self.table_ids = table_ids
        self.spans = spans
        self.n_flat = n_flat

    def close(self) -> None:
        if self.ct is not None:
            self.ct.close()
            self.ct = None


class Certifier:
    """certify() for many witnesses in one device pass, with the compiled constraints resident
    (one per Sieve: ``Sieve.certifier()``).

    A query's constraints are cut, in path order, into chunks of CHUNK_ROOTS; a chunk is compiled
    once and kept (an LRU of CHUNK_CACHE chunks), so a LASER child's certification finds every
    full chunk of its parent and compiles at most the last one.  One certification is one
    ``mh_values_job`` per chunk; N certifications are all their jobs in ceil(jobs / 256)
    submissions (native.eval_values_jobs), their rows in one upload of one grow-only buffer
    (job j reads row j, columns by the chunk's own positions) and their table sets in one
    native.tables_create_many.  ``certify`` / ``certify_values`` stay the checked reference: a
    verdict here equals theirs."""

    def __init__(self, sieve):
        self.sieve = sieve
        self.chunks: "OrderedDict[tuple, _Chunk]" = OrderedDict()
        self.assign = None
        # eval_values_jobs submissions: of the table build's asks, of the inverses' forward
        # applications, and of the constraints ("submissions")
        self.stats = {"chunk_compiles": 0, "chunk_hits": 0, "ask_submissions": 0,
                      "inverse_submissions": 0, "submissions": 0}

    def close(self) -> None:
        for c in self.chunks.values():
            c.close()
        self.chunks.clear()
        if self.assign is not None:
            self.assign.close()
            self.assign = None

    # -- chunks ------------------------------------------------------------------------------
    def _chunk(self, b: TapeBuilder, roots: Sequence[int]) -> _Chunk:
        from .model import Slicer
        from .sieve import local_tapeset

        key = (id(b),) + tuple(roots)
        got = self.chunks.get(key)
        if got is not None and got.b is b:
            self.chunks.move_to_end(key)
            self.stats["chunk_hits"] += 1
            return got
        flat: List[int] = []
        spans = []
        try:
            for r in roots:
                sl = [r] if b.widths[r] <= SLICE else Slicer(b).slices(r)
                spans.append((len(flat), len(sl)))
                flat.extend(sl)
        except CertifyUnsupported:
            raise
        except TapeError as e:
            raise CertifyUnsupported(str(e)) from e
        columns = _columns(b, flat)
        ts = local_tapeset(b, flat, columns)
        table_ids = _local_tables(b, ts, flat)
        ct = self.sieve.compile(ts)
        self.stats["chunk_compiles"] += 1
        if got is not None:
            got.close()
        c = self.chunks[key] = _Chunk(b, ct, columns, table_ids, spans, len(flat))
        self.chunks.move_to_end(key)
        return c

    def _chunks_of(self, b: TapeBuilder, nodes: Sequence[int]) -> List[_Chunk]:
        roots = [ext_lower(b, n) for n in nodes]
        return [self._chunk(b, roots[lo:lo + CHUNK_ROOTS])
                for lo in range(0, len(roots), CHUNK_ROOTS)]

    def _evict(self) -> None:
        while len(self.chunks) > CHUNK_CACHE:
            _, c = self.chunks.popitem(last=False)
            c.close()

    def _buffer(self, n_cols: int, rows: int):
        a = self.assign
        if a is None or a.n_vars < n_cols or a.capacity < rows:
            n_cols = max(n_cols, a.n_vars if a is not None else 0)
            rows = max(rows, a.capacity if a is not None else 0, 16)
            if a is not None:
                a.close()
            self.assign = a = self.sieve.ctx.assignments(n_cols, 1 << (rows - 1).bit_length())
        return a

    # -- API ---------------------------------------------------------------------------------
    def certify_many(self, models: Sequence, terms_list: Sequence[Sequence],
                     exts: Optional[Sequence[Optional[ExtModel]]] = None) -> list:
        """Entry i: the Verdict ``certify(models[i], terms_list[i])`` gives (the failing indices
        match; an ``ext.rejected`` model gives its rejection verdict), or the CertifyUnsupported
        / native.Unsupported instance when that one model cannot be judged.  A device or ABI
        error raises for the whole call.  ``exts[i]``, when given, is certify()'s ``ext``."""
        out: list = [None] * len(models)
        nodes_of: list = [None] * len(models)
        ext_of: list = [None] * len(models)
        unjudged = (CertifyUnsupported, native.Unsupported)
        try:
            # 1. the table build's ask: every model's read-index terms in one table-free submission
            asks = []
            for i, (model, terms) in enumerate(zip(models, terms_list)):
                try:
                    nodes_of[i] = _nodes(terms)
                    if exts is not None and exts[i] is not None:
                        ext_of[i] = exts[i]
                        continue
                    parts, keys = model.tables_ask()
                    res, prep = model._evaluate_prepare(keys, [], True) if keys else ({}, None)
                    asks.append((i, parts, res, prep))
                except unjudged as e:
                    out[i] = e
            tabs = self._ask(models, asks, out)
            # 2. the inverses: the forward keccak applications of every model that has an inverse
            # in a second submission, made only when some model has one
            inverse = []  # (i, ext, chunks, asked)
            for i, _, _, _ in asks:
                if out[i] is not None:
                    continue
                try:
                    ext = ExtModel.from_tables(models[i], tabs[i])
                    asked = ExtModel._inverse_ask(models[i], nodes_of[i])
                    if asked is None:
                        ext_of[i] = ext
                    elif not asked[3]:
                        ext._inverse_answer(models[i], asked, [])
                        ext_of[i] = ext
                    else:
                        inverse.append((i, ext, self._chunks_of(models[i].ctx.b, asked[3]), asked))
                except unjudged as e:
                    out[i] = e
            if inverse:
                vals = self._term_values([(i, ext, chunks) for i, ext, chunks, _ in inverse],
                                         "inverse_submissions")
                for (i, ext, _, asked), v in zip(inverse, vals):
                    ext._inverse_answer(models[i], asked, v)
                    ext_of[i] = ext
            # 3. the constraints
            plans = []  # (i, ext, chunks)
            for i, model in enumerate(models):
                if out[i] is not None:
                    continue
                try:
                    ext, nodes = ext_of[i], nodes_of[i]
                    if ext.rejected:
                        out[i] = Verdict(False, (), ext.rejected)
                        continue
                    b = model.ctx.b
                    if any(b.widths[n] != BOOL for n in nodes):
                        raise CertifyUnsupported("certify takes Bool constraints")
                    if not nodes:
                        out[i] = Verdict(True)
                        continue
                    plans.append((i, ext, self._chunks_of(b, nodes)))
                except unjudged as e:
                    out[i] = e
            if plans:
                for (i, _, _), flat in zip(plans, self._term_values(plans, "submissions")):
                    failing = [k for k, v in enumerate(flat) if not v]
                    out[i] = Verdict(not failing, failing)
        finally:
            self._evict()
        return out

    def _ask(self, models, asks, out) -> Dict[int, dict]:
        """``Model.tables()`` of every asking model, {model index: tables}: the lowered index
        terms of all of them as table-free jobs of one submission (what Model._evaluate sends
        through Sieve.eval_terms one model at a time).  A model whose terms do not compile gets
        its exception in `out`."""
        from .sieve import _limbs, local_tapeset

        jobs = []  # (i, compiled tapes, columns, terms)
        try:
            for i, _, _, prep in asks:
                if prep is None:
                    continue
                _, flat, columns = prep
                try:
                    ct = self.sieve.compile(local_tapeset(models[i].ctx.b, flat, columns))
                except native.Unsupported as e:
                    out[i] = e
                    continue
                jobs.append((i, ct, columns, len(flat)))
            vals: Dict[int, List[int]] = {}
            if jobs:
                assign = self._buffer(max(len(c) for _, _, c, _ in jobs), len(jobs))
                soa = np.zeros((assign.n_vars, 8, len(jobs)), dtype=np.uint32)
                for j, (i, _, columns, _) in enumerate(jobs):
                    values = models[i].values
                    for p, name in enumerate(columns):
                        v = values.get(name, 0)
                        if v:
                            soa[p, :, j] = [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]
                assign.upload(soa)
                got = native.eval_values_jobs(
                    self.sieve.ctx, [(ct, None, list(range(n)), assign, j)
                                     for j, (_, ct, _, n) in enumerate(jobs)])
                self.stats["ask_submissions"] += -(-len(jobs) // native.VALUES_JOBS_MAX)
                for (i, _, _, n), o in zip(jobs, got):
                    vals[i] = [_limbs(o[t]) for t in range(n)]
        finally:
            for _, ct, _, _ in jobs:
                ct.close()
        tabs = {}
        for i, parts, res, prep in asks:
            if out[i] is not None:
                continue
            at = res if prep is None else models[i]._evaluate_finish(res, prep[0], vals[i])
            tabs[i] = models[i].tables_answer(parts, at)
        return tabs

    def _term_values(self, plans, counter: str) -> List[List[int]]:
        """Per plan (model index, ext, chunks) the values of its chunks' terms, in order."""
        vals = self._run([(i, ext, c) for i, ext, chunks in plans for c in chunks], counter)
        out, at = [], 0
        for _, _, chunks in plans:
            flat: List[int] = []
            for c in chunks:
                v = vals[at]
                at += 1
                flat += [sum(v[s + j] << (SLICE * j) for j in range(k)) for s, k in c.spans]
            out.append(flat)
        return out

    def certify(self, model, terms, ext: Optional[ExtModel] = None) -> Verdict:
        """certify(model, terms, ext) through the resident chunks: one model, one submission."""
        got = self.certify_many([model], [terms], None if ext is None else [ext])[0]
        if isinstance(got, Exception):
            raise got
        return got

    def _run(self, jobs, counter: str) -> List[List[int]]:
        """Per job (model index, ext, chunk) the values of the chunk's tapes: every job's row in
        one upload, every table set in one allocation, the jobs in ceil(jobs / 256) submissions."""
        sieve = self.sieve
        assign = self._buffer(max(len(c.columns) for _, _, c in jobs), len(jobs))
        soa = np.zeros((assign.n_vars, 8, len(jobs)), dtype=np.uint32)
        rows: Dict[int, Dict[str, int]] = {}
        sets, set_of = [], []
        for j, (i, ext, c) in enumerate(jobs):
            row = rows.get(i)
            if row is None:
                row = rows[i] = ext.row()
            for p, name in enumerate(c.columns):
                v = row.get(name, 0)
                if v:
                    soa[p, :, j] = [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]
            if c.table_ids:
                set_of.append(len(sets))
                sets.append(ext.tables(c.b, c.table_ids))
            else:
                set_of.append(None)  # no lookup in the chunk: a table-free job
        assign.upload(soa)
        tables = native.tables_create_many(sieve.ctx, sets) if sets else []
        try:
            out = native.eval_values_jobs(
                sieve.ctx, [(c.ct, None if set_of[j] is None else tables[set_of[j]],
                             list(range(c.n_flat)), assign, j)
                            for j, (_, _, c) in enumerate(jobs)])
            self.stats[counter] += -(-len(jobs) // native.VALUES_JOBS_MAX)
        finally:
            for t in tables:
                t.close()
        return [[sum(int(o[t, k]) << (32 * k) for k in range(8)) for t in range(len(o))]
                for o in out]


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
