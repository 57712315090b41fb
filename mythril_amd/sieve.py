"""The sieve engine behind ``get_model``: one path condition -> a witness, or nothing.

For one query (the tuple of Bool constraints ``Constraints.is_possible`` hands to ``get_model``,
mythril/laser/ethereum/state/constraints.py:25-35, support/model.py:15-62):

1. lower arrays / keccak UFs onto scalar columns, split the conjuncts into column-disjoint groups
   and linearise the tapes -- in one native call (mh_query_build, csrc/query.cpp; the Python
   stages lower.py / buckets / local_tapeset are its reference and the definitions path);
   unsupported constructs -> the fallback, a self-contradicting query -> no device round;
2. harvest a candidate guide from the lowered term and the parent query's witness
   (mh_guide_harvest_with, harvest.cpp -- the algorithm of candidates.py, same arrays; the
   session reuses the inversions of the path's earlier queries); the guide stays in the library;
3. compile the group tapes over the query's own columns (mh_tapes_compile; tapes compiled
   before in this context, a LASER parent's unchanged groups, come from its cache);
4. two rounds at most, each ONE call (mh_query_round: guided generator, MH_MODE_FIRST_HIT run,
   and the witness rows, one host sync): ``first_rows`` guided rows, then, when a group is still
   unsolved, the remaining ``(max_rounds - 1) * rows`` rows over the unsolved groups' tapes;
5. on a hit, the witness (column name -> value) from the row that came back with the results.

Everything on the device path raises on failure; the caller (frontend.get_model) treats any
exception as "no answer from the sieve" and asks the fallback solver, so the reference's
behaviour is kept on every error (SURVEY.md §5 "fail closed").
"""
from __future__ import annotations

import os
import re
import threading
import time
from collections import OrderedDict
from copy import deepcopy
from dataclasses import dataclass, field
from typing import Callable, Dict, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import decide, native
from .lower import (Column, KeccakMap, Lowering, LoweringUnsupported, Schema, cell_name,
                    lower_query, node_columns)
from .tape import ARITY, NODE_DTYPE, Op, Tape, TapeBuilder, TapeError, TapeSet


@dataclass
class Witness:
    schema: Schema
    values: Dict[str, int]             # column name -> value
    index: int = 0                     # global candidate index that satisfied the query
    rounds: int = 0
    repaired: bool = False             # a group's row came from the repair step (Sieve._repair)
    # further models of the query found beside it (Sieve(spares=K)): the query's columns only
    spares: List[Dict[str, int]] = field(default_factory=list)


@dataclass
class SieveStats:
    queries: int = 0
    hits: int = 0
    misses: int = 0
    unsupported: int = 0
    errors: int = 0
    rounds: int = 0
    rows: int = 0
    host_s: float = 0.0
    device_s: float = 0.0
    extra: Dict[str, int] = field(default_factory=dict)
    # seconds per stage: lower, guide, tapes, compile, generate, run, download
    stage_s: Dict[str, float] = field(default_factory=dict)

    def add(self, stage: str, dt: float) -> None:
        self.stage_s[stage] = self.stage_s.get(stage, 0.0) + dt

    def bump(self, name: str, n: int = 1) -> None:
        """Count `n` more of `extra[name]` (the key appears with its first bump, even of 0)."""
        self.extra[name] = self.extra.get(name, 0) + n


def local_tape(b: TapeBuilder, root: int, columns: Sequence[str]) -> np.ndarray:
    """The tape of `root` with VAR columns renumbered to the query's own column order."""
    tape = b.finish(root)
    nodes = tape.nodes.copy()
    local = {b.var_index[c]: i for i, c in enumerate(columns)}
    is_var = nodes["op"] == int(Op.VAR)
    if is_var.any():
        nodes["imm0"][is_var] = [local[int(x)] for x in nodes["imm0"][is_var]]
    return nodes


class LocalPool:
    """The constants one query's tapes read, renumbered 0..k-1 (the builder's pool holds every
    constant of the run: uploading it with each query would grow with the run)."""

    def __init__(self, rows: np.ndarray):
        self.rows = rows
        self.values = range(len(rows))

    def to_array(self) -> np.ndarray:
        return self.rows


def local_tapeset(b: TapeBuilder, roots: Sequence[int], columns: Sequence[str]) -> TapeSet:
    """One tape per root over the query's own columns (VAR renumbered to `columns` order) and
    its own constant pool (CONST renumbered to the constants the tapes read)."""
    ts = TapeSet(columns)
    tapes = [b.finish(r).nodes for r in roots]
    nodes = np.concatenate(tapes) if tapes else np.zeros(0, dtype=NODE_DTYPE)
    ops, imm0 = nodes["op"], nodes["imm0"].astype(np.int64)
    is_var = ops == int(Op.VAR)
    is_const = ops == int(Op.CONST)
    new0 = imm0.copy()
    if is_var.any():
        lut = np.full(len(b.var_index), -1, dtype=np.int64)
        vi = b.var_index
        for i, c in enumerate(columns):
            v = vi.get(c)  # a column no builder term reads (a native query's cell) maps nothing
            if v is not None:
                lut[v] = i
        new0[is_var] = lut[imm0[is_var]]
        if (new0[is_var] < 0).any():
            raise ValueError("a tape reads a variable outside the query's columns")
    used = np.unique(imm0[is_const])
    new0[is_const] = np.searchsorted(used, imm0[is_const])
    nodes = nodes.copy()
    nodes["imm0"] = new0.astype(nodes["imm0"].dtype)
    ts.pool = LocalPool(np.ascontiguousarray(b.pool.to_array()[used]) if len(used)
                        else np.zeros((1, 8), dtype=np.uint32))
    off = 0
    for t in tapes:
        ts.tapes.append(Tape(nodes[off:off + len(t)]))
        off += len(t)
    return ts


REFUTED = object()  # what a refuted query has in place of a schema (_attempt, last_miss)


class _Host(NamedTuple):
    """A query after _host_native / _host_python: its lowering, groups and tapes."""
    columns: Sequence[str]
    widths: Sequence[int]
    schema: Schema
    root_nodes: np.ndarray  # the root's tape, which the guide is harvested from
    ts: TapeSet             # one tape per group
    group_cols: Sequence[Sequence[int]]
    defs: list
    root_ends: Sequence[int]
    # what decide.eligible reads of a natively built query: (keccak reads?, keccak table?, column
    # kinds); None: never decided (the Python host stages, or decide_rows = 0)
    decide: Optional[tuple] = None
    refuted = False


class _Refuted:
    """_host_native's and _stage's answer for a query that contradicts itself: no device round.
    ``unsat``: every group was eligible for the decision step, so the query is decided UNSAT."""
    refuted = True

    def __init__(self, unsat: bool):
        self.unsat = unsat

    def close(self) -> None:
        pass


class NativeDefs(list):
    """The definitions the native query compiler eliminated (MH_QUERY_DEFINITIONS):
    [(column, tape of its defining term)] over the query's columns and constants ``consts``."""

    def __init__(self, items, consts):
        super().__init__(items)
        self.consts = consts


class NativeSchema(Schema):
    """The Schema of a query the native compiler built, decoded on first use: a witness's
    schema is read only when a model is evaluated (mythril/laser/smt/model.py:45-59, model.py
    here), LASER's is_possible never reads it (constraints.py:25-35)."""

    _FIELDS = ("cells", "uf_cells", "keccak", "columns")
    # one decode at a time, process-wide (a remembered witness may be read by several threads;
    # decodes are rare and short); not on the instance, so copies and pickles see only _cq
    _DECODE_LOCK = threading.Lock()

    def __init__(self, cq: "native.CompiledQuery", keccak_reads: bool = False):  # noqa: deferred
        self.__dict__["_cq"] = cq
        self.__dict__["keccak_reads"] = keccak_reads

    def __getattr__(self, name):
        if name not in self._FIELDS:
            raise AttributeError(name)
        # the compiled query is dropped only once the Schema is complete, so a decode that
        # raises leaves the next read to try again
        with NativeSchema._DECODE_LOCK:
            if name in self.__dict__:
                return self.__dict__[name]
            if "_cq" not in self.__dict__:
                raise AttributeError(name)
            self._decode(self.__dict__["_cq"])
            del self.__dict__["_cq"]
        return self.__dict__[name]

    def _decode(self, cq) -> None:
        cols = {n: Column(n, w, k, s, key) for n, w, k, s, key in cq.columns}
        cells: Dict[str, Dict[int, str]] = {}
        uf_cells: Dict[str, Dict[int, str]] = {}
        keccak: Dict[str, KeccakMap] = {}
        for kind, name_, items in cq.tables:
            if kind == native.TABLE_KECCAK:
                keccak[name_] = KeccakMap(items[0], dict(zip(items[1::2], items[2::2])))
            else:
                (cells if kind == native.TABLE_CELLS else uf_cells)[name_] = {
                    k: cell_name(name_, k) for k in items}
        Schema.__init__(self, cells, uf_cells, keccak, cols, self.__dict__["keccak_reads"])


def substitute(b: TapeBuilder, root: int, env: Dict[int, int]) -> int:
    """`root` with every VAR whose index is in `env` replaced by env's term (a rebuild of the
    nodes above the replaced ones; hash-consing shares everything else)."""
    nodes, out = b.nodes, {}
    st = [root]
    while st:
        n = st[-1]
        if n in out:
            st.pop()
            continue
        op, w, a, bb, c, i0, i1 = nodes[n]
        if op == Op.VAR:
            out[n] = env.get(i0, n)
            st.pop()
            continue
        k = ARITY[Op(op)]
        kids = (a, bb, c)[:k]
        todo = [x for x in kids if x not in out]
        if todo:
            st += todo
            continue
        st.pop()
        new = tuple(out[x] for x in kids)
        out[n] = n if new == kids else b.op(Op(op), *new, imm0=i0, imm1=i1)
    return out[root]


def eliminate_definitions(b: TapeBuilder, conj: Sequence[int], schema: Schema
                          ) -> Tuple[List[int], List[Tuple[str, int]]]:
    """Solve-for-a-symbol on the lowered conjuncts: a conjunct ``v == t`` whose one side is a
    scalar symbol ``v`` and whose other side is a computed term ``t`` over other columns (not a
    constant, not a symbol: the guide already proposes those) defines ``v``.  The definition is
    dropped and ``v`` replaced by ``t`` in every other conjunct; the query is equisatisfiable, and
    a row satisfying the rest extends to a model with ``v = t(row)``.  This is what a query like
    ``b == keccak(2 * keccak(a))`` (tests/laser/keccak_tests.py:122-138) needs: no candidate row
    guesses a 256-bit hash, but every row of ``a`` determines ``b``.

    Returns (remaining conjuncts over the other columns, [(column, defining term)]) with every
    defining term over undefined columns only."""
    kinds = schema.columns
    var_col = {b.var_index[n]: n for n, c in kinds.items() if c.kind == "var"}
    nodes = b.nodes
    env: Dict[int, int] = {}
    defs: List[Tuple[str, int]] = []
    rest: List[int] = []
    for cn in conj:
        op, _, a, bb, _, _, _ = nodes[cn]
        done = False
        if op == Op.EQ:
            for vn, t in ((a, bb), (bb, a)):
                nv = nodes[vn]
                if nv[0] != Op.VAR or nv[5] not in var_col or nv[5] in env:
                    continue
                if nodes[t][0] in (Op.VAR, Op.CONST):
                    continue
                t2 = substitute(b, t, env) if env else t
                reads = node_columns(b, [t2])[t2]
                if not reads or nv[5] in reads:
                    continue
                one = {nv[5]: t2}
                for v in list(env):  # earlier definitions may read v: keep them closed
                    env[v] = substitute(b, env[v], one)
                env[nv[5]] = t2
                defs.append((var_col[nv[5]], nv[5]))
                done = True
                break
        if not done:
            rest.append(cn)
    if not env:
        return list(conj), []
    return ([substitute(b, cn, env) for cn in rest],
            [(col, env[idx]) for col, idx in defs])


def _may_define(b: TapeBuilder, root: int) -> bool:
    """Whether a conjunct of `root` has the shape of a definition (``v == t`` with a symbol on
    one side and a computed term on the other; eliminate_definitions decides), memoised per
    node on the builder: a child query's AND node answers from its parent's."""
    memo = b.__dict__.setdefault("_may_define", {})
    got = memo.get(root)
    if got is not None:
        return got
    nodes = b.nodes
    stack, order = [root], []
    while stack:  # the AND nodes not answered yet, parents after children
        n = stack.pop()
        if n in memo:
            continue
        order.append(n)
        if nodes[n][0] == Op.AND:
            stack += [x for x in (nodes[n][2], nodes[n][3]) if x not in memo]
    for n in reversed(order):
        op, _, a, bb = nodes[n][:4]
        if op == Op.AND:
            memo[n] = memo[a] or memo[bb]
        elif op == Op.EQ:
            ka, kb = nodes[a][0], nodes[bb][0]
            memo[n] = ((ka == Op.VAR and kb not in (Op.VAR, Op.CONST))
                       or (kb == Op.VAR and ka not in (Op.VAR, Op.CONST)))
        else:
            memo[n] = False
    return memo[root]


class _Group:
    __slots__ = ("first", "idx", "conj", "vars", "acc")

    def __init__(self, first, idx, conj, vars_, acc):
        self.first, self.idx, self.conj, self.vars, self.acc = first, idx, conj, vars_, acc


class _BucketState:
    """The variable-disjoint groups of an AND chain's conjuncts, extendable by more conjuncts.
    Groups are immutable (a child state shares its parent's)."""

    def __init__(self):
        self.n = 0
        self.groups: Dict[object, _Group] = {}
        self.var_group: Dict[int, object] = {}

    def copy(self) -> "_BucketState":
        st = _BucketState()
        st.n, st.groups, st.var_group = self.n, dict(self.groups), dict(self.var_group)
        return st

    def add(self, b: TapeBuilder, cn: int, vs: frozenset) -> None:
        i = self.n
        self.n += 1
        and_ = int(Op.AND)
        if not vs:  # a ground conjunct: its own group (one per node)
            key = ("ground", cn)
            g = self.groups.get(key)
            self.groups[key] = (_Group(i, (i,), (cn,), frozenset(), cn) if g is None else
                                _Group(g.first, g.idx + (i,), g.conj + (cn,), g.vars,
                                       b._add(and_, 0, g.acc, cn)))
            return
        gids = {self.var_group[v] for v in vs if v in self.var_group}
        if not gids:
            key = ("vars", i)
            self.groups[key] = _Group(i, (i,), (cn,), vs, cn)
        elif len(gids) == 1:
            key = next(iter(gids))
            g = self.groups[key]
            self.groups[key] = _Group(g.first, g.idx + (i,), g.conj + (cn,), g.vars | vs,
                                      b._add(and_, 0, g.acc, cn))
        else:  # the conjunct joins several groups: one group, conjuncts in path order
            members = [self.groups.pop(k) for k in gids]
            pairs = sorted([p for g in members for p in zip(g.idx, g.conj)] + [(i, cn)])
            acc = pairs[0][1]
            for _, x in pairs[1:]:
                acc = b._add(and_, 0, acc, x)
            vars_ = frozenset(vs).union(*[g.vars for g in members])
            key = ("vars", min(g.first for g in members))
            self.groups[key] = _Group(pairs[0][0], tuple(p[0] for p in pairs),
                                      tuple(p[1] for p in pairs), vars_, acc)
        for v in self.groups[key].vars:
            self.var_group[v] = key

    def ordered(self) -> List[_Group]:
        return sorted(self.groups.values(), key=lambda g: g.first)


BUCKET_STATES = 256  # states of recent AND roots kept per builder


def _bucket_state(b: TapeBuilder, root: int) -> _BucketState:
    """The grouping of `root`'s conjuncts, memoised per AND root on the builder: a query that
    extends its parent (svm.py:257-262, root = AND(parent, new)) adds only its new conjunct."""
    memo = b.__dict__.setdefault("_bucket_states", OrderedDict())
    got = memo.get(root)
    if got is not None:
        memo.move_to_end(root)
        return got
    node = b.nodes[root]
    base = memo.get(node[2]) if node[0] == Op.AND else None
    if base is not None:
        st = base.copy()
        new = Sieve.conjuncts(b, node[3])
    else:
        st = _BucketState()
        new = Sieve.conjuncts(b, root)
    cols = node_columns(b, new)
    for cn in new:
        st.add(b, cn, cols[cn])
    memo[root] = st
    while len(memo) > BUCKET_STATES:
        memo.popitem(last=False)
    return st


# ops whose recomputation is cheap enough to duplicate instead of keeping a value live
_HEAVY = {Op.BVMUL, Op.BVUDIV, Op.BVUREM, Op.BVSDIV, Op.BVSREM, Op.BVSMOD, Op.KECCAK,
          Op.EVM_EXP, Op.BVMUL_NOOVFL_U, Op.EVM_ADDMOD, Op.EVM_MULMOD}


def rematerialize(nodes: np.ndarray, max_size: int) -> np.ndarray:
    """Duplicate cheap shared sub-terms (at most `max_size` nodes, no multiply / divide /
    keccak) at every use instead of keeping their values live.  A path condition reads the same
    calldata bytes in several overlapping words (calldata.py:48-54: word(0) and word(4) share 28
    byte terms), which otherwise holds more values live than the device register file has; the
    copies cost a few cheap instructions each."""
    n = len(nodes)
    ops = nodes["op"].astype(int)
    opnds = np.stack([nodes["a"], nodes["b"], nodes["c"]], axis=1).astype(int)
    ar = [ARITY[Op(o)] for o in ops]
    uses = np.zeros(n, dtype=int)
    size = np.zeros(n, dtype=int)
    cheap = np.zeros(n, dtype=bool)
    for i in range(n):
        kids = opnds[i, :ar[i]]
        for k in kids:
            uses[k] += 1
        size[i] = 1 + sum(int(size[k]) for k in kids)
        cheap[i] = (Op(ops[i]) not in _HEAVY and size[i] <= max_size
                    and all(cheap[k] for k in kids) and nodes["width"][i] <= 256)
    dup = cheap & (uses > 1)
    out: List[tuple] = []
    remap = {}

    def copy(k: int, deep: bool) -> int:
        # inside a duplicated sub-term every cheap node is copied too, so copies share nothing
        kids = [copy(int(x), True) if cheap[x] and (deep or dup[x]) else remap[int(x)]
                for x in opnds[k, :ar[k]]]
        rec = list(nodes[k].tolist())
        for j, x in enumerate(kids):
            rec[3 + j] = x
        out.append(tuple(rec))
        return len(out) - 1

    for i in range(n):
        if dup[i] and i != n - 1:
            continue
        remap[i] = copy(i, False)
    return np.array(out, dtype=nodes.dtype)


class _Staged:
    """A query after its host stage (Sieve._stage), before its rounds (Sieve._rounds): the
    lowering, the parent witness it was harvested under, the kept guide and the compiled tapes."""
    __slots__ = ("b", "key", "keccak_reads", "base_schema", "qno", "host", "col_index", "parent",
                 "parent_len", "guide", "ct", "t1")
    refuted = False  # (_stage's other answer is a _Refuted)

    def __init__(self, b, key, keccak_reads, base_schema, qno, host, col_index, parent,
                 parent_len, guide, ct, t1):
        self.b, self.key, self.keccak_reads, self.base_schema = b, key, keccak_reads, base_schema
        self.qno, self.host, self.col_index = qno, host, col_index
        self.parent, self.parent_len, self.guide, self.ct, self.t1 = (parent, parent_len, guide,
                                                                      ct, t1)

    def close(self) -> None:  # a staged query whose rounds never ran
        self.ct.close()
        self.guide.close()


def _row_values(row, columns: Sequence[str], cols: Sequence[int], out: Dict[str, int]):
    """A witness row's values (32 little-endian bytes each) in the columns `cols`, by name, put
    into `out`."""
    raw = np.ascontiguousarray(row, dtype="<u4").tobytes()
    for c in cols:
        out[columns[c]] = int.from_bytes(raw[32 * c:32 * c + 32], "little")
    return out


class _Run:
    """One staged query's rounds in progress (Sieve._rounds): what the rounds, the repair step
    and the decision step read and fill.  ``first``: its first round's results when a batched
    round has run it already -- (first hits, witness rows, buffer, listing): without a listing
    (None) no round of the query lists spare hits; with one (Sieve(batch_spares=True): the batch
    listed them, (hits, n_hits, rows, the spare rows it tried first)) every round does."""
    __slots__ = ("sieve", "s", "first", "budget", "t0", "columns", "group_cols", "solved", "values",
                 "ghits", "first_index", "use_hits", "buffer")

    def __init__(self, sieve: "Sieve", s: _Staged, first, budget: float, t0: float):
        self.sieve, self.s, self.first, self.budget, self.t0 = sieve, s, first, budget, t0
        self.columns, self.group_cols = s.host.columns, s.host.group_cols
        self.solved = [False] * len(self.group_cols)
        self.values: Dict[str, int] = {}
        # spare witnesses: a sequential query's guided rounds list K hits per group
        self.use_hits = sieve.spares > 0 and (first is None or first[3] is not None)
        self.ghits: List[Optional[List[Dict[str, int]]]] = [None] * len(self.group_cols)
        self.first_index: Optional[int] = None  # the smallest over rounds, repair and decide
        self.buffer: Optional[native.Assignments] = None  # the sieve's, once a step needed it

    def assign(self) -> native.Assignments:
        if self.buffer is None:
            self.buffer = self.sieve._buffer(len(self.columns))
        return self.buffer

    def spent(self) -> bool:
        return time.perf_counter() - self.t0 > self.budget

    def take(self, g: int, row, hit: int) -> None:
        """Group `g` is answered by witness row `row`, candidate number `hit`."""
        _row_values(row, self.columns, self.group_cols[g], self.values)
        self.solved[g] = True
        self.first_index = hit if self.first_index is None else min(self.first_index, hit)

    def complete(self, rounds: int, repaired: bool = False) -> Witness:
        """The witness of a query whose groups are all solved."""
        sieve, host, values = self.sieve, self.s.host, self.values
        for c in self.columns:  # columns no conjunct reads: any value is a model
            values.setdefault(c, 0)
        if host.defs:  # defined symbols take their terms' values under the row
            td = time.perf_counter()
            got = sieve.eval_definitions(self.s.b, host.defs, self.columns, values)
            for (c, _), v in zip(host.defs, got):
                values[c] = v
            sieve.stats.add("definitions", time.perf_counter() - td)
        w = Witness(host.schema, values, self.first_index, rounds, repaired=repaired)
        if self.use_hits:
            w.spares = self.spares(sieve.spares)
        return w

    def spares(self, k: int) -> List[Dict[str, int]]:
        """A solved query's spares: spare j (1 <= j < k) takes from every group g its hit
        j mod n_hits_g (a group solved by one row contributes that row); the query's columns
        only, a column no conjunct reads at 0 as in the witness.  Spares equal to the witness or
        to an earlier spare are dropped."""
        columns, values = self.columns, self.values
        lists = [self.ghits[g] or [{columns[c]: values[columns[c]] for c in cols}]
                 for g, cols in enumerate(self.group_cols)]
        base = {c: values[c] for c in columns}
        out: List[Dict[str, int]] = []
        for j in range(1, k):
            row = {c: 0 for c in columns}
            for rows in lists:
                row.update(rows[j % len(rows)])
            if row != base and row not in out:
                out.append(row)
        return out


class Sieve:
    """A device context plus reusable buffers; one per thread (handles are not shared)."""

    def __init__(self, device: int = 0, rows: int = 1 << 16, max_rounds: int = 2,
                 seed: int = 0x5EED5EED, budget_s: float = 0.25, first_rows: Optional[int] = None,
                 native_query: bool = True, second_round: Optional[str] = None,
                 keccak_second_chance: Optional[bool] = None, repair_rounds: int = 0,
                 repair_elites: Optional[int] = None, repair_children: Optional[int] = None,
                 decide_rows: int = 0, spares: int = 0, batch_spares: bool = False):
        self.ctx = native.Context(device)
        # host stages by the native query compiler (csrc/query.cpp); False: the Python stages
        # (lower.py, buckets, local_tapeset) it is checked against (tests/test_query_native.py)
        self.native_query = native_query
        # guide harvests that reuse the memo of the path's earlier queries (mh_harvester)
        self.guides = native.GuideSession()
        self.guides_kr: Optional[native.GuideSession] = None  # the second chance's (made on use)
        self.rows = rows
        # the harvested guide usually solves a LASER query in its first rows (round 1 found every
        # SAT witness of tests/laser_like.py within the first 16 rows): a small first round
        # answers those at a fraction of the latency, the full-size rounds follow.  4096 rows
        # (64 waves, one per SIMD of 64 CUs) take the 256-row round's time -- a short round is
        # latency-bound per wave -- and find in round 1 most of what round 2 found after 256
        # (planted random paths: 179 -> 60 round-2-only hits, profiles/r05g)
        if first_rows is None:  # SIEVE_FIRST_ROWS overrides the default (measurements)
            first_rows = int(os.environ.get("SIEVE_FIRST_ROWS", "4096"))
        self.first_rows = min(first_rows, rows)
        # a miss pays every round before z3 runs (an infeasible JUMPI branch, svm.py:257-262):
        # one 2^16-row round after the guided 256 keeps a miss near 1 ms of device time
        # (profiles/r03f: three such rounds took 1.6-2.3 ms) while no LASER-shaped SAT query
        # needed more than the first 256 rows
        self.max_rounds = max_rounds
        # when the rounds after the first run (SIEVE_ROUND2 overrides): "always"; "progress" --
        # only when the first round solved some of the query's groups but not all (a query
        # whose first round found nothing at all is left to the fallback at once); "never".
        # Default "progress": a first round that solves no group is almost always an UNSAT query
        # (EtherThief's UNSAT variant: 0.73 -> 0.45 ms, 400 constraints 2.48 -> 1.78 ms) and
        # the planted-SAT paths lose 2 of 2449 LASER-family answers (profiles/r05h)
        self.second_round = second_round or os.environ.get("SIEVE_ROUND2", "progress")
        if self.second_round not in ("always", "progress", "never"):
            raise ValueError("second_round must be always / progress / never")
        # a query the first lowering missed while an unsolved group read a keccak application
        # (fixed there at H(x), lower.py) is lowered again with keccak applications as read
        # columns (lower_query keccak_reads, MH_TERMS_KECCAK_READS) and given one more first
        # round: a path that pins keccak values elsewhere than H (VERDICT r5 missing 2; DESIGN
        # §6).  SIEVE_KECCAK2=0 turns it off (measurements)
        if keccak_second_chance is None:
            keccak_second_chance = os.environ.get("SIEVE_KECCAK2", "1") != "0"
        self.keccak_second_chance = keccak_second_chance
        # the second round of a query whose parent has a witness: the parent's witness under
        # the newest root's conjuncts (SIEVE_INCREMENTAL=0: the 2^16-row full-guide round)
        self.incremental_round = os.environ.get("SIEVE_INCREMENTAL", "1") != "0"
        # its rows: 16384 (256 one-wave workgroups, one per CU: a round's latency-bound cost
        # barely moves) answered 1.5 points more of the random family than 4096, LASER-shaped
        # latency unchanged (profiles/r06s)
        self.inc_rows = int(os.environ.get("SIEVE_INC_ROWS", "16384"))
        self.inc_hops = int(os.environ.get("SIEVE_INC_HOPS", "0"))  # newest_tape(hops)
        # its guide solving for one side of x op y == k with the other at the parent's value
        # (mh_guide_harvest_inc, SIEVE_INC_PEVAL=1): measured, not kept -- random recall 0.6686
        # -> 0.6625, learnt 0.9183 -> 0.9107 (profiles/r06v): its extra sets override the
        # parent's values in more rows than they complete
        self.inc_parent_eval = os.environ.get("SIEVE_INC_PEVAL", "0") == "1"
        # after the incremental round, the 2^16-row round of the full guide (SIEVE_ROUND3=1)
        self.round3 = os.environ.get("SIEVE_ROUND3", "0") == "1"
        # the last solve's rounds (diagnostics: scripts/planted_recall.py)
        self.last_rounds: Dict[str, int] = {}
        self.seed = seed
        self.budget_s = budget_s
        self.assign: Optional[native.Assignments] = None
        self.stats = SieveStats()
        self.witnesses: "OrderedDict[tuple, Dict[str, int]]" = OrderedDict()
        self.max_witnesses = 1 << 14
        # spare witnesses: with spares = K > 0 every guided round of a sequential
        # query lists its K smallest hits per group (native.query_round_hits), a solved query
        # keeps up to K - 1 further models beside its witness, and a query's first round tries its
        # nearest ancestor's witness and spares as its first rows.  0 (the default) runs none of
        # it.  SIEVE_SPARES overrides.
        self.spares = min(native.HITS_MAX, max(0, int(os.environ.get("SIEVE_SPARES", spares))))
        self.spare_witnesses: "OrderedDict[tuple, List[Dict[str, int]]]" = OrderedDict()
        # spares in solve_many's batched first rounds: the batch lists K hits per group
        # (native.query_round_hits_many) with every job's ancestor rows tried first, and the
        # batched queries store spares, as solve() does.  Only with spares > 0; off by default: a
        # batched first round then neither reads nor makes spares.  SIEVE_BATCH_SPARES overrides.
        self.batch_spares = self.spares > 0 and os.environ.get(
            "SIEVE_BATCH_SPARES", "1" if batch_spares else "0") == "1"
        # the last query this sieve missed after a device round, (key, schema): a model the
        # fallback then finds for it is learnt as its witness (learn)
        # (key, schema[, the keccak second chance's schema])
        self.last_miss: Optional[tuple] = None
        # the tape compile runs on the context's worker thread (mh_tapes_compile_async) while
        # this one harvests the guide: the harvest is host-only, both only read the query's
        # tapes, and the round needs both (SIEVE_OVERLAP=0: one after the other)
        self.overlap = os.environ.get("SIEVE_OVERLAP", "1") != "0"
        # repair of near-miss rows (Sieve._repair): iterations per unsolved group after
        # an attempt's ordinary rounds; 0 (the default) runs none of it.  SIEVE_REPAIR overrides.
        self.repair_rounds = int(os.environ.get("SIEVE_REPAIR", repair_rounds))
        # K elites x `per` children each: 64 x 64 = 4096 rows, the short-run launch shape (64
        # waves, one per SIMD of 64 CUs, as first_rows above)
        self.repair_elites = min(256, max(1, int(
            os.environ.get("SIEVE_REPAIR_ELITES", 64) if repair_elites is None else repair_elites)))
        self.repair_children = max(1, int(
            os.environ.get("SIEVE_REPAIR_CHILDREN", 64) if repair_children is None
            else repair_children))
        # a group stops when its best fail_count has not decreased for this many iterations, and
        # is not started when the best row of the first score fails more conjuncts than max_fail.
        # Tuned on the planted random family (20 paths x 16): an iteration costs tens
        # of microseconds of device time, so far rows are worth starting from (max_fail 4 -> 16:
        # recall 0.811 -> 0.840) and the stall rule is what ends a hopeless group (3 -> 2: the
        # same recall, 0.3 ms off the miss p50; 1 loses 4 points)
        self.repair_stall = int(os.environ.get("SIEVE_REPAIR_STALL", "2"))
        self.repair_max_fail = int(os.environ.get("SIEVE_REPAIR_MAX_FAIL", "16"))
        self.repair_max_conjuncts = int(os.environ.get("SIEVE_REPAIR_MAX_CONJUNCTS", "512"))
        # of the rows the last round left in the buffer, the first this many are scored: 4096
        # (the short-run launch shape) found better elites than all 16384 / 65536 -- the later
        # rows' best are no nearer, and K is fixed -- 0.840 -> 0.862 on the same workload
        self.repair_score_rows = min(1 << 16, max(1, int(
            os.environ.get("SIEVE_REPAIR_SCORE_ROWS", "4096"))))
        # decision by enumeration (Sieve._decide): after the rounds and repair, a group
        # still unsolved whose columns all have provable finite domains (native.domains_build)
        # with at most this many rows in their cross product is enumerated in order and decided
        # exactly -- its smallest row, or none, which makes the query UNSAT (last_unsat).  0 (the
        # default) runs none of it.  SIEVE_DECIDE_ROWS overrides.  (Capped far below the 2^64 - 1
        # at which a row count only reads "at least".)
        self.decide_rows = min(1 << 40, max(0, int(os.environ.get("SIEVE_DECIDE_ROWS",
                                                                   decide_rows))))
        # the last query was decided UNSAT: an eligible group has no row, or the host refuted an
        # eligible query.  Cleared per query; solve() still returns None.
        self.last_unsat = False
        self.repairer = None                                  # native.Repair, made on first use
        self.assign2: Optional[native.Assignments] = None     # the children's buffer
        # solve_many: first-round buffers (first_rows rows) by column capacity, kept between
        # calls; and the last call's per-query records
        self.round_pool: Dict[int, List[native.Assignments]] = {}
        self.last_many: List[Dict] = []
        self._certifier = None  # certify.Certifier, made on first use (certifier())

    def certifier(self):
        """This sieve's resident certifier (certify.Certifier): made on first use, closed with
        the sieve."""
        if self._certifier is None:
            from .certify import Certifier

            self._certifier = Certifier(self)
        return self._certifier

    def close(self) -> None:
        if self._certifier is not None:
            self._certifier.close()
            self._certifier = None
        if self.repairer is not None:
            self.repairer.close()
            self.repairer = None
        if self.assign2 is not None:
            self.assign2.close()
            self.assign2 = None
        if self.assign is not None:
            self.assign.close()
            self.assign = None
        for bufs in self.round_pool.values():
            for a in bufs:
                a.close()
        self.round_pool = {}
        self.guides.close()
        if self.guides_kr is not None:
            self.guides_kr.close()
        self.ctx.close()

    @staticmethod
    def _col_capacity(n_cols: int) -> int:
        """The column capacity of a buffer for `n_cols` columns: a power of two, 64 at least."""
        return 1 << (max(n_cols, 64) - 1).bit_length()

    def _buffer(self, n_cols: int) -> native.Assignments:
        rows = max(self.first_rows, (self.max_rounds - 1) * self.rows)
        if self.assign is None or self.assign.n_vars < n_cols or self.assign.capacity < rows:
            if self.assign is not None:
                self.assign.close()
            self.assign = self.ctx.assignments(self._col_capacity(n_cols), rows)
        return self.assign

    def remember(self, key: tuple, w: Witness) -> None:
        self._store(key, w.values, w.spares)

    def _store(self, key: tuple, values: Dict[str, int],
               spares: Optional[List[Dict[str, int]]] = None) -> None:
        self.witnesses[key] = values
        self.witnesses.move_to_end(key)
        if spares:
            self.spare_witnesses[key] = spares
            self.spare_witnesses.move_to_end(key)
        else:  # (a learnt model, or a witness found alone, replaces one that had spares)
            self.spare_witnesses.pop(key, None)
        while len(self.witnesses) > self.max_witnesses:
            old, _ = self.witnesses.popitem(last=False)
            self.spare_witnesses.pop(old, None)

    def forget(self, key: tuple) -> None:
        """Drop a query's witness and its spares (a witness the verifier or certifier rejected
        does not seed the query's children)."""
        self.witnesses.pop(key, None)
        self.spare_witnesses.pop(key, None)

    def learn(self, key: tuple, value_of: Callable[[Column], Optional[int]], ctx=None,
              value_at: Optional[Callable[[Column, int], Optional[int]]] = None) -> int:
        """A model the fallback found for the query this sieve missed last (the same ``key``)
        becomes that query's remembered witness, so the query's LASER children are generated
        around it as around a witness of the sieve's own (svm.py:257-262: the children of a state
        z3 found feasible are asked next).  Without it one miss leaves every later query of the
        path without parent-guided rows.  ``value_of(column)`` is the model's value of a column
        (lower.Column: a variable, an array or function cell), None where the model does not fix
        it.  With the query's term context ``ctx`` and ``value_at(column, index)``, the read
        columns (arrays, functions and keccak at symbolic index terms) are learnt too: their index
        terms are evaluated on the device over what was learnt so far (a read inside an index term
        is learnt on the next pass).  Returns the number of columns learnt."""
        lm, self.last_miss = self.last_miss, None
        if not key or lm is None or lm[0] != key:
            return 0
        values: Dict[str, int] = {}
        # the columns of both lowerings the miss tried (the keccak second chance's reads too:
        # a child's second chance is then generated around the model's keccak values)
        for sc in lm[1:]:
            for name, col in sc.columns.items():
                if name in values:
                    continue
                try:
                    v = value_of(col)
                except Exception:  # noqa: BLE001 - a column the model cannot evaluate stays free
                    v = None
                if v is not None:
                    values[name] = int(v) & ((1 << col.width) - 1)
        if ctx is not None and value_at is not None:
            self._learn_reads(lm[1:], values, ctx, value_at)
        if values:
            self._store(key, values)
            self.stats.bump("learnt")
        return len(values)

    def _learn_reads(self, schemas, values: Dict[str, int], ctx, value_at) -> None:
        """Sieve.learn's read columns: each index term evaluated over the values learnt so far
        (Model._evaluate, one device batch per pass), the model's value there; three passes at
        most (a read whose index reads another read)."""
        from .lower import READ_KINDS
        from .model import Model

        for sc in schemas:
            reads = [c for c in sc.columns.values() if c.kind in READ_KINDS]
            for _ in range(3):
                todo = [c for c in reads if c.name not in values]
                if not todo:
                    break
                try:
                    at = Model(self, ctx, sc, dict(values), 0)._evaluate(
                        [c.key for c in todo], [], True)
                except Exception:  # noqa: BLE001 - learning is best effort
                    return
                got = 0
                for c in todo:
                    idx = at.get(c.key)
                    if not isinstance(idx, int):
                        continue
                    try:
                        v = value_at(c, idx)
                    except Exception:  # noqa: BLE001
                        v = None
                    if v is not None:
                        values[c.name] = int(v) & ((1 << c.width) - 1)
                        got += 1
                if not got:
                    break

    def compile(self, ts: TapeSet) -> native.CompiledTapes:
        """Compile a query's tapes; a tape that runs out of registers is retried with cheap
        sub-terms duplicated at their uses (rematerialize), widening what counts as cheap."""
        orig = [t.nodes for t in ts.tapes]
        level = [0] * len(orig)
        sizes = (0, 8, 32, 256)
        while True:
            try:
                return self._count_spills(self.ctx.compile(ts))
            except native.Unsupported as e:
                m = re.search(r"tape (\d+): register pressure", str(e))
                if not m:
                    raise
                t = int(m.group(1))
                level[t] += 1
                if level[t] >= len(sizes):
                    raise
                ts.tapes[t] = Tape(rematerialize(orig[t], sizes[level[t]]))
                ts.flat = None  # the tapes no longer lie back to back
                self.stats.bump("remat_%d" % sizes[level[t]])

    def _count_spills(self, ct: native.CompiledTapes) -> native.CompiledTapes:
        """Counts the tapes whose live values exceed the interpreter's registers: they compile
        with spill code and run in the spill kernel (stats.extra["spilled_tapes"])."""
        spills = getattr(ct, "spills", None)  # (a stand-in context's tapes have none)
        n = int(np.count_nonzero(spills())) if spills is not None else 0
        if n:
            self.stats.bump("spilled_tapes", n)
        return ct

    @staticmethod
    def conjuncts(b: TapeBuilder, root: int) -> List[int]:
        """The leaves of `root`'s AND tree, left to right."""
        conj, stack = [], [root]
        while stack:
            n = stack.pop()
            if b.nodes[n][0] == Op.AND:
                stack += [b.nodes[n][3], b.nodes[n][2]]
            else:
                conj.append(n)
        return conj

    def solve_definitions(self, b: TapeBuilder, root: int, schema: Schema
                          ) -> Tuple[int, List[Tuple[str, int]]]:
        """`root` with its definitions eliminated (eliminate_definitions), and the definitions.
        A root whose conjuncts hold no candidate definition (memoised per AND node) is returned
        as it is without a walk over its conjuncts."""
        if not _may_define(b, root):
            return root, []
        conj = self.conjuncts(b, root)
        rest, defs = eliminate_definitions(b, conj, schema)
        if not defs:
            return root, []
        self.stats.bump("definitions", len(defs))
        if not rest:
            return b.true(), defs
        acc = rest[0]
        for x in rest[1:]:
            acc = b.op(Op.AND, acc, x)
        return acc, defs

    def eval_terms(self, b: TapeBuilder, terms: Sequence[int], columns: Sequence[str],
                   values: Dict[str, int], resident: Optional[dict] = None) -> List[int]:
        """The values of `terms` (bit-vector or Bool nodes over `columns`) under one assignment,
        evaluated on the device (mh_eval_values_many over a one-row buffer; `resident`, a dict
        the caller keeps, holds that buffer per column tuple across calls)."""
        return self.eval_tapeset(local_tapeset(b, terms, columns), columns, values, resident)

    def eval_definitions(self, b: TapeBuilder, defs, columns: Sequence[str],
                         values: Dict[str, int]) -> List[int]:
        """The defined columns' values under the witness row: the native compiler's definition
        tapes (NativeDefs), or the Python stages' terms."""
        if isinstance(defs, NativeDefs):
            ts = TapeSet(columns)
            ts.pool = LocalPool(defs.consts)
            ts.tapes = [Tape(t) for _, t in defs]
            return self.eval_tapeset(ts, columns, values)
        return self.eval_terms(b, [t for _, t in defs], columns, values)

    def eval_tapeset(self, ts: TapeSet, columns: Sequence[str], values: Dict[str, int],
                     resident: Optional[dict] = None) -> List[int]:
        """The root values of every tape of `ts` under one assignment of `columns`."""
        terms = ts.tapes
        ct = self.compile(ts)
        try:
            key = tuple(columns)
            assign = resident.get(key) if resident is not None else None
            if assign is None:
                assign = self.ctx.assignments(len(columns), 1)
                soa = np.zeros((len(columns), 8, 1), dtype=np.uint32)
                for i, c in enumerate(columns):
                    v = values.get(c, 0)
                    for k in range(8):
                        soa[i, k, 0] = (v >> (32 * k)) & 0xFFFFFFFF
                assign.upload(soa)
                if resident is not None:
                    resident[key] = assign
            try:
                # every root in one batch (mh_eval_values_many: one launch per register class)
                out = native.eval_values_many(self.ctx, ct, list(range(len(terms))), assign, 0)
                return [_limbs(out[i]) for i in range(len(terms))]
            finally:
                if resident is None:
                    assign.close()
        finally:
            ct.close()

    def _host_native(self, b: TapeBuilder, roots: Sequence[int], keccak_reads: bool = False):
        """The host stages by the native query compiler (mh_query_build: lowering, groups and
        tapes in one call, csrc/query.cpp); None for a query with a candidate definition (those
        take _host_python, whose eliminate_definitions solves for the symbol); a _Refuted for a
        conjunction that contradicts itself syntactically (MH_QUERY_REFUTED: x == 1 and x == 2,
        p and not p, bounds with an empty range), which no row can satisfy."""
        t0 = time.perf_counter()
        st = self.stats
        try:
            cq = native.TermMirror.of(b, keccak_reads).build(b, roots)
        except native.Unsupported:
            # a shape the native compiler refuses (a variable named like an array cell, ...):
            # the Python stages it restates may still take it
            st.bump("native_unsupported")
            st.add("lower", time.perf_counter() - t0)
            return None
        st.add("lower", time.perf_counter() - t0)
        dinfo = ((keccak_reads, cq.has_keccak_table(), cq.column_kinds())
                 if self.decide_rows > 0 else None)  # what eligibility reads (decide.eligible)
        if cq.flags & native.QUERY_REFUTED:
            st.bump("refuted")
            # the refuted conjunction is the lowered one: it stands for the caller's only when
            # every group is eligible (none of the query's columns or tapes touches keccak)
            return _Refuted(dinfo is not None and decide.eligible(
                *dinfo, range(len(cq.names)), cq.nodes))
        columns = cq.names
        defs = []
        if cq.flags & native.QUERY_DEFINITIONS:  # solved for the defined symbols natively
            st.bump("definitions", len(cq.defs))
            defs = NativeDefs([(columns[c], t) for c, t in zip(cq.defs, cq.def_tapes)],
                              cq.consts)
        ts = TapeSet(columns)
        ts.pool = LocalPool(cq.consts)
        tapes = cq.tapes
        ts.tapes = [Tape(t) for t in (tapes if len(tapes) == 1 else tapes[1:])]
        # the group tapes already lie back to back (tapes 1.., or the one tape): no concatenation
        k = 0 if len(tapes) == 1 else 1
        off = np.asarray(cq.tape_off[k:], dtype=np.uint64)
        ts.flat = (cq.nodes[cq.tape_off[k]:cq.tape_off[-1]], off - off[0], cq.consts)
        if len(cq.groups) > 1:
            st.bump("bucketed")
        return _Host(columns, cq.widths, NativeSchema(cq, keccak_reads), tapes[0], ts, cq.groups,
                     defs, [] if defs else cq.root_ends, dinfo)

    def _host_python(self, b: TapeBuilder, roots: Sequence[int], keccak_reads: bool = False):
        """The host stages in Python: lower_query, definitions, buckets, local tapes."""
        t0 = time.perf_counter()
        st = self.stats
        root, schema = lower_query(b, roots, keccak_reads=keccak_reads)
        t_l = time.perf_counter()
        st.add("lower", t_l - t0)
        columns = list(schema.columns)
        if not columns:  # ground query: one row decides it
            columns = ["__ground__"]
            b.var("__ground__", 1)
            schema.columns["__ground__"] = Column("__ground__", 1, "var", "__ground__")
        root, defs = self.solve_definitions(b, root, schema)
        groups = self.bucket_roots(b, root)
        col_of = {b.var_index[c]: i for i, c in enumerate(columns)}
        group_cols = [[col_of[v] for v in vs] for _, vs in groups]
        accs = [acc for acc, _ in groups]
        # the guide is harvested natively from the root's tape: the one tape of a query whose
        # conjuncts share columns (the same AND chain), else an extra tape of the same tape set
        # (same constants), not compiled
        if accs == [root]:
            ts = local_tapeset(b, accs, columns)
            root_nodes = ts.tapes[0].nodes
        else:
            ts = local_tapeset(b, [root] + accs, columns)
            root_nodes = ts.tapes.pop(0).nodes
        if len(groups) > 1:
            st.bump("bucketed")
        st.add("tapes", time.perf_counter() - t_l)
        widths = [schema.columns[c].width for c in columns]
        return _Host(columns, widths, schema, root_nodes, ts, group_cols, defs, [])

    @classmethod
    def buckets(cls, b: TapeBuilder, root: int) -> List[Tuple[List[int], set]]:
        """Variable-disjoint groups of the conjuncts of `root` (the DependenceMap of
        laser/smt/solver/independence_solver.py:38-83, over lowered columns): [(conjunct nodes,
        column var indices)], in order of each group's first conjunct.  Groups share no column,
        so each can take its witness from a different candidate row."""
        return [(list(g.conj), set(g.vars)) for g in _bucket_state(b, root).ordered()]

    @staticmethod
    def bucket_roots(b: TapeBuilder, root: int) -> List[Tuple[int, List[int]]]:
        """Per group of ``buckets``: (the AND of its conjuncts in order, its var indices)."""
        return [(g.acc, list(g.vars)) for g in _bucket_state(b, root).ordered()]

    def solve(self, b: TapeBuilder, roots: Sequence[int], key: Optional[tuple] = None,
              budget_s: Optional[float] = None) -> Optional[Witness]:
        """A witness of the conjunction of Bool nodes `roots` of builder `b`, or None.
        ``budget_s`` (get_model's remaining solver budget) caps this query's rounds below the
        sieve's own ``self.budget_s``; no round starts once it is spent.  A miss whose unsolved
        groups read a keccak application is tried once more with keccak applications as read
        columns (``keccak_second_chance``)."""
        t0 = time.perf_counter()
        budget = self.budget_s if budget_s is None else min(self.budget_s, budget_s)
        self.stats.queries += 1
        self.last_rounds = {}
        self.last_miss = None
        self.last_unsat = False
        if budget <= 0:
            self.stats.misses += 1
            return None
        qno = self.stats.queries
        staged = self._stage(b, roots, key, False, qno)
        return self._finish(b, roots, key, qno, staged, None, budget, t0)

    def _finish(self, b: TapeBuilder, roots: Sequence[int], key: Optional[tuple], qno: int,
                staged, first, budget: float, t0: float) -> Optional[Witness]:
        """A query from its host stage on (``staged``: _stage's result): the rounds, the keccak
        second chance and the accounting of the answer.  ``first``: its first round's results when
        a batched round (solve_many) has run it already."""
        st = self.stats
        self.last_unsat = False
        if staged.refuted:
            w, schema, kec = None, REFUTED, False
            if staged.unsat:
                self.last_unsat = True
                st.bump("decided_unsat")
        else:
            w, schema, kec = self._rounds(staged, budget, t0, first)
        schema2 = None
        if (w is None and kec and self.keccak_second_chance
                and time.perf_counter() - t0 < budget):
            st.bump("keccak2_tries")
            first_rounds = self.last_rounds
            try:
                w, schema2, _ = self._attempt(b, roots, key, budget, t0, True,
                                              base_schema=schema, qno=qno)
            except (LoweringUnsupported, native.Unsupported):
                # a shape the second lowering cannot take (register pressure of its larger
                # tapes, ...): the first attempt's miss stands
                st.bump("keccak2_unsupported")
                w = None
            self.last_rounds = dict(first_rounds, keccak2=int(w is not None))
            if w is not None:
                st.bump("keccak2_hits")
        if w is None:
            self.stats.misses += 1
            if schema is not REFUTED and key:
                self.last_miss = ((key, schema) if schema2 is None or schema2 is REFUTED
                                  else (key, schema, schema2))
            return None
        if key:
            self.remember(key, w)
        self.stats.hits += 1
        return w

    # queries per batched round: each has a first-round buffer of its own (first_rows rows by its
    # columns, 8 MiB at 64 columns), so the pool stays within half a GiB
    BATCH_MAX = 64

    def _pool_buffer(self, n_cols: int, taken: Dict[int, int]) -> native.Assignments:
        """A first-round buffer from the pool, of _buffer's column capacity; `taken` counts the
        ones this batch uses already."""
        cap = self._col_capacity(n_cols)
        bufs = self.round_pool.setdefault(cap, [])
        k = taken.get(cap, 0)
        taken[cap] = k + 1
        if k == len(bufs) or bufs[k].capacity < self.first_rows:
            a = self.ctx.assignments(cap, self.first_rows)
            if k == len(bufs):
                bufs.append(a)
            else:
                bufs[k].close()
                bufs[k] = a
        return bufs[k]

    def solve_many(self, b, queries: Sequence[Sequence[int]],
                   keys: Optional[Sequence[Optional[tuple]]] = None,
                   budget_s: Optional[float] = None) -> List[Optional[Witness]]:
        """solve() for a list of independent queries of builder `b` (or of one builder per query,
        given as a list), with the first round of
        every query that needs one run in one device submission (native.query_round_many; with
        ``batch_spares`` native.query_round_hits_many, which lists every group's K smallest hits
        after trying each query's ancestor rows first, as solve()'s first round does)
        instead of one submission each.  Returns a witness or None per query; ``last_many`` has,
        per query, ``miss`` (what last_miss would have been), ``rounds`` (last_rounds), ``unsat``
        (True for a query decided UNSAT, last_unsat; absent otherwise) and ``error`` (the exception
        an unsupported query raises from solve(), reported here instead: it does not fail the list).

        On Sieves created alike, the witnesses, their ``index`` and ``rounds``, the stats counters
        and the ``witnesses`` store are what calling solve() on the list in order gives:
        query numbers (the generator's global_base) go by list position; a query whose parent key
        (within ANCESTORS) is an earlier query's key in the list starts a new batch, after that
        one has finished, so it is harvested under the same parent witness; every later round
        (incremental, second_round, keccak second chance, repair) runs one query at a time as in
        solve().  An exact duplicate (same key and roots) of an earlier query in the list is not
        solved again: it takes a query number and the earlier one's answer.  ``budget_s`` is the
        whole list's budget; a query not started when it is spent is a miss."""
        t0 = time.perf_counter()
        budget = self.budget_s if budget_s is None else min(self.budget_s, budget_s)
        n = len(queries)
        packed: Dict[tuple, np.ndarray] = {}  # ancestors' rows as limbs, shared by siblings
        # (one builder for the list, or one per query: paths built in contexts of their own)
        bs = list(b) if isinstance(b, (list, tuple)) else [b] * n
        if len(bs) != n:
            raise ValueError("solve_many: one builder, or one per query")
        keys = list(keys) if keys is not None else [None] * n
        if len(keys) != n:
            raise ValueError("solve_many: one key (or None) per query")
        out: List[Optional[Witness]] = [None] * n
        rec: List[Dict] = [dict(miss=None, rounds={}, error=None) for _ in range(n)]
        self.last_many = rec
        st = self.stats
        ident = [(id(bs[i]), keys[i], tuple(queries[i])) for i in range(n)]
        seen: Dict[tuple, int] = {}
        i = 0
        while i < n:
            # the next batch: queries up to one that must see an earlier one's witness
            seg_keys, seg, dups = set(), [], []
            j = i
            while j < n and len(seg) < self.BATCH_MAX:
                k = keys[j]
                if any(p in seg_keys for p in self._prefixes(k)):
                    break
                if ident[j] in seen:
                    dups.append((j, seen[ident[j]]))
                else:
                    seen[ident[j]] = j
                    seg.append(j)
                    if k:
                        seg_keys.add(k)
                j += 1
            staged: Dict[int, object] = {}
            try:
                # 1. numbers and host stages, in list order
                qnos = {}
                for q in sorted(seg + [d for d, _ in dups]):
                    st.queries += 1
                    qnos[q] = st.queries
                for q in seg:
                    if budget <= 0 or time.perf_counter() - t0 >= budget:
                        st.misses += 1
                        continue
                    try:
                        staged[q] = self._stage(bs[q], queries[q], keys[q], False, qnos[q])
                    except Exception as e:  # noqa: BLE001 - what solve() raises, per query
                        rec[q]["error"] = e
                # 2. one submission for every first round
                live = [q for q in seg if q in staged and not staged[q].refuted]
                firsts: Dict[int, tuple] = {}
                if len(live) > 1:
                    taken: Dict[int, int] = {}
                    jobs = []
                    for q in live:
                        s = staged[q]
                        n_cols = len(s.host.columns)
                        job = dict(tapes=s.ct, assign=self._pool_buffer(n_cols, taken),
                                   guide=s.guide, seed=self.seed, global_base=s.qno << 24,
                                   count=self.first_rows, n_cols=n_cols)
                        if self.batch_spares:
                            # the rows the query's first round tries first: its ancestor has
                            # finished (it is in an earlier batch), so they are what solve() reads
                            job.update(k=self.spares, spares=self._spare_rows(
                                s.key, s.parent, s.col_index, self.first_rows, packed))
                        else:
                            job["mode"] = native.MODE_FIRST_HIT
                        jobs.append(job)
                    tb = time.perf_counter()
                    try:
                        res = (native.query_round_hits_many(self.ctx, jobs) if self.batch_spares
                               else native.query_round_many(self.ctx, jobs))
                    except native.SieveError:  # (a shape the batch refuses: one by one instead)
                        st.bump("batch_refused")
                        res = None
                    st.add("run", time.perf_counter() - tb)
                    if res is not None:
                        st.bump("batched_rounds", len(live))
                        st.bump("batches")
                        for q, job, r in zip(live, jobs, res):
                            if self.batch_spares:
                                hh, nh, _, hrows = r
                                firsts[q] = (hh[:, 0], hrows[:, 0], job["assign"],
                                             (hh, nh, hrows, job["spares"]))
                            else:
                                firsts[q] = (r[0], r[2], job["assign"], None)
                # 3. every query's later rounds and accounting, in list order
                dup_of = dict(dups)
                for q in range(i, j):
                    if q in dup_of:  # the earlier query's answer, accounted and stored again
                        orig = dup_of[q]
                        out[q] = out[orig]
                        rec[q] = dict(rec[orig])
                        if rec[orig]["error"] is None:
                            if out[orig] is None:
                                st.misses += 1
                            else:
                                st.hits += 1
                                if keys[q]:
                                    self.remember(keys[q], out[orig])
                        continue
                    if q not in staged:
                        continue
                    s = staged.pop(q)
                    self.last_rounds = {}
                    self.last_miss = None
                    try:
                        out[q] = self._finish(bs[q], queries[q], keys[q], qnos[q], s, firsts.get(q),
                                              budget, t0)
                    except Exception as e:  # noqa: BLE001
                        rec[q]["error"] = e
                    rec[q]["miss"], rec[q]["rounds"] = self.last_miss, self.last_rounds
                    if self.last_unsat:  # (only ever with decide_rows set)
                        rec[q]["unsat"] = True
            finally:
                for s in staged.values():  # an interrupted batch: nothing stays open
                    s.close()
            i = j
        self.last_rounds = {}
        self.last_miss = None
        self.last_unsat = False
        return out

    def _guide_session(self, keccak_reads: bool) -> "native.GuideSession":
        """The harvester session of a lowering mode (each keeps its own path's memo)."""
        if not keccak_reads:
            return self.guides
        if self.guides_kr is None:
            self.guides_kr = native.GuideSession()
        return self.guides_kr

    # how far up a path Sieve._ancestor looks for a witness: 1, the parent.  Looking 8 up (past a
    # missed parent) answered 13 instead of 8 queries after a miss on the planted random family
    # (recall 0.651 either way) and took its misses from 1.32 to 2.24 ms (p50; profiles/r06l):
    # under the plugin a missed parent has the fallback's model learnt anyway
    ANCESTORS = int(os.environ.get("SIEVE_ANCESTORS", "1"))

    def _prefixes(self, key: Optional[tuple]) -> Iterator[tuple]:
        """The keys of the query's last ANCESTORS prefixes, the parent's first."""
        n = len(key) if key else 0
        for j in range(n - 1, max(n - 1 - self.ANCESTORS, 0), -1):
            yield key[:j]

    def _ancestor(self, key: Optional[tuple], root_ends: Sequence[int]):
        """(witness, root-tape nodes of its query) of the nearest of the query's last ANCESTORS
        prefixes that has a witness -- the parent, or past a missed parent the state above it
        (its children are then searched around the last model the path had) -- or (None, 0)."""
        p = self._ancestor_key(key)
        if p is None:
            return None, 0
        return self.witnesses[p], (root_ends[len(p) - 1] if len(p) - 1 < len(root_ends) else 0)

    def _ancestor_key(self, key: Optional[tuple]) -> Optional[tuple]:
        """The key _ancestor's witness is stored under, or None."""
        for p in self._prefixes(key):
            if p in self.witnesses:
                return p
        return None

    def _spare_rows(self, key: Optional[tuple], parent, col_index: Dict[str, int], n: int,
                    packed: Optional[Dict[tuple, np.ndarray]] = None):
        """The rows a query's first round tries first: its ancestor's witness, then the ancestor's
        spares, over the columns every one of them and the query have -- (column numbers
        ascending, values u32 [rows, columns, 8]) -- or None when the ancestor has no spares.
        At most `n` rows (the round's).  ``packed`` (solve_many): the values by (ancestor key,
        column names), so that siblings pack their ancestor's rows into limbs once."""
        pk = self._ancestor_key(key)
        extra = self.spare_witnesses.get(pk) if pk is not None else None
        if not extra or not parent or self.witnesses.get(pk) is not parent:
            return None
        rows = ([parent] + list(extra))[:n]
        names = [c for c in col_index if all(c in r for r in rows)]
        if not names:
            return None
        names.sort(key=col_index.__getitem__)
        vals = packed.get((pk, tuple(names), len(rows))) if packed is not None else None
        if vals is None:
            vals = np.zeros((len(rows), len(names), 8), dtype=np.uint32)
            for i, r in enumerate(rows):
                raw = b"".join((int(r[c]) & ((1 << 256) - 1)).to_bytes(32, "little")
                               for c in names)
                vals[i] = np.frombuffer(raw, dtype="<u4").reshape(len(names), 8)
            if packed is not None:
                packed[pk, tuple(names), len(rows)] = vals
        return np.array([col_index[c] for c in names], dtype=np.uint32), vals

    def _parent_kreads(self, b: TapeBuilder, schema: Schema, base_schema: Schema,
                       parent: Dict[str, int]) -> Dict[str, int]:
        """The parent's witness with the keccak read columns of `schema` (the second chance's
        lowering) it lacks -- a witness of the default lowering has none -- at the values the
        default lowering gives those applications under it (the stated pair or H(x),
        `base_schema`; one device batch).  The incremental round's parent rows then satisfy
        the parent's keccak conjuncts too."""
        need = [c for c in schema.columns.values()
                if c.kind == "kread" and c.name not in parent]
        if not need:
            return parent
        try:
            sc = deepcopy(base_schema)
            L = Lowering(b, sc)
            terms = [L.lower(b.apply(c.symbol, b.widths[c.key], 256, c.key)) for c in need]
            vals = self.eval_terms(b, terms, list(sc.columns) or ["__ground__"], parent)
        except (LoweringUnsupported, native.Unsupported, TapeError):
            return parent
        out = dict(parent)
        for c, v in zip(need, vals):
            out[c.name] = v
        self.stats.bump("parent_kreads")
        return out

    def _attempt(self, b: TapeBuilder, roots: Sequence[int], key: Optional[tuple],
                 budget: float, t0: float, keccak_reads: bool,
                 base_schema: Optional[Schema] = None, qno: Optional[int] = None):
        """One lowering of the query and its rounds: (witness or None, schema or REFUTED,
        whether a group left unsolved reads a keccak application).  ``base_schema``: the
        default lowering's schema, for the second chance's incremental round."""
        staged = self._stage(b, roots, key, keccak_reads,
                             self.stats.queries if qno is None else qno, base_schema)
        if staged.refuted:
            return None, REFUTED, False
        return self._rounds(staged, budget, t0)

    def _stage(self, b: TapeBuilder, roots: Sequence[int], key: Optional[tuple],
               keccak_reads: bool, qno: int, base_schema: Optional[Schema] = None):
        """The host stage of one lowering of a query: native build (a _Refuted when the query
        contradicts itself: no device round), guide harvest and tape compile.  ``qno``: the
        query's number (stats.queries when sequential solve reaches it), which its rounds'
        global_base is made of.  The result owns the guide and the compiled tapes until _rounds
        (or its close()) releases them."""
        st = self.stats
        th = time.perf_counter()
        host = self._host_native(b, roots, keccak_reads) if self.native_query else None
        if host is None:  # (a query that takes the Python stages is never decided)
            host = self._host_python(b, roots, keccak_reads)
        if host.refuted:  # no witness exists: no device round (the fallback still runs)
            self.stats.host_s += time.perf_counter() - th
            return host
        columns, widths, ts = host.columns, host.widths, host.ts
        t_t = time.perf_counter()
        pending = None
        try:  # from the compile's start: an error on this side still collects it
            if self.overlap and hasattr(self.ctx, "compile_async"):
                pending = self.ctx.compile_async(ts)
            col_index = {c: i for i, c in enumerate(columns)}
            parent, parent_len = self._ancestor(key, host.root_ends)
            guide = native.harvest_guide(
                host.root_nodes, ts.pool.to_array(), widths,
                [(col_index[k], v) for k, v in parent.items() if k in col_index] if parent else (),
                session=self._guide_session(keccak_reads), keep=True)  # kept for the rounds
        except BaseException:
            if pending is not None:  # the compile's tapes are not needed
                try:
                    pending.wait().close()
                except Exception:  # noqa: BLE001 - the harvest's error is the one to report
                    pass
            raise
        t1 = time.perf_counter()
        st.add("guide", t1 - t_t)
        self.stats.host_s += t1 - th
        try:
            ct = None
            if pending is not None:
                try:
                    ct = pending.wait()
                except native.Unsupported:  # register pressure: Sieve.compile's retries
                    ct = None
                if ct is not None:  # its own duration; the part the harvest did not hide
                    self._count_spills(ct)
                    st.add("compile", ct.timing[1])
                    st.add("compile_wait", time.perf_counter() - t1)
            if ct is None:
                ct = self.compile(ts)
                st.add("compile", time.perf_counter() - t1)
        except BaseException:
            guide.close()
            raise
        return _Staged(b, key, keccak_reads, base_schema, qno, host, col_index, parent, parent_len,
                       guide, ct, t1)

    def _launches(self, s: _Staged) -> Tuple[List[int], bool]:
        """The rows of a staged query's rounds, and whether the second is the incremental one."""
        # the incremental round: the parent's witness under the newest root's conjuncts' sets only
        # (the parent's conjuncts hold there already), instead of the 2^16-row round of the full
        # guide -- a child whose own conjunct the full guide's rows keep breaking while they break
        # the parent's
        inc_ok = bool(s.parent) and s.parent_len > 0 and self.incremental_round
        launches = [self.first_rows]
        if self.max_rounds > 1:
            launches.append(min(self.inc_rows, self.rows) if inc_ok
                            else (self.max_rounds - 1) * self.rows)
        if s.keccak_reads and not inc_ok:  # the second chance: one first round
            launches = launches[:1]
        if inc_ok and self.round3 and self.max_rounds > 1 and not s.keccak_reads:
            launches.append((self.max_rounds - 1) * self.rows)  # then the full guide's
        return launches, inc_ok

    def _incremental_guide(self, s: _Staged):
        """The incremental round's guide (kept; the caller closes it): harvested from the conjuncts
        the query adds to its parent's, under the parent's witness.  None when it adds none."""
        st, host = self.stats, s.host
        ti = time.perf_counter()
        inc = newest_tape(host.root_nodes, s.parent_len, self.inc_hops)
        if inc is None:
            return None
        pv = s.parent
        if s.keccak_reads and s.base_schema is not None and s.base_schema is not REFUTED:
            pv = self._parent_kreads(s.b, host.schema, s.base_schema, s.parent)
        guide = native.harvest_guide(
            inc, host.ts.pool.to_array(), host.widths,
            [(s.col_index[k], v) for k, v in pv.items() if k in s.col_index],
            keep=True, parent_eval=self.inc_parent_eval)
        st.add("guide", time.perf_counter() - ti)
        st.bump("inc_rounds")
        self.last_rounds["incremental"] = 1
        return guide

    def _round(self, run: _Run, rnd: int, n: int, base: int, guide) -> None:
        """Round `rnd` of a query: `n` rows of `guide` numbered from `base`, over the tapes from
        the first to the last unsolved group; the groups it answers are taken into `run`."""
        st, s, solved, n_cols = self.stats, run.s, run.solved, len(run.columns)
        tb = time.perf_counter()
        g0 = solved.index(False)
        g1 = len(solved) - solved[::-1].index(False)
        hrows, nh, n_sp = None, None, 0
        if rnd == 0 and run.first is not None:
            fh, wrows = run.first[0], run.first[1]  # run by solve_many's batched round
            if run.first[3] is not None:  # which listed the hits and tried the ancestor's rows
                _, nh, hrows, sp = run.first[3]
                n_sp = len(sp[1]) if sp is not None else 0
                st.bump("spare_rows", n_sp)
                self.last_rounds["spares"] = n_sp
                self.last_rounds["spare_hit"] = 0
        else:
            assign = run.assign()
            # generator, run, and the first witnesses with their rows' columns in one call and one
            # copy back (mh_query_round)
            if run.use_hits:
                # the same round with the K smallest hits of every group listed
                # (mh_query_round_hits); hit 0 is the witness's row.  The first round's first rows
                # are the ancestor's witness and spares
                sp = self._spare_rows(s.key, s.parent, s.col_index, n) if rnd == 0 else None
                n_sp = len(sp[1]) if sp is not None else 0
                if rnd == 0:
                    st.bump("spare_rows", n_sp)
                    self.last_rounds["spares"] = n_sp
                    self.last_rounds["spare_hit"] = 0
                hh, nh, _, hrows = native.query_round_hits(
                    self.ctx, s.ct, assign, guide, self.seed, base, n, n_cols, self.spares,
                    spares=sp, tape_first=g0, tape_count=g1 - g0)
                fh, wrows = hh[:, 0], hrows[:, 0]
            else:
                fh, _, wrows = native.query_round(
                    self.ctx, s.ct, assign, guide, self.seed, base, n, n_cols,
                    tape_first=g0, tape_count=g1 - g0, mode=native.MODE_FIRST_HIT)
            st.add("run", time.perf_counter() - tb)
        st.rounds += 1
        st.rows += n
        fresh = []  # the groups this round solves
        for i, hit in enumerate(fh.tolist()):
            g = g0 + i
            if solved[g] or hit == native.NO_HIT:
                continue
            run.take(g, wrows[i], hit)
            fresh.append(hit)
            if hrows is not None:
                run.ghits[g] = [_row_values(hrows[i, j], run.columns, run.group_cols[g], {})
                                for j in range(int(nh[i]))]
        if n_sp and all(solved) and len(fresh) == len(solved) and max(fresh) < base + n_sp:
            # every group answered by one of the ancestor's rows
            st.bump("spare_hits")
            self.last_rounds["spare_hit"] = 1

    def _rounds(self, s: _Staged, budget: float, t0: float, first=None):
        """The rounds of a staged query: (witness or None, schema, whether a group left unsolved
        reads a keccak application).  ``first`` = (first_hit, witness rows, the buffer they were
        generated into, the listing or None: _Run) of its first round when a batched round has
        run it already: the round is then accounted and read as if it had run here."""
        st, schema = self.stats, s.host.schema
        t_c = time.perf_counter()
        run = _Run(self, s, first, budget, t0)
        inc_guide = None
        ft, nt = getattr(s.ct, "timing", (0.0, 0.0))
        st.add("compile_flatten", ft)
        st.add("compile_native", nt)
        try:
            launches, inc_ok = self._launches(s)
            self.last_rounds = {"groups": len(run.solved), "r1_solved": 0, "rounds": 0}
            round_guide = s.guide  # the incremental round's own guide replaces it (closed below)
            offset = (1 << 23) if s.keccak_reads else 0
            last_n = 0
            for rnd, n in enumerate(launches):
                if rnd == 2:
                    round_guide = s.guide
                if rnd == 1:
                    k = sum(run.solved)
                    self.last_rounds["r1_solved"] = k
                    if self.second_round == "never" or (self.second_round == "progress"
                                                        and k == 0):
                        st.bump("round2_skipped")
                        break
                    if inc_ok:
                        round_guide = inc_guide = self._incremental_guide(s)
                        if inc_guide is None:
                            break
                self.last_rounds["rounds"] = rnd + 1
                base = (s.qno << 24) + offset
                offset += n
                last_n = n
                self._round(run, rnd, n, base, round_guide)
                if all(run.solved):
                    w = run.complete(rnd + 1)
                    if rnd and inc_ok:
                        st.bump("inc_hits")
                    return w, schema, False
                if run.spent():
                    break
            if self.repair_rounds > 0 and last_n and not all(run.solved) and not run.spent():
                if run.buffer is None:
                    # repair straight after a batched first round: its rows regenerated into the
                    # buffer repair reads (and writes children into), the one sequential solve
                    # leaves them in -- one deterministic launch on a rare path
                    run.assign().generate_guided(self.seed, s.guide.arrays(),
                                                 global_base=s.qno << 24, first=0, count=last_n)
                    if first is not None and first[3] is not None and first[3][3] is not None:
                        run.assign().scatter(0, *first[3][3])  # (with the rows it tried first)
                    st.bump("repair_regenerated")
                self._repair(run, last_n, (s.qno << 24) + offset)
                if all(run.solved):
                    return run.complete(self.last_rounds["rounds"], repaired=True), schema, False
            if self.decide_rows > 0 and s.host.decide is not None and not all(run.solved):
                unsat, _ = self._decide(run)
                if unsat:  # an eligible group has no row: no witness, and no second chance
                    self.last_unsat = True
                    st.bump("decided_unsat")
                    return None, schema, False
                if all(run.solved):
                    return run.complete(self.last_rounds.get("rounds", 0)), schema, False
            kec = any(not run.solved[g] and _reads_keccak(s.host.ts.tapes[g].nodes)
                      for g in range(len(run.solved)))
            return None, schema, kec
        finally:
            s.ct.close()
            s.guide.close()
            if inc_guide is not None:
                inc_guide.close()
            # (a batched query's stage ended before the other queries' stages and the batch)
            self.stats.device_s += time.perf_counter() - (s.t1 if first is None else t_c)

    def _decide(self, run: _Run):
        """The decision step (DESIGN §6 "Decision by enumeration"), after the rounds and repair:
        every group still unsolved that is eligible (decide.eligible: UNSAT of the lowered group
        implies UNSAT of the caller's constraints) and whose domains' cross product has at most
        decide_rows rows is enumerated in order, in windows of the sieve's buffer
        (mh_query_enumerate, FIRST_HIT), up to the first window with a hit.  A hit is taken into
        `run` as a round's is.  Returns (whether some group was found empty --
        no rows at all, or enumerated to the end without a hit -- which makes the query UNSAT,
        the smallest hit index or None).  A group whose enumeration the budget cuts short stays
        undecided, never empty."""
        st, host, solved, group_cols = self.stats, run.s.host, run.solved, run.group_cols
        ts, assign = host.ts, run.assign()
        first_hit = None
        consts = ts.pool.to_array()
        for g in range(len(solved)):
            if solved[g]:  # (a ground group's product is the one empty row: its tape decides)
                continue
            nodes = ts.tapes[g].nodes
            if not decide.eligible(*host.decide, group_cols[g], nodes):
                st.bump("decide_ineligible")
                continue
            td = time.perf_counter()
            dom = native.domains_build(nodes, consts, host.widths, group_cols[g])
            try:
                if dom.rows > self.decide_rows:
                    st.bump("decide_too_large")
                    continue
                window = assign.capacity
                base, hit, row = 0, None, None
                while base < dom.rows:
                    if run.spent():
                        break
                    n = min(window, dom.rows - base)
                    fh, _, wrows = native.query_enumerate(self.ctx, run.s.ct, assign, dom, base, n,
                                                          len(run.columns), tape=g,
                                                          mode=native.MODE_FIRST_HIT)
                    st.bump("decide_rows", n)
                    st.rows += n
                    base += n
                    if int(fh[0]) != native.NO_HIT:
                        hit, row = int(fh[0]), wrows[0]
                        break
                if hit is not None:
                    run.take(g, row, hit)
                    first_hit = hit if first_hit is None else min(first_hit, hit)
                    st.bump("decided_sat")
                elif base >= dom.rows:  # the whole product (or an empty one) holds no model
                    return True, first_hit
                else:
                    st.bump("decide_budget")
            finally:
                dom.close()
                st.add("decide", time.perf_counter() - td)
        return False, first_hit

    def _repair(self, run: _Run, n_rows: int, base: int):
        """The repair step, after an attempt's ordinary rounds left groups unsolved:
        per unsolved group, the `n_rows` rows the last round left in the buffer are scored by the
        group's conjuncts they fail (mh_repair_score over the conjunct plan's tapes), the best K kept
        (mh_repair_select) and `per` children made of each with ONE failing conjunct's columns
        regenerated from that conjunct's own sets (mh_repair_mutate); the group's tape decides
        over the children as in an ordinary round, and the children are scored for the next
        iteration (children numbered from `base`).  The groups it answers are taken into `run`;
        returns the smallest hit index or None."""
        st, s, solved, group_cols = self.stats, run.s, run.solved, run.group_cols
        columns, ts, ct, guide, assign = run.columns, s.host.ts, s.ct, s.guide, run.assign()
        K, per = self.repair_elites, self.repair_children
        n_rows = min(n_rows, self.repair_score_rows)
        lr = self.last_rounds
        lr["repair"] = 0
        first_hit = set_leaf = None
        for g in range(len(solved)):
            if solved[g] or not group_cols[g]:  # (a ground group has no column to repair)
                continue
            if run.spent():
                break
            tr = time.perf_counter()
            try:
                plan = native.ConjunctPlan(s.host.root_nodes,
                                           group_cols[g] if len(group_cols) > 1 else (),
                                           self.repair_max_conjuncts)
            except native.Unsupported:  # one conjunct, or too many: no repair for this group
                st.bump("repair_skipped")
                continue
            cts = TapeSet(columns)
            cts.pool = ts.pool
            cts.tapes = [Tape(t) for t in plan.tapes]
            cts.flat = (plan.nodes, plan.tape_off, ts.pool.to_array())
            try:
                cct = self.compile(cts)
            except native.Unsupported:
                st.bump("repair_skipped")
                continue
            try:
                st.bump("repair_tries")
                if set_leaf is None:
                    set_leaf = guide.set_conjuncts()
                tags = plan.set_ordinals(set_leaf)
                if self.repairer is None:
                    self.repairer = native.repair_open(self.ctx, self.repair_max_conjuncts, 1 << 16,
                                                       256)
                rep = self.repairer
                if (self.assign2 is None or self.assign2.n_vars != assign.n_vars
                        or self.assign2.capacity < K * per):
                    if self.assign2 is not None:
                        self.assign2.close()
                    self.assign2 = self.ctx.assignments(assign.n_vars, K * per)
                src, dst = assign, self.assign2
                if src.capacity < K * per:  # the children ping-pong between the two buffers
                    K = max(1, src.capacity // per)
                native.repair_score(rep, cct, src, row_count=n_rows)
                best_seen, stalled = None, 0
                for it in range(self.repair_rounds):
                    if run.spent():
                        break
                    el = native.repair_select(rep, K, self.seed + it)
                    best = int(el[0]["fail_count"])
                    if it == 0 and best > self.repair_max_fail:
                        st.bump("repair_far")
                        break
                    hit = native.NO_HIT
                    if best == 0:
                        # every conjunct of the group holds on the row: confirmed by the group's own
                        # tape, the authority of an ordinary round
                        r0 = int(el[0]["row"])
                        fh, _, wrows = native.run_rows(self.ctx, ct, src, len(columns), tape_first=g,
                                                       tape_count=1, row_first=r0, row_count=1,
                                                       index_base=base - r0,
                                                       mode=native.MODE_FIRST_HIT)
                        hit = int(fh[0])
                    if hit == native.NO_HIT:
                        if best_seen is not None and best >= best_seen:
                            stalled += 1
                            if stalled >= self.repair_stall:
                                break
                        else:
                            best_seen, stalled = best, 0
                        st.bump("repair_iters")
                        lr["repair"] += 1
                        n_ch = len(el) * per
                        native.repair_mutate(rep, src, dst, guide, tags, plan.col_off,
                                             plan.cols_flat, per, seed=self.seed, global_base=base)
                        fh, _, wrows = native.run_rows(self.ctx, ct, dst, len(columns), tape_first=g,
                                                       tape_count=1, row_first=0, row_count=n_ch,
                                                       index_base=base, mode=native.MODE_FIRST_HIT)
                        st.rows += n_ch
                        base += n_ch
                        hit = int(fh[0])
                        if hit == native.NO_HIT:
                            native.repair_score(rep, cct, dst, row_count=n_ch)
                            src, dst = dst, src
                            continue
                    run.take(g, wrows[0], hit)
                    first_hit = hit if first_hit is None else min(first_hit, hit)
                    st.bump("repair_hits")
                    break
            finally:
                cct.close()
                st.add("repair", time.perf_counter() - tr)
        return first_hit


def newest_tape(nodes: np.ndarray, parent_len: int, hops: int = 0) -> Optional[np.ndarray]:
    """The conjunction of the conjuncts a query's root tape adds to an ancestor's: the tape of
    ``AND(...AND(parent, c1)..., ck)`` lists the parent's root tape first (linearised root by
    root, query.cpp), ending in the parent's root at ``parent_len - 1``; the right operands of
    the AND chain above it are the new conjuncts (the newest constraint's lowering and its
    congruence conjuncts).  Their AND, re-linearised over the same columns and constants;
    None when there is none.  The guide harvested from it (the parent's witness under the newest
    conjuncts' sets only) is Sieve.solve's incremental round.  ``hops`` = 1 puts the parent's
    conjuncts that read a column a new conjunct reads in front of them (their sets re-satisfy
    what the new conjuncts' sets break; measured, SIEVE_INC_HOPS)."""
    n = len(nodes)
    if parent_len <= 0 or parent_len >= n:
        return None
    op, a, bb, cc = nodes["op"], nodes["a"], nodes["b"], nodes["c"]
    AND = int(Op.AND)
    # down the root's AND chain to the parent's root (the last prefix node): the right operands
    # on the way are the new conjuncts (a hash-consed one may be a node of the prefix), each
    # flattened into its AND leaves
    tops, x = [], n - 1
    while x >= parent_len and op[x] == AND:
        tops.append(int(bb[x]))
        x = int(a[x])
    if x != parent_len - 1 or not tops:
        return None
    leaves = []
    for top in reversed(tops):
        stack = [top]
        while stack:
            y = stack.pop()
            if op[y] == AND:
                stack += [int(bb[y]), int(a[y])]
            else:
                leaves.append(y)
    if hops:
        leaves = _column_neighbours(nodes, parent_len - 1, leaves) + leaves
    ar = {int(o): ARITY[o] for o in Op}
    remap: Dict[int, int] = {}
    out: List[np.void] = []
    for leaf in leaves:
        st = [(leaf, False)]
        while st:
            x, done = st.pop()
            if x in remap:
                continue
            k = ar[int(op[x])]
            kids = (int(a[x]), int(bb[x]), int(cc[x]))[:k]
            if not done:
                st.append((x, True))
                st += [(y, False) for y in reversed(kids) if y not in remap]
                continue
            y = nodes[x].copy()
            for f, kid in zip(("a", "b", "c"), kids):
                y[f] = remap[kid]
            remap[x] = len(out)
            out.append(y)
    acc = remap[leaves[0]]
    for leaf in leaves[1:]:
        y = np.zeros((), dtype=nodes.dtype)
        y["op"], y["a"], y["b"] = AND, acc, remap[leaf]
        acc = len(out)
        out.append(y)
    return np.array(out, dtype=nodes.dtype)


def _column_neighbours(nodes: np.ndarray, parent_root: int, leaves: List[int]) -> List[int]:
    """The AND leaves under `parent_root` that read a column one of `leaves` reads."""
    op, a, bb, cc, i0 = nodes["op"], nodes["a"], nodes["b"], nodes["c"], nodes["imm0"]
    ar = {int(o): ARITY[o] for o in Op}
    VAR, AND = int(Op.VAR), int(Op.AND)

    def cols(root: int) -> set:
        out, seen, st = set(), set(), [root]
        while st:
            x = st.pop()
            if x in seen:
                continue
            seen.add(x)
            o = int(op[x])
            if o == VAR:
                out.add(int(i0[x]))
                continue
            st += [int(y) for y in (a[x], bb[x], cc[x])[:ar[o]]]
        return out

    want = set()
    for leaf in leaves:
        want |= cols(leaf)
    pl, st = [], [parent_root]
    while st:
        y = st.pop()
        if int(op[y]) == AND:
            st += [int(bb[y]), int(a[y])]
        else:
            pl.append(y)
    return [y for y in pl if cols(y) & want]


def _reads_keccak(nodes) -> bool:
    """A tape applies keccak (the default lowering's H(x), lower.py)."""
    ops = nodes["op"] if isinstance(nodes, np.ndarray) else [n[0] for n in nodes]
    return bool(np.any(np.asarray(ops) == int(Op.KECCAK)))


def _limbs(col: np.ndarray) -> int:
    return sum(int(x) << (32 * k) for k, x in enumerate(col))
