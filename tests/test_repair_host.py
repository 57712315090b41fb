"""The host side of the repair step without a GPU: the conjunct plan (csrc/conjuncts.cpp), the
guide's set provenance (csrc/harvest.cpp mh_harvest_set_conjuncts), both under AddressSanitizer +
UBSan in a stand-alone program, and Sieve's repair policy end to end on the CPU stand-in
(tests/repair_ref.py over tests/fake_device.py)."""
import os
import random

import numpy as np
import pytest

from mythril_amd import native
from mythril_amd.sieve import Sieve
from mythril_amd.tape import Op, TapeSet
from oracle import smt_eval as E
from tests import fake_device, repair_ref
from tests.fuzz import TapeFuzzer, interesting
from tests.laser_like import queries
from tests.repair_cases import chain_query
from tests.test_host_sanitized import CSRC, NATIVE, needs_gxx, replay, sanitized_build
from tests.test_reference_fixtures import holds_original

COPY = 0x80000000


def flatten(nodes):
    """The AND leaves of a tape's root, left to right (Sieve.conjuncts on a tape)."""
    conj, stack = [], [len(nodes) - 1]
    while stack:
        n = stack.pop()
        if int(nodes[n]["op"]) == int(Op.AND):
            stack += [int(nodes[n]["b"]), int(nodes[n]["a"])]
        else:
            conj.append(n)
    return conj


def columns_of(nodes, root):
    """The VAR columns reached from `root`."""
    from mythril_amd.tape import ARITY

    out, seen, st = set(), set(), [root]
    while st:
        x = st.pop()
        if x in seen:
            continue
        seen.add(x)
        op = Op(int(nodes[x]["op"]))
        if op == Op.VAR:
            out.add(int(nodes[x]["imm0"]))
        st += [int(nodes[x][f]) for f in ("a", "b", "c")[:ARITY[op]]]
    return sorted(out)


def fuzzed_conjunction(seed, n_leaves=7, n_vars=4):
    """(root tape nodes, pool values): Bool leaves ANDed in a random tree shape."""
    rng = random.Random(seed)
    ts = TapeSet(["v%d" % i for i in range(n_vars)])
    fz = TapeFuzzer(rng, ts, n_vars=n_vars, allow_keccak=False, max_depth=3)
    parts = [fz.boolean(3) for _ in range(n_leaves)]
    while len(parts) > 1:  # left chains, right chains and balanced trees
        i = rng.randrange(len(parts) - 1)
        parts[i:i + 2] = [fz.b.op(Op.AND, parts[i], parts[i + 1])]
    return fz.b.finish(parts[0]).nodes, ts.pool.values


def check_plan(nodes, pool, plan, group_cols, rows):
    leaves = flatten(nodes)
    cols = {n: columns_of(nodes, n) for n in set(leaves)}
    want = [n for n in leaves if cols[n] and (not group_cols or set(cols[n]) & set(group_cols))]
    assert plan.leaf.tolist() == want                       # the harvester's order, filtered
    assert plan.cols == [cols[n] for n in want]
    for t, n in zip(plan.tapes, want):
        assert columns_of(t, len(t) - 1) == cols[n]         # self-contained, columns unchanged
    for row in rows:
        vals = E.evaluate(nodes, pool, row, all_values=True)
        got = [bool(E.evaluate(t, pool, row)) for t in plan.tapes]
        assert got == [bool(vals[n]) for n in want]
        if not group_cols and len(want) == len(leaves):     # every leaf kept: the AND is the tape
            assert all(got) == bool(vals[-1])


def test_plan_on_fuzzed_conjunctions():
    rng = random.Random(7)
    built = 0
    for seed in range(40):
        nodes, pool = fuzzed_conjunction(seed)
        rows = [[interesting(rng, 256) for _ in range(4)] for _ in range(24)]
        for gc in ([], [0], [1, 3]):
            try:
                plan = native.ConjunctPlan(nodes, gc)
            except native.Unsupported:  # the fuzzer folded the conjunction to under two leaves
                leaves = flatten(nodes)
                kept = [n for n in leaves if columns_of(nodes, n)
                        and (not gc or set(columns_of(nodes, n)) & set(gc))]
                assert len(kept) < 2
                continue
            check_plan(nodes, pool, plan, gc, rows)
            built += 1
    assert built >= 60


def test_plan_on_laser_group_tapes():
    """Per group of a LASER-shaped query: the group's conjuncts, whose AND is the group's tape."""
    ctx, qs = queries()
    rng = random.Random(11)
    plans = 0
    for name in ("ether_thief", "killbilly", "balance"):
        cs = dict(qs)[name]
        cq = native.TermMirror.of(ctx.b).build(ctx.b, [c.node for c in cs])
        pool = native._ints(cq.consts)
        root = cq.tapes[0]
        widths = [int(w) for w in cq.widths]
        rows = [[interesting(rng, w) for w in widths] for _ in range(24)]
        check_plan(root, pool, native.ConjunctPlan(root), [], rows)
        plans += 1
        if len(cq.groups) < 2:
            continue
        for g, gc in enumerate(cq.groups):
            if not gc:
                continue  # a ground group reads no column: nothing to plan
            try:
                plan = native.ConjunctPlan(root, gc)
            except native.Unsupported:
                continue  # a one-conjunct group
            check_plan(root, pool, plan, gc, rows)
            for row in rows:
                assert (all(bool(E.evaluate(t, pool, row)) for t in plan.tapes)
                        == bool(E.evaluate(cq.tapes[1 + g], pool, row)))
            plans += 1
    assert plans >= 4


def test_plan_refusals():
    ctx, cs = chain_query(6)
    cq = native.TermMirror.of(ctx.b).build(ctx.b, [c.node for c in cs])
    root = cq.tapes[0]
    assert native.ConjunctPlan(root).n == 11
    assert native.ConjunctPlan(root, max_conjuncts=11).n == 11
    with pytest.raises(native.Unsupported):      # more leaves than max_conjuncts: no grouping
        native.ConjunctPlan(root, max_conjuncts=10)
    one = native.ConjunctPlan(root, [0])         # x0's equality and its one disequality
    assert one.n == 2 and all(0 in c for c in one.cols)
    ctx1, cs1 = chain_query(1)
    cq1 = native.TermMirror.of(ctx1.b).build(ctx1.b, [c.node for c in cs1])
    with pytest.raises(native.Unsupported):      # fewer than two kept leaves
        native.ConjunctPlan(cq1.tapes[0])
    with pytest.raises(native.Unsupported):      # no leaf reads the column
        native.ConjunctPlan(root, [len(cq.names)])
    lib = native.load()
    assert lib.mh_conjuncts_build(None, 0, None, 0, 8, None, None) == native.MH_E_INVALID
    assert lib.mh_harvest_set_conjuncts(None, None, 0) == native.MH_E_INVALID


def _query(name):
    if name == "chain6":
        ctx, cs = chain_query(6)
    else:
        ctx, qs = queries()
        cs = dict(qs)[name]
    cq = native.TermMirror.of(ctx.b).build(ctx.b, [c.node for c in cs])
    return cq


@pytest.mark.parametrize("name", ["chain6", "ether_thief"])
def test_set_tags(name):
    cq = _query(name)
    root, widths = cq.tapes[0], [int(w) for w in cq.widths]
    plain = native.harvest_guide(root, cq.consts, widths)
    h = native.harvest_guide(root, cq.consts, widths, keep=True)
    try:
        tags = h.set_conjuncts()
        arrays = h.arrays()
    finally:
        h.close()
    for k in plain:                                   # the accessor leaves the guide as it was
        assert np.array_equal(plain[k], arrays[k]), k
    n_sets = len(arrays["set_off"]) - 1
    assert len(tags) == n_sets
    plan = native.ConjunctPlan(root)
    ords = plan.set_ordinals(tags)
    assert set(int(t) for t in tags if t != native.NO_CONJUNCT) <= set(plan.leaf.tolist())
    tagged = 0
    value_ords = []
    for j in range(n_sets):
        if ords[j] == native.NO_CONJUNCT:
            continue
        tagged += 1
        copy = False
        for a in range(int(arrays["set_off"][j]), int(arrays["set_off"][j + 1])):
            for e in range(int(arrays["alt_off"][a]), int(arrays["alt_off"][a + 1])):
                col = int(arrays["entry_col"][e])
                copy = copy or bool(col & COPY)
                assert (col & ~COPY) in plan.cols[ords[j]], (j, col)  # only its conjunct's columns
        if not copy:
            value_ords.append(int(ords[j]))
    assert tagged > 0
    assert value_ords == sorted(value_ords)           # sets come in the plan's leaf order
    if name == "chain6":
        # every conjunct inverts (x ^ A == K gives x, x != y gives a value apart): one inversion
        # set each at the default probability, all tagged
        inv = [int(ords[j]) for j in range(n_sets)
               if ords[j] != native.NO_CONJUNCT and int(arrays["set_prob"][j]) == 208]
        assert sorted(set(inv)) == list(range(11))


@needs_gxx
def test_plan_and_tags_under_asan_ubsan(tmp_path):
    """conjuncts.cpp and harvest.cpp (with the tag accessor) sanitized, driven by a stand-alone
    program (tests/native/repair_replay.cpp) over recorded root tapes: the chain queries and
    LASER-shaped ones, with a group's columns each."""
    recs = []
    for name in ("chain6", "ether_thief", "killbilly", "selector"):
        cq = _query(name)
        gc = cq.groups[-1] if len(cq.groups) > 1 else [0]
        recs.append((cq.tapes[0], cq.consts, cq.widths, gc))
    for seed in range(6):
        nodes, pool = fuzzed_conjunction(seed)
        consts = native._limb_rows(pool) if len(pool) else np.zeros((0, 8), np.uint32)
        recs.append((nodes, consts, [256] * 4, [seed % 4]))
    words = [np.array([len(recs)], dtype="<u4")]
    for nodes, consts, widths, gc in recs:
        nodes = np.ascontiguousarray(nodes, dtype=native.NODE_DTYPE)
        words += [np.array([len(nodes), len(consts), len(widths), len(gc)], dtype="<u4"),
                  np.frombuffer(nodes.tobytes(), dtype="<u4"),
                  np.ascontiguousarray(consts, dtype="<u4").ravel(),
                  np.asarray(widths, dtype="<u4"), np.asarray(gc, dtype="<u4")]
    data = str(tmp_path / "tapes.bin")
    with open(data, "wb") as f:
        f.write(np.concatenate(words).tobytes())
    exe = str(tmp_path / "repair_replay")
    sanitized_build([os.path.join(CSRC, "conjuncts.cpp"), os.path.join(CSRC, "harvest.cpp"),
                     os.path.join(NATIVE, "repair_replay.cpp")], exe)
    stats = replay(exe, data)
    assert int(stats["records"]) == len(recs) and int(stats["guides"]) == len(recs)
    assert int(stats["plans"]) >= len(recs) and int(stats["tagged"]) > 20


# ---- the policy on the stand-in -----------------------------------------------------------------
CHAIN_SIEVE = dict(rows=256, first_rows=256, max_rounds=1, keccak_second_chance=False,
                   budget_s=600.0)        # the stand-in is slow: no budget cut
REPAIR = dict(repair_rounds=8, repair_elites=8, repair_children=8)


def solve_chain(m, **kw):
    ctx, cs = chain_query(m)
    s = Sieve(**dict(CHAIN_SIEVE, **kw))
    try:
        w = s.solve(ctx.b, [c.node for c in cs])
        return ctx, cs, w, s.stats.extra.copy(), dict(s.last_rounds)
    finally:
        s.close()


def test_chain_misses_without_repair_and_hits_with_it(monkeypatch):
    repair_ref.install(monkeypatch)
    _, _, w, extra, lr = solve_chain(6)
    assert w is None
    assert not [k for k in extra if k.startswith("repair")] and "repair" not in lr
    ctx, cs, w, extra, lr = solve_chain(6, **REPAIR)
    assert w is not None and w.repaired
    assert holds_original(ctx, cs, w.schema, w.values)
    assert extra["repair_tries"] == 1 and extra["repair_hits"] == 1
    assert 1 <= extra["repair_iters"] <= REPAIR["repair_rounds"] and lr["repair"] >= 1


def test_repair_env_override(monkeypatch):
    repair_ref.install(monkeypatch)
    monkeypatch.setenv("SIEVE_REPAIR", "8")
    monkeypatch.setenv("SIEVE_REPAIR_ELITES", "8")
    monkeypatch.setenv("SIEVE_REPAIR_CHILDREN", "8")
    _, _, w, extra, _ = solve_chain(6)
    assert w is not None and w.repaired and extra["repair_hits"] == 1


def test_far_rows_are_not_repaired(monkeypatch):
    """A first score whose best row fails more conjuncts than SIEVE_REPAIR_MAX_FAIL stops the
    group at once (M = 12: the best of the 256 rows fails 8 of 23)."""
    repair_ref.install(monkeypatch)
    monkeypatch.setenv("SIEVE_REPAIR_MAX_FAIL", "4")
    _, _, w, extra, lr = solve_chain(12, **REPAIR)
    assert w is None and extra.get("repair_far") == 1 and lr["repair"] == 0


@pytest.mark.parametrize("name", ["selector", "owner_check", "balance", "keccak_mapping",
                                  "keccak_alias", "ether_thief", "overflow", "killbilly",
                                  "unsat_actor"])
def test_default_is_unchanged(monkeypatch, name):
    """repair_rounds=0 (the default): the witnesses of tests/test_sieve_solve.py's shapes are
    those of a sieve without the repair functions at all, and no repair_* stat appears."""
    def run(with_repair_fns):
        mp = pytest.MonkeyPatch()
        try:
            fake_device.install(mp)
            if not with_repair_fns:  # any call into the repair step would fail
                for fn in ("repair_open", "repair_score", "repair_select", "repair_mutate",
                           "ConjunctPlan"):
                    mp.delattr(native, fn)
            else:
                repair_ref.install(mp)
            ctx, qs = queries()
            cs = dict(qs)[name]
            s = Sieve(rows=256)
            assert s.repair_rounds == 0
            nodes = [c.node for c in cs]
            out = []
            for k in range(1, len(nodes) + 1):
                w = s.solve(ctx.b, nodes[:k], key=tuple(nodes[:k]))
                out.append(None if w is None else (w.values, w.index, w.rounds, w.repaired))
            extra = dict(s.stats.extra)
            s.close()
            return out, extra, dict(s.last_rounds)
        finally:
            mp.undo()

    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    assert not [k for k in a[1] if k.startswith("repair")] and "repair" not in a[2]
