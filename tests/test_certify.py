"""Certification of sieve witnesses against the original constraints (mythril_amd/certify.py), on
the CPU: tests/fake_tables.py stands in for the device's table calls, tests/native/lookup_emu.cpp
runs the device's own D_LOOKUP step() on the host.

* parity with the oracle: every constraint of the planted paths has the value
  oracle/term_eval.py gives the ORIGINAL term, under the planted model and under perturbed ones;
* the shapes of witnesses the lowering's dropped conjuncts let through (VERDICT "What's weak 3"),
  by hand: rejected, while ``Model.eval_many`` accepts them;
* the front end's switch; the extensional lowering; the table lookup against its restatement.

``Model.eval_many`` accepts a tampered witness only where the violated condition is a conjunct of
the lowered query alone: congruence of two reads, injectivity of two keccak reads.  A read at a
cell's key is different: lower.py lowers ``A[i]`` to ``ite(i == c, A[c], A[@i])``, the cell
comparison is inside the term's value, so eval_many gives [False, True] for that witness too.
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from mythril_amd import frontend, smt
from mythril_amd.certify import (CertifyUnsupported, ExtModel, KeccakRule, certify,
                                 certify_values, ext_lower)
from mythril_amd.lower import lower_query
from mythril_amd.model import Model
from mythril_amd.sieve import Sieve, Witness
from mythril_amd.smt import UGT, Array, Function, Not, symbol_factory
from mythril_amd.support import SolverStatistics
from mythril_amd.tape import F_ARRAY, NODE_DTYPE, Op
from tests import fake_tables, lookup_cases
from tests.planted import planted_path

BVV, BVS = symbol_factory.BitVecVal, symbol_factory.BitVecSym
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def sieve(monkeypatch):
    fake_tables.install(monkeypatch)
    s = Sieve(rows=256)
    yield s
    s.close()


# ---- parity with the oracle ----------------------------------------------------------------------
def _planted_ext(ctx, cs, m):
    """The planted model as an ExtModel: its functions tabled at every argument the constraints
    apply them to (default 0)."""
    seen = {}
    orig = dict(m.funcs)
    for name, f in orig.items():
        def rec(x, f=f, name=name):
            y = f(x)
            seen.setdefault(name, {})[x] = y
            return y
        m.funcs[name] = rec
    try:
        assert all(m.holds(ctx, c) for c in cs)
    finally:
        m.funcs.update(orig)
    return ExtModel(dict(m.vars), {a: (dict(t), e) for a, (t, e) in m.arrays.items()},
                    {f: (dict(seen.get(f, {})), 0) for f in orig})


def _perturbed(ext, rng):
    """`ext`, and copies with one scalar, one array entry, one else value and one function value
    changed."""
    out = [("planted", ext)]

    def copy():
        return ExtModel(dict(ext.scalars), {a: (dict(t), e) for a, (t, e) in ext.arrays.items()},
                        {f: (dict(t), d) for f, (t, d) in ext.functions.items()})

    e = copy()
    name = sorted(e.scalars)[rng.randrange(len(e.scalars))]
    e.scalars[name] ^= 1 << rng.randrange(8)
    out.append(("scalar", e))
    arrs = sorted(a for a, (t, _) in ext.arrays.items() if t)
    if arrs:
        e = copy()
        a = arrs[rng.randrange(len(arrs))]
        k = sorted(e.arrays[a][0])[0]
        e.arrays[a][0][k] ^= 1
        out.append(("entry", e))
    if ext.arrays:
        e = copy()
        a = sorted(e.arrays)[rng.randrange(len(e.arrays))]
        e.arrays[a] = (e.arrays[a][0], e.arrays[a][1] ^ 1)
        out.append(("else", e))
    funcs = sorted(f for f, (t, _) in ext.functions.items() if t)
    if funcs:
        e = copy()
        f = funcs[rng.randrange(len(funcs))]
        k = sorted(e.functions[f][0])[0]
        e.functions[f][0][k] ^= 1 << 7
        out.append(("function", e))
        # ... and the keccak rule as the default of a keccak function with half its table
        kf = [f for f in funcs if f.startswith("keccak256_") and not f.endswith("-1")]
        if kf:
            e = copy()
            tab = e.functions[kf[0]][0]
            for k in sorted(tab)[::2]:
                del tab[k]
            e.functions[kf[0]] = (tab, KeccakRule(64 * rng.getrandbits(200)))
            out.append(("rule", e))
    return out


@pytest.mark.parametrize("family,seed,n", [("random", 1, 14), ("random", 5, 14), ("laser", 2, 12),
                                           ("laser", 7, 12)])
def test_certified_values_equal_the_oracle(sieve, family, seed, n):
    ctx, cs, m, _ = planted_path(family, seed, n)
    assert cs
    ext = _planted_ext(ctx, cs, m)
    nodes = [c.node for c in cs]
    verdicts = set()
    for what, e in _perturbed(ext, random.Random(seed)):
        got = certify_values(sieve, ctx.b, nodes, e)
        want = [int(fake_tables.oracle_value(e, ctx, x)) for x in nodes]
        assert got == want, (what, [i for i in range(len(nodes)) if got[i] != want[i]])
        if what == "planted":
            assert all(got)
        verdicts.add(all(got))
    assert verdicts == {True, False}  # some perturbation breaks a constraint


# ---- the witnesses the dropped conjuncts let through, by hand ---------------------------------
def _read_cols(schema, kind):
    return [c.name for c in sorted((c for c in schema.columns.values() if c.kind == kind),
                                   key=lambda c: c.key)]


def test_read_at_a_cell_key_with_another_value_is_rejected(sieve):
    """The r06c shape: A[i] == 5, A[c] == 7, witness i = c, read column 5, cell 7."""
    ctx = smt.set_context(smt.Context())
    A = Array("A", 256, 256)
    i, c = BVS("i", 256), BVV(0x20, 256)
    cs = [A[i] == BVV(5, 256), A[c] == BVV(7, 256)]
    _, schema = lower_query(ctx.b, [x.node for x in cs])
    (read,), (cell,) = _read_cols(schema, "read"), _read_cols(schema, "cell")
    bad = Model(sieve, ctx, schema, {"i": 0x20, read: 5, cell: 7}, 0)
    v = certify(bad, cs)
    assert not v and v.failing == (0,)
    # (the cell comparison is part of A[i]'s lowered value, so eval_many rejects this one too)
    assert bad.eval_many(cs, True) == [False, True]
    good = Model(sieve, ctx, schema, {"i": 0x21, read: 5, cell: 7}, 0)
    assert certify(good, cs) and good.eval_many(cs, True) == [True, True]


def test_two_reads_at_one_index_with_unequal_columns_are_rejected(sieve):
    ctx = smt.set_context(smt.Context())
    A = Array("A", 256, 256)
    i, j = BVS("i", 256), BVS("j", 256)
    cs = [A[i] == BVV(5, 256), A[j] == BVV(6, 256)]
    _, schema = lower_query(ctx.b, [x.node for x in cs])
    ri, rj = _read_cols(schema, "read")
    bad = Model(sieve, ctx, schema, {"i": 9, "j": 9, ri: 5, rj: 6}, 0)
    assert bad.eval_many(cs, True) == [True, True]  # why the feature exists
    v = certify(bad, cs)
    assert not v and v.failing == (1,)
    good = Model(sieve, ctx, schema, {"i": 9, "j": 10, ri: 5, rj: 6}, 0)
    assert good.eval_many(cs, True) == [True, True]
    assert certify(good, cs)


def _kread_case(sieve):
    ctx = smt.set_context(smt.Context())
    f = Function("keccak256_256", 256, 256)
    finv = Function("keccak256_256-1", 256, 256)
    x, y = BVS("x", 256), BVS("y", 256)
    cs = [finv(f(x)) == x, finv(f(y)) == y, Not(x == y), UGT(f(x), BVV(16, 256)),
          UGT(f(y), BVV(16, 256))]
    _, schema = lower_query(ctx.b, [c.node for c in cs], keccak_reads=True)
    kx, ky = _read_cols(schema, "kread")
    return ctx, cs, schema, kx, ky


def test_two_keccak_reads_with_one_image_are_rejected(sieve):
    ctx, cs, schema, kx, ky = _kread_case(sieve)
    bad = Model(sieve, ctx, schema, {"x": 1, "y": 2, kx: 0x1000, ky: 0x1000}, 0)
    assert bad.eval_many(cs, True) == [True] * 5  # why the feature exists
    v = certify(bad, cs)
    assert not v and "maps" in v.reason  # an injectivity failure is a rejection, not an error
    good = Model(sieve, ctx, schema, {"x": 1, "y": 2, kx: 0x1000, ky: 0x2000}, 0)
    assert good.eval_many(cs, True) == [True] * 5
    assert certify(good, cs)


def test_from_model_reads_every_table_in_one_batch(sieve):
    ctx = smt.set_context(smt.Context())
    A, B = Array("A", 256, 256), Array("B", 256, 8)
    i, j = BVS("i", 256), BVS("j", 256)
    cs = [A[i] == BVV(5, 256), B[j] == BVV(6, 8), A[BVV(3, 256)] == BVV(1, 256)]
    _, schema = lower_query(ctx.b, [x.node for x in cs])
    (ra,) = [c.name for c in schema.columns.values() if c.kind == "read" and c.symbol == "A"]
    (rb,) = [c.name for c in schema.columns.values() if c.kind == "read" and c.symbol == "B"]
    (cell,) = _read_cols(schema, "cell")
    m = Model(sieve, ctx, schema, {"i": 9, "j": 4, ra: 5, rb: 6, cell: 1}, 0)
    before = fake_tables.fake_device.LAUNCHES[0]
    tabs = m.tables()
    assert fake_tables.fake_device.LAUNCHES[0] == before + 1
    assert tabs == {"A": m.table("A"), "B": m.table("B")}
    assert tabs["A"] == ({3: 1, 9: 5}, 0) and tabs["B"] == ({4: 6}, 0)
    ext = ExtModel.from_model(m, [c.node for c in cs])
    assert ext.arrays == {"A": ({3: 1, 9: 5}, 0), "B": ({4: 6}, 0)}
    assert ext.scalars == {"i": 9, "j": 4} and not ext.rejected


def test_only_the_tables_the_terms_look_up_are_packed(sieve, monkeypatch):
    """A symbol the context declares elsewhere -- here a keccak function over 1024 bits, whose
    keys no table can hold, and forty arrays -- costs a certification nothing and cannot fail its
    table upload (tests/fake_tables.FakeTables refuses what mh_tables_create refuses)."""
    from mythril_amd import native

    ctx = smt.set_context(smt.Context())
    wide = Function("keccak256_1024", 1024, 256)
    big = symbol_factory.BitVecSym("big", 256)
    big = smt.Concat(big, big, big, big)
    unrelated = wide(big) == BVV(1, 256)
    for k in range(40):
        Array("pad%d" % k, 256, 256)[BVV(k, 256)]
    A = Array("A", 256, 256)
    i, j = BVS("i", 256), BVS("j", 256)
    cs = [A[i] == BVV(5, 256), A[j] == BVV(6, 256)]
    _, schema = lower_query(ctx.b, [x.node for x in cs])
    ri, rj = _read_cols(schema, "read")
    packed = []
    create = native.tables_create
    monkeypatch.setattr(native, "tables_create",
                        lambda c, tables: packed.append(tables) or create(c, tables))
    assert certify(Model(sieve, ctx, schema, {"i": 9, "j": 10, ri: 5, rj: 6}, 0), cs)
    assert not certify(Model(sieve, ctx, schema, {"i": 9, "j": 9, ri: 5, rj: 6}, 0), cs)
    assert [len(t) for t in packed] == [1, 1] and packed[0][0] == ({9: 5, 10: 6}, 0, 256)
    # the same set with every declared symbol in it is what the library refuses
    with pytest.raises(native.SieveError):
        create(None, [({}, 0, 256), ({}, 0, 1024)])
    with pytest.raises(CertifyUnsupported):  # a term that does use the wide function
        certify_values(sieve, ctx.b, [unrelated.node], ExtModel())


def test_a_child_query_keeps_its_parents_tapes(sieve, monkeypatch):
    """What the ctx's by-content tape cache keys on (the column count, a tape's nodes, the values
    of the constants it reads) is the same for a parent's constraints when they are certified
    again as part of a child query with new columns, a new table and new constants."""
    ctx = smt.set_context(smt.Context())
    A, B = Array("A", 256, 256), Array("B", 256, 8)
    f = Function("f", 256, 256)
    i, j = BVS("i", 256), BVS("j", 256)
    parent = [A[i] == BVV(5, 256), f(A[j]) == BVV(6, 256)]
    seen = []
    compile_ = Sieve.compile
    monkeypatch.setattr(Sieve, "compile", lambda self, ts: seen.append(ts) or compile_(self, ts))
    ext = ExtModel({"i": 1, "j": 2, "k": 3}, {"A": ({1: 5, 2: 7}, 0), "B": ({3: 9}, 0)},
                   {"f": ({7: 6}, 0)})
    assert certify_values(sieve, ctx.b, [c.node for c in parent], ext) == [1, 1]
    k = BVS("k", 256)
    child = parent + [B[k] == BVV(9, 8), A[k + BVV(77, 256)] == BVV(0, 256)]
    assert certify_values(sieve, ctx.b, [c.node for c in child], ext) == [1, 1, 1, 1]

    def keys(ts):
        consts = ts.pool.to_array()
        out = []
        for t in ts.tapes:
            cv = [consts[int(n["imm0"])].tobytes() for n in t.nodes if int(n["op"]) == int(Op.CONST)]
            out.append((ts.n_vars, t.nodes.tobytes(), tuple(cv)))
        return out

    p, c = keys(seen[0]), keys(seen[1])
    assert c[:len(p)] == p and len(c) == len(p) + 2


# ---- front end -----------------------------------------------------------------------------------
@pytest.fixture
def tampered_frontend(monkeypatch):
    """get_model over a sieve whose solve() returns the tampered two-reads witness for the
    parent query and records what parent witness a child query would be given."""
    fake_tables.install(monkeypatch)
    ctx = smt.set_context(smt.Context())
    A = Array("A", 256, 256)
    i, j = BVS("i", 256), BVS("j", 256)
    cs = (A[i] == BVV(5, 256), A[j] == BVV(6, 256))
    _, schema = lower_query(ctx.b, [x.node for x in cs])
    ri, rj = _read_cols(schema, "read")
    values = {"i": 9, "j": 9, ri: 5, rj: 6}
    seen = {}

    def solve(self, b, roots, key=None, budget_s=None):
        if len(roots) == len(cs):
            w = Witness(schema, dict(values), 0, 1)
            self.remember(key, w)  # as Sieve.solve does for a hit
            return w
        seen["parent"] = self._ancestor(key, [0] * len(key))[0]
        return None

    monkeypatch.setattr(Sieve, "solve", solve)
    frontend.reset()
    frontend.configure(fallback=lambda *a: "z3", rows=256)
    yield cs, values, seen
    frontend.reset()


def test_front_end_rejects_a_tampered_witness(tampered_frontend):
    cs, values, seen = tampered_frontend
    frontend.configure(certify=True)
    before = SolverStatistics().sieve_rejected
    hits = SolverStatistics().sieve_hits
    assert frontend.get_model(cs) == "z3"
    assert SolverStatistics().sieve_rejected == before + 1
    assert SolverStatistics().sieve_hits == hits
    # the child query is not seeded with the rejected witness
    k = BVS("k", 256)
    assert frontend.get_model(cs + (k == BVV(1, 256),)) == "z3"
    assert seen["parent"] is None


def test_front_end_without_certification_is_unchanged(tampered_frontend, monkeypatch):
    cs, values, seen = tampered_frontend
    monkeypatch.delenv("SIEVE_CERTIFY", raising=False)
    before = SolverStatistics().sieve_rejected
    m = frontend.get_model(cs)
    assert isinstance(m, Model) and m.values == values
    assert SolverStatistics().sieve_rejected == before
    k = BVS("k", 256)
    assert frontend.get_model(cs + (k == BVV(1, 256),)) == "z3"
    assert seen["parent"] == values  # today's behaviour: the witness seeds the child


def test_environment_switch_and_uncertified_counter(tampered_frontend, monkeypatch):
    cs, values, seen = tampered_frontend
    monkeypatch.setenv("SIEVE_CERTIFY", "1")
    assert frontend.certification_on()
    from mythril_amd import certify as certify_mod

    def refuse(model, terms, ext=None):
        raise CertifyUnsupported("ite over arrays")

    monkeypatch.setattr(certify_mod, "certify", refuse)
    st = SolverStatistics()
    before = (st.sieve_rejected, st.sieve_uncertified)
    assert frontend.get_model(cs) == "z3"
    assert (st.sieve_rejected, st.sieve_uncertified) == (before[0] + 1, before[1] + 1)
    frontend.configure(certify=False)  # configure() wins over the environment
    assert not frontend.certification_on()


def test_a_certification_error_is_an_error_not_a_rejection(tampered_frontend, monkeypatch):
    cs, values, seen = tampered_frontend
    frontend.configure(certify=True)
    from mythril_amd import certify as certify_mod
    from mythril_amd import native

    def broken(model, terms, ext=None):
        raise native.SieveError(native.MH_E_DEVICE, "hipMemcpyAsync: out of memory")

    monkeypatch.setattr(certify_mod, "certify", broken)
    st = SolverStatistics()
    before = (st.sieve_errors, st.sieve_rejected, st.sieve_uncertified, st.sieve_hits)
    assert frontend.get_model(cs) == "z3"  # fail closed
    assert (st.sieve_errors, st.sieve_rejected, st.sieve_uncertified, st.sieve_hits) == \
        (before[0] + 1, before[1], before[2], before[3])


# ---- extensional lowering ------------------------------------------------------------------------
def test_extensional_lowering_depends_on_the_term_only(sieve):
    ctx = smt.set_context(smt.Context())
    b = ctx.b
    A = Array("A", 256, 256)
    f = Function("f", 256, 256)
    i = BVS("i", 256)
    t = f(A[i]) == BVV(3, 256)
    A[BVV(1, 256)] = i  # a store: the array term is now store(A, 1, i)
    u = A[f(i)] == BVV(4, 256)
    low_t, low_u = ext_lower(b, t.node), ext_lower(b, u.node)
    ops = {int(o) for r in (low_t, low_u) for o in b.finish(r).nodes["op"]}
    assert int(Op.LOOKUP) in ops and not ops & {int(o) for o in
                                                 (Op.ARRAY, Op.STORE, Op.SELECT, Op.UF)}
    n_nodes = len(b.nodes)
    e1 = ExtModel({"i": 2}, {"A": ({2: 7}, 0)}, {"f": ({7: 3, 2: 1}, 0)})
    e2 = ExtModel({"i": 1}, {"A": ({1: 9}, 5)}, {"f": ({}, 4)})
    assert certify_values(sieve, b, [t.node, u.node], e1) == [1, 0]
    assert certify_values(sieve, b, [t.node, u.node], e2) == [0, 0]
    # the same nodes for both models, nothing lowered again (memoised on the builder)
    assert (ext_lower(b, t.node), ext_lower(b, u.node)) == (low_t, low_u)
    assert len(b.nodes) == n_nodes
    assert [int(fake_tables.oracle_value(e1, ctx, x.node)) for x in (t, u)] == [1, 0]


def test_ite_over_arrays_is_unsupported(sieve):
    ctx = smt.set_context(smt.Context())
    b = ctx.b
    A, B = Array("A", 256, 256), Array("B", 256, 256)
    cond = (BVS("x", 256) == BVV(1, 256)).node
    ite = b._add(Op.ITE, 256, cond, A.node, B.node, 0, 256, flags=F_ARRAY)
    sel = b.select(ite, BVS("i", 256).node)
    with pytest.raises(CertifyUnsupported):
        ext_lower(b, b.op(Op.EQ, sel, b.const(1, 256)))
    # a key wider than three words
    wide = b.symbols.function_id("g", 1024, 256)
    k = b.op(Op.CONCAT, b.op(Op.CONCAT, BVS("x", 256).node, BVS("x", 256).node),
             b.op(Op.CONCAT, BVS("i", 256).node, BVS("i", 256).node))
    with pytest.raises(CertifyUnsupported):
        ext_lower(b, b.apply("g", 1024, 256, k))
    assert wide == b.symbols.functions["g"][0]


# ---- the device's table lookup on the host ----------------------------------------------------
@pytest.fixture(scope="module")
def lookup_emu(tmp_path_factory):
    if not any(os.access(os.path.join(p, "g++"), os.X_OK)
               for p in os.environ.get("PATH", "").split(os.pathsep)):
        pytest.skip("g++ not installed")
    csrc = os.path.join(ROOT, "mythril_amd", "csrc")
    lib = str(tmp_path_factory.mktemp("lookup_emu") / "liblookup_emu.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", lib,
                    os.path.join(ROOT, "tests", "native", "lookup_emu.cpp"),
                    os.path.join(csrc, "compile.cpp")], check=True, capture_output=True)
    return C.CDLL(lib)


def _emu_eval(lib, ts, tape, soa, tables, raw=None):
    from mythril_amd import native

    nodes, offs, consts = ts.flatten()
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    consts = np.ascontiguousarray(consts, dtype=np.uint32)
    soa = np.ascontiguousarray(soa, dtype=np.uint32)
    rows = soa.shape[2]
    counts, nws, koffs, keys, voffs, vals, elses, n_keys, n_vals = raw or \
        native.pack_tables(tables)
    out = np.zeros((8, rows), dtype=np.uint32)
    feats = C.c_uint32()
    err = C.create_string_buffer(256)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    r = lib.lookup_emu_eval(p(nodes), p(offs), C.c_uint32(len(ts.tapes)), p(consts),
                            C.c_uint32(len(ts.pool.values)), C.c_uint32(ts.n_vars),
                            C.c_uint32(tape), p(soa), C.c_uint64(rows), C.c_uint32(len(tables)),
                            p(counts), p(nws), p(koffs), p(keys), C.c_uint64(n_keys), p(voffs),
                            p(vals), C.c_uint64(n_vals), p(elses), p(out), C.byref(feats), err,
                            C.c_int(256))
    vals_out = [sum(int(out[k, j]) << (32 * k) for k in range(8)) for j in range(rows)]
    return r, vals_out, feats.value, err.value.decode()


@pytest.mark.parametrize("nw", [1, 2, 3])
def test_lookup_step_matches_the_restatement(lookup_emu, nw):
    for n in lookup_cases.SIZES:
        for width in lookup_cases.WIDTHS:
            rng = lookup_cases.case_rng(nw, n, width)
            table, els = lookup_cases.make_table(rng, n, nw, width)
            keys = lookup_cases.probes(rng, table, nw, 70)
            ts = lookup_cases.lookup_tapeset(nw, width)
            soa = lookup_cases.key_soa(keys, nw)
            tabs = [(table, els, 256 * nw)]
            for tape, hit in ((0, False), (1, True)):
                r, got, feats, err = _emu_eval(lookup_emu, ts, tape, soa, tabs)
                assert r == 0, err
                assert feats & 16  # F_TABLE
                want = [fake_tables.lookup_ref(table, els, k, hit, width) for k in keys]
                assert got == want, (n, width, hit)
            if n:
                assert any(k in table for k in keys) and any(k not in table for k in keys)


def test_lookup_emulator_refuses_bad_tables(lookup_emu):
    from mythril_amd import native

    ts = lookup_cases.lookup_tapeset(1, 256)
    soa = lookup_cases.key_soa([1, 2], 1)
    raw = list(native.pack_tables([({3: 1, 5: 2}, 0, 256)]))
    keys = raw[3].copy()
    keys[0], keys[8] = 5, 3  # descending
    raw[3] = keys
    r, _, _, err = _emu_eval(lookup_emu, ts, 0, soa, [None], raw=tuple(raw))
    assert r == -1 and "ascending" in err
    # a lookup of a table the set lacks, and of a table with another key width
    r, _, _, err = _emu_eval(lookup_emu, lookup_cases.lookup_tapeset(1, 256, table=3), 0, soa,
                             [({}, 0, 256)])
    assert r == -1 and "table 3" in err
    r, _, _, err = _emu_eval(lookup_emu, ts, 0, soa, [({}, 0, 512)])
    assert r == -1 and "key words" in err


def test_stand_alone_driver_under_sanitizers(tmp_path):
    """tests/native/lookup_emu.cpp with its own main: the table validation and the LOOKUP
    compile path under AddressSanitizer + UBSan (a program run directly, nothing loaded into
    Python)."""
    import shutil

    from tests.test_host_sanitized import ENV, sanitized_build

    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    exe = str(tmp_path / "lookup_main")
    csrc = os.path.join(ROOT, "mythril_amd", "csrc")
    main_src = str(tmp_path / "lookup_main.cpp")
    with open(main_src, "w") as fh:
        fh.write('#define LOOKUP_EMU_MAIN 1\n#include "%s"\n'
                 % os.path.join(ROOT, "tests", "native", "lookup_emu.cpp"))
    sanitized_build([main_src, os.path.join(csrc, "compile.cpp")], exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    stats = dict(kv.split("=") for kv in r.stdout.split())
    assert int(stats["lookups"]) > 5000 and int(stats["refusals"]) == 7
