"""certify.Certifier on the CPU (tests/fake_jobs.py stands in for the device): certify_many equals
certify per entry on the planted paths and tampered models of tests/test_certify.py; a child
query after its parent compiles at most one chunk; the LRU closes what it evicts; with
certification on, prefetch certifies its witnesses in one jobs submission and sieve_model uses
the parked verdicts; certify_resident routes sieve_model's own certification through the sieve's
Certifier, and off it calls certify.certify as before."""
import random
import types

import pytest

from mythril_amd import certify as certify_mod
from mythril_amd import frontend, smt
from mythril_amd.certify import (CHUNK_ROOTS, Certifier, CertifyUnsupported, ExtModel, Verdict,
                                 certify)
from mythril_amd.lower import lower_query
from mythril_amd.model import Model
from mythril_amd.sieve import Sieve, Witness
from mythril_amd.smt import Array, Function, symbol_factory
from mythril_amd.support import SolverStatistics
from tests import fake_jobs
from tests.planted import planted_path
from tests.test_certify import _kread_case, _perturbed, _planted_ext, _read_cols

BVV, BVS = symbol_factory.BitVecVal, symbol_factory.BitVecSym


@pytest.fixture
def sieve(monkeypatch):
    fake_jobs.install(monkeypatch)
    s = Sieve(rows=256)
    yield s
    s.close()


def _same(got, want):
    assert isinstance(got, Verdict), got
    assert (bool(got), got.failing, got.reason) == (bool(want), want.failing, want.reason)


@pytest.mark.parametrize("family,seed,n", [("random", 1, 14), ("random", 5, 14), ("laser", 2, 12),
                                           ("laser", 7, 12)])
def test_certify_many_equals_certify_on_planted_and_perturbed_models(sieve, family, seed, n):
    """One scalar, array entry, else value or function value changed, and the keccak rule."""
    ctx, cs, m, _ = planted_path(family, seed, n)
    ext = _planted_ext(ctx, cs, m)
    cases = _perturbed(ext, random.Random(seed))
    model = types.SimpleNamespace(ctx=ctx, sieve=sieve)
    want = [certify(model, cs, ext=e) for _, e in cases]
    before = fake_jobs.SUBMISSIONS[0]
    got = sieve.certifier().certify_many([model] * len(cases), [cs] * len(cases),
                                         [e for _, e in cases])
    assert fake_jobs.SUBMISSIONS[0] == before + 1  # every model's jobs in one submission
    for g, w in zip(got, want):
        _same(g, w)
    assert {bool(g) for g in got} == {True, False}
    assert got[0] and not got[0].failing  # the planted model itself


def test_models_from_witnesses_injectivity_and_unsupported_entries(sieve):
    """Sieve Models (ExtModel.from_model): the two-reads witness, the keccak reads with one image
    (an ext.rejected model is a rejection verdict), and a model that cannot be judged is an
    entry of its own, not an error of the call."""
    ctx = smt.set_context(smt.Context())
    A = Array("A", 256, 256)
    i, j = BVS("i", 256), BVS("j", 256)
    cs = [A[i] == BVV(5, 256), A[j] == BVV(6, 256)]
    _, schema = lower_query(ctx.b, [x.node for x in cs])
    ri, rj = _read_cols(schema, "read")
    bad = Model(sieve, ctx, schema, {"i": 9, "j": 9, ri: 5, rj: 6}, 0)
    good = Model(sieve, ctx, schema, {"i": 9, "j": 10, ri: 5, rj: 6}, 0)
    wide = Function("keccak256_1024", 1024, 256)
    big = BVS("big", 256)
    unsupported = [wide(smt.Concat(big, big, big, big)) == BVV(1, 256)]
    got = sieve.certifier().certify_many([bad, good, good, good],
                                         [cs, cs, unsupported, [i + j]])
    _same(got[0], certify(bad, cs))
    assert got[0].failing == (1,)
    _same(got[1], certify(good, cs))
    assert got[1]
    assert isinstance(got[2], CertifyUnsupported) and isinstance(got[3], CertifyUnsupported)
    with pytest.raises(CertifyUnsupported):
        sieve.certifier().certify(good, unsupported)
    kctx, kcs, kschema, kx, ky = _kread_case(sieve)
    clash = Model(sieve, kctx, kschema, {"x": 1, "y": 2, kx: 0x1000, ky: 0x1000}, 0)
    fine = Model(sieve, kctx, kschema, {"x": 1, "y": 2, kx: 0x1000, ky: 0x2000}, 0)
    stats = dict(sieve.certifier().stats)
    got = sieve.certifier().certify_many([clash, fine], [kcs, kcs])
    after = sieve.certifier().stats
    # both models' forward applications in one inverse submission; the clash is found there, so
    # only the other model's constraints are evaluated
    assert after["inverse_submissions"] == stats["inverse_submissions"] + 1
    assert after["submissions"] == stats["submissions"] + 1
    _same(got[0], certify(clash, kcs))
    assert not got[0] and "maps" in got[0].reason
    _same(got[1], certify(fine, kcs))
    assert got[1]


def _long_path(n):
    ctx = smt.set_context(smt.Context())
    A = Array("A", 256, 256)
    xs = [BVS("x%d" % k, 256) for k in range(n)]
    cs = [A[x] == BVV(k + 1, 256) if k % 3 == 0 else x + BVV(k, 256) == BVV(2 * k, 256)
          for k, x in enumerate(xs)]
    ext = ExtModel({"x%d" % k: k for k in range(n)}, {"A": ({k: k + 1 for k in range(n)}, 0)}, {})
    return ctx, cs, ext


def test_a_child_query_compiles_at_most_one_chunk(sieve, monkeypatch):
    n = 2 * CHUNK_ROOTS + 5
    ctx, cs, ext = _long_path(n + 40)
    model = types.SimpleNamespace(ctx=ctx, sieve=sieve)
    compiled = []
    compile_ = Sieve.compile
    monkeypatch.setattr(Sieve, "compile", lambda self, ts: compiled.append(len(ts.tapes)) or
                        compile_(self, ts))
    c = sieve.certifier()
    _same(c.certify(model, cs[:n], ext), certify(model, cs[:n], ext=ext))
    compiled.clear()
    assert c.certify(model, cs[:n], ext)
    assert compiled == []  # the same query again: everything resident
    # children: one more constraint at a time compiles the last chunk only; a child that starts
    # a new chunk compiles that one alone
    for k in range(n + 1, n + 32):
        compiled.clear()
        v = c.certify(model, cs[:k], ext)
        assert v and len(compiled) <= 1, (k, compiled)
        assert compiled == [k - k // CHUNK_ROOTS * CHUNK_ROOTS or CHUNK_ROOTS]
    # a failing constraint deep in a resident chunk is found at its own index
    broken = ExtModel(dict(ext.scalars, x40=41), ext.arrays, ext.functions)
    compiled.clear()
    v = c.certify(model, cs[:n], broken)
    _same(v, certify(model, cs[:n], ext=broken))
    assert not v and v.failing == (40,)


def test_the_lru_closes_what_it_evicts(sieve, monkeypatch):
    monkeypatch.setattr(certify_mod, "CHUNK_CACHE", 3)
    ctx, cs, ext = _long_path(6 * CHUNK_ROOTS)
    model = types.SimpleNamespace(ctx=ctx, sieve=sieve)
    c = Certifier(sieve)
    closed = []
    assert c.certify(model, cs[:2 * CHUNK_ROOTS], ext)
    first = list(c.chunks.values())
    assert len(first) == 2
    for ch in first:
        ct = ch.ct
        monkeypatch.setattr(ct, "close", lambda ct=ct: closed.append(ct))
    assert c.certify(model, cs[2 * CHUNK_ROOTS:5 * CHUNK_ROOTS], ext)
    assert len(c.chunks) == 3 and [ch.ct for ch in first] == [None, None]
    assert len(closed) == 2 and closed[0] is not closed[1]  # each evicted tape set closed once
    compiles = c.stats["chunk_compiles"]
    assert c.certify(model, cs[:CHUNK_ROOTS], ext)  # evicted: compiled again
    assert c.stats["chunk_compiles"] == compiles + 1
    c.close()
    assert not c.chunks


# ---- front end -----------------------------------------------------------------------------------
@pytest.fixture
def two_reads(monkeypatch):
    """N queries A[i] == 5, A[j] == v over one context, answered by a stand-in solve_many: query
    0 with the tampered two-reads witness (i = j, unequal read columns), the others honestly."""
    fake_jobs.install(monkeypatch)
    ctx = smt.set_context(smt.Context())
    A = Array("A", 256, 256)
    i, j = BVS("i", 256), BVS("j", 256)
    css = [(A[i] == BVV(5, 256), A[j] == BVV(6 + q, 256)) for q in range(4)]
    wit = {}
    for q, cs in enumerate(css):
        _, schema = lower_query(ctx.b, [t.node for t in cs])
        ri, rj = _read_cols(schema, "read")
        wit[tuple(t.node for t in cs)] = (schema, {"i": 9, "j": 9 if q == 0 else 10 + q, ri: 5,
                                                   rj: 6 + q})

    def solve_many(self, b, queries, keys=None, budget_s=None):
        out = []
        for key in keys:
            schema, values = wit[key]
            w = Witness(schema, dict(values), 0, 1)
            self.remember(key, w)  # as solve_many does for a hit
            out.append(w)
        self.last_many = [dict(miss=None, rounds={"rounds": 1}, error=None) for _ in keys]
        return out

    def solve(self, b, roots, key=None, budget_s=None):
        schema, values = wit[key]
        w = Witness(schema, dict(values), 0, 1)
        self.remember(key, w)
        return w

    monkeypatch.setattr(Sieve, "solve_many", solve_many)
    monkeypatch.setattr(Sieve, "solve", solve)
    frontend.reset()
    frontend.configure(fallback=lambda *a: "z3", rows=256)
    yield css
    frontend.reset()


def test_prefetch_certifies_in_one_submission_and_parks_the_verdicts(two_reads, monkeypatch):
    css = two_reads
    frontend.configure(certify=True)
    seen = []
    monkeypatch.setattr(certify_mod, "certify", lambda *a, **k: seen.append(a) or Verdict(True))
    before = fake_jobs.SUBMISSIONS[0]
    assert frontend.prefetch(css) == 4
    # the table asks of the four witnesses in one submission, their constraints in one more:
    # not four of each, and no inverse submission without an inverse
    assert fake_jobs.SUBMISSIONS[0] == before + 2
    stats = frontend.sieve().certifier().stats
    assert (stats["ask_submissions"], stats["inverse_submissions"], stats["submissions"]) == \
        (1, 0, 1)
    keys = [tuple(t.node for t in cs) for cs in css]
    s = frontend.sieve()
    # the rejected witness is dropped when the verdict is known; the others stay
    assert keys[0] not in s.witnesses and all(k in s.witnesses for k in keys[1:])
    st = SolverStatistics()
    rejected, hits = st.sieve_rejected, st.sieve_hits
    assert frontend.get_model(css[0]) == "z3"  # the bad parked witness reaches the fallback
    assert (st.sieve_rejected, st.sieve_hits) == (rejected + 1, hits)
    for cs in css[1:]:
        m = frontend.get_model(cs)
        assert isinstance(m, Model) and m.values["i"] == 9
    assert (st.sieve_rejected, st.sieve_hits) == (rejected + 1, hits + 3)
    assert seen == [] and fake_jobs.SUBMISSIONS[0] == before + 2  # nothing was certified again
    assert not frontend._parked() and not frontend._parked_verdicts()


def test_an_unjudged_parked_witness_counts_as_uncertified(two_reads, monkeypatch):
    css = two_reads
    frontend.configure(certify=True)
    monkeypatch.setattr(Certifier, "certify_many",
                        lambda self, models, terms: [CertifyUnsupported("ite over arrays")])
    assert frontend.prefetch(css[1:2]) == 1
    st = SolverStatistics()
    before = (st.sieve_rejected, st.sieve_uncertified, st.sieve_errors)
    assert frontend.get_model(css[1]) == "z3"
    assert (st.sieve_rejected, st.sieve_uncertified, st.sieve_errors) == \
        (before[0] + 1, before[1] + 1, before[2])


def test_a_certification_error_in_prefetch_leaves_todays_path(two_reads, monkeypatch):
    from mythril_amd import native

    css = two_reads
    frontend.configure(certify=True)

    def broken(self, models, terms):
        raise native.SieveError(native.MH_E_DEVICE, "hipMemcpyAsync: out of memory")

    monkeypatch.setattr(Certifier, "certify_many", broken)
    assert frontend.prefetch(css) == 4  # the answers stay parked, unverdicted
    assert len(frontend._parked()) == 4 and not frontend._parked_verdicts()
    key = tuple(t.node for t in css[0])
    assert key in frontend.sieve().witnesses
    st = SolverStatistics()
    rejected = st.sieve_rejected
    assert frontend.get_model(css[0]) == "z3"  # certified now, by certify(), and rejected
    assert st.sieve_rejected == rejected + 1
    assert isinstance(frontend.get_model(css[1]), Model)


def test_configure_clears_the_parked_verdicts(two_reads):
    css = two_reads
    frontend.configure(certify=True)
    assert frontend.prefetch(css) == 4 and len(frontend._parked_verdicts()) == 4
    frontend.configure(enabled=True)
    assert not frontend._parked() and not frontend._parked_verdicts()
    assert frontend.prefetch(css) == 4
    frontend.forget_witnesses()
    assert not frontend._parked_verdicts()


def test_certify_resident_switch(two_reads, monkeypatch):
    css = two_reads
    frontend.configure(certify=True)
    assert not frontend.certify_resident_on()
    seen = []
    real = certify_mod.certify
    monkeypatch.setattr(certify_mod, "certify",
                        lambda m, terms, ext=None: seen.append(len(terms)) or real(m, terms, ext))
    before = fake_jobs.SUBMISSIONS[0]
    st = SolverStatistics()
    rejected = st.sieve_rejected
    assert frontend.get_model(css[0]) == "z3" and isinstance(frontend.get_model(css[1]), Model)
    assert seen == [2, 2] and fake_jobs.SUBMISSIONS[0] == before  # off: certify.certify, as before
    assert st.sieve_rejected == rejected + 1
    frontend.get_model.cache_clear()
    frontend.configure(certify_resident=True)
    assert frontend.certify_resident_on()
    assert frontend.get_model(css[0]) == "z3" and isinstance(frontend.get_model(css[1]), Model)
    # on: the sieve's Certifier (per model one table-ask and one certify submission)
    assert seen == [2, 2] and fake_jobs.SUBMISSIONS[0] == before + 4
    assert st.sieve_rejected == rejected + 2
    assert frontend.sieve().certifier().stats["chunk_compiles"] == 2
    frontend.configure(certify_resident=False)
    monkeypatch.setenv("SIEVE_CERTIFY_RESIDENT", "1")
    assert not frontend.certify_resident_on()  # configure() wins over the environment
    frontend.reset()
    assert frontend.certify_resident_on()
