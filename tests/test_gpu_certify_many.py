"""certify.Certifier on the device: every witness the sieve returns on the planted LASER and random
families (the sizes of tests/test_gpu_certify.py: 20 paths x 16 constraint attempts, every prefix)
gets the same verdict from certify_many -- a path's witnesses in one call, so a prefix finds its
parent's chunks resident -- as from certify; the tampered witnesses of tests/test_certify.py are
rejected with certify's failing indices; 16 certifications of lookup-only queries are one
table-ask and one certify submission."""
import pytest

from mythril_amd import native, smt
from mythril_amd.certify import CertifyUnsupported, Verdict, certify
from mythril_amd.lower import lower_query
from mythril_amd.model import Model
from mythril_amd.sieve import Sieve
from mythril_amd.smt import Array, symbol_factory
from tests.planted import planted_path
from tests.test_certify import _kread_case, _read_cols

pytestmark = pytest.mark.gpu
BVV, BVS = symbol_factory.BitVecVal, symbol_factory.BitVecSym


def _same(got, want):
    assert isinstance(got, Verdict), got
    assert (bool(got), got.failing, got.reason) == (bool(want), want.failing, want.reason)


@pytest.mark.parametrize("family", ["laser", "random"])
def test_every_returned_witness_gets_certifys_verdict(gpu_ctx, family):
    s = Sieve()
    hits, differ, rejected = 0, [], []
    try:
        for seed in range(20):
            ctx, cs, m, kinds = planted_path(family, seed, 16)
            nodes = [c.node for c in cs]
            models, terms = [], []
            for k in range(1, len(nodes) + 1):
                try:
                    w = s.solve(ctx.b, nodes[:k], key=tuple(nodes[:k]))
                except Exception:  # noqa: BLE001 - the front end falls back (the recall test's)
                    continue
                if w is not None:
                    models.append(Model(s, ctx, w.schema, w.values, w.index))
                    terms.append(nodes[:k])
            got = s.certifier().certify_many(models, terms)
            assert len(got) == len(models)
            for model, t, g in zip(models, terms, got):
                hits += 1
                try:
                    want = certify(model, t)
                except CertifyUnsupported as e:
                    want = e
                if isinstance(want, Exception) or isinstance(g, Exception):
                    if type(want) is not type(g):
                        differ.append((seed, len(t), repr(g), repr(want)))
                elif (bool(g), g.failing, g.reason) != (bool(want), want.failing, want.reason):
                    differ.append((seed, len(t), repr(g), repr(want)))
                elif not g:
                    rejected.append((seed, len(t), repr(g)))
        st = s.certifier().stats
    finally:
        s.close()
    print(family, "witnesses", hits, "rejected", len(rejected), "chunks compiled",
          st["chunk_compiles"], "found resident", st["chunk_hits"])
    assert hits > 100
    assert not differ, differ[:5]
    assert not rejected, rejected[:5]  # (real witnesses: certify rejects none either)


def test_tampered_witnesses_are_rejected_in_one_call(gpu_ctx):
    s = Sieve()
    try:
        models, terms = [], []
        ctx = smt.set_context(smt.Context())
        A = Array("A", 256, 256)
        i, c = BVS("i", 256), BVV(0x20, 256)
        cs = [A[i] == BVV(5, 256), A[c] == BVV(7, 256)]
        _, schema = lower_query(ctx.b, [x.node for x in cs])
        (read,), (cell,) = _read_cols(schema, "read"), _read_cols(schema, "cell")
        for iv in (0x20, 0x21):  # a read at a cell's key with another value, and its honest twin
            models.append(Model(s, ctx, schema, {"i": iv, read: 5, cell: 7}, 0))
            terms.append(cs)
        ctx = smt.set_context(smt.Context())
        A = Array("A", 256, 256)
        i, j = BVS("i", 256), BVS("j", 256)
        cs = [A[i] == BVV(5, 256), A[j] == BVV(6, 256)]
        _, schema = lower_query(ctx.b, [x.node for x in cs])
        ri, rj = _read_cols(schema, "read")
        for jv in (9, 10):  # two reads at one index with unequal read columns
            models.append(Model(s, ctx, schema, {"i": 9, "j": jv, ri: 5, rj: 6}, 0))
            terms.append(cs)
        ctx, cs, schema, kx, ky = _kread_case(s)
        for img in (0x1000, 0x2000):  # two keccak reads with one image under an inverse
            models.append(Model(s, ctx, schema, {"x": 1, "y": 2, kx: 0x1000, ky: img}, 0))
            terms.append(cs)
        got = s.certifier().certify_many(models, terms)
        for model, t, g in zip(models, terms, got):
            _same(g, certify(model, t))
        assert [bool(g) for g in got] == [False, True, False, True, False, True]
        assert got[0].failing == (0,) and got[2].failing == (1,) and "maps" in got[4].reason
    finally:
        s.close()


def test_16_certifications_are_one_certification_submission(gpu_ctx, monkeypatch):
    """16 short lookup-only queries: one table-ask submission (the models' read indices as
    table-free jobs), no inverse submission, and one certify submission whose table sets go up in
    one mh_tables_create_many; one launch per kernel variant among the jobs' tapes, whatever the
    number of models; a second round over the same queries compiles no chunk."""
    s = Sieve()
    try:
        ctx = smt.set_context(smt.Context())
        A = Array("A", 256, 256)
        i, j = BVS("i", 256), BVS("j", 256)
        models, terms = [], []
        for q in range(16):
            cs = [A[i] == BVV(5, 256), A[j] == BVV(6 + q, 256)]
            _, schema = lower_query(ctx.b, [x.node for x in cs])
            ri, rj = _read_cols(schema, "read")
            models.append(Model(s, ctx, schema, {"i": 9, "j": 9 if q % 4 == 0 else 10 + q, ri: 5,
                                                 rj: 6 + q}, 0))
            terms.append(cs)
        c = s.certifier()
        calls = {"jobs": 0, "many": 0, "launches": 0}
        jobs_, many_ = native.eval_values_jobs, native.tables_create_many

        def count_jobs(ctx_, jobs):
            calls["jobs"] += 1
            assert len(jobs) == 16
            before = native.eval_launches(ctx_)
            out = jobs_(ctx_, jobs)
            calls["launches"] += native.eval_launches(ctx_) - before
            return out

        def count_many(ctx_, sets):
            calls["many"] += 1
            return many_(ctx_, sets)

        monkeypatch.setattr(native, "eval_values_jobs", count_jobs)
        monkeypatch.setattr(native, "tables_create_many", count_many)
        got = c.certify_many(models, terms)
        assert (calls["jobs"], calls["many"]) == (2, 1)
        assert (c.stats["ask_submissions"], c.stats["inverse_submissions"],
                c.stats["submissions"]) == (1, 0, 1)
        assert 2 <= calls["launches"] <= 4  # per kernel variant of a submission, not per model
        assert [bool(g) for g in got] == [q % 4 != 0 for q in range(16)]
        compiled = c.stats["chunk_compiles"]
        again = c.certify_many(models, terms)
        assert c.stats["chunk_compiles"] == compiled and calls["jobs"] == 4
        for g, a, model, t in zip(got, again, models, terms):
            _same(g, certify(model, t))
            _same(a, g)
    finally:
        s.close()
