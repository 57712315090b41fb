"""The certifier (mythril_amd/certify.py) on the device.

* Real witnesses: the planted random and LASER families at the sizes of tests/test_gpu_recall.py's
  quick case (20 paths x 16 constraint attempts, every prefix in LASER order).  Every witness the
  sieve returns certifies: those witnesses are models of the original query (the existing recall
  test checks each against the oracle), so the allowed share of false rejections is zero.
* Tampered witnesses: the hand-made ones of tests/test_certify.py are rejected, their untampered
  twins certify.
* The front end with certification on: a real query still comes back as a Model.
"""
import pytest

from mythril_amd import frontend, smt
from mythril_amd.certify import CertifyUnsupported, certify
from mythril_amd.lower import lower_query
from mythril_amd.model import Model
from mythril_amd.sieve import Sieve
from mythril_amd.smt import Array, symbol_factory
from mythril_amd.support import SolverStatistics
from tests.planted import planted_path
from tests.test_certify import _kread_case, _read_cols

pytestmark = pytest.mark.gpu
BVV, BVS = symbol_factory.BitVecVal, symbol_factory.BitVecSym


@pytest.mark.parametrize("family", ["laser", "random"])
def test_every_returned_witness_certifies(gpu_ctx, family):
    s = Sieve()
    hits, rejected, unsupported = 0, [], []
    try:
        for seed in range(20):
            ctx, cs, m, kinds = planted_path(family, seed, 16)
            nodes = [c.node for c in cs]
            for k in range(1, len(nodes) + 1):
                try:
                    w = s.solve(ctx.b, nodes[:k], key=tuple(nodes[:k]))
                except Exception:  # noqa: BLE001 - the front end falls back (the recall test's)
                    continue
                if w is None:
                    continue
                hits += 1
                model = Model(s, ctx, w.schema, w.values, w.index)
                try:
                    v = certify(model, nodes[:k])
                except CertifyUnsupported as e:
                    unsupported.append((seed, k, str(e)))
                    continue
                if not v:
                    rejected.append((seed, k, repr(v)))
    finally:
        s.close()
    print(family, "witnesses", hits, "rejected", len(rejected), "unsupported", len(unsupported))
    assert hits > 100
    assert not rejected, rejected[:5]
    assert not unsupported, unsupported[:5]


def test_tampered_witnesses_are_rejected(gpu_ctx):
    s = Sieve()
    try:
        # a read at a cell's key with another value (the r06c shape)
        ctx = smt.set_context(smt.Context())
        A = Array("A", 256, 256)
        i, c = BVS("i", 256), BVV(0x20, 256)
        cs = [A[i] == BVV(5, 256), A[c] == BVV(7, 256)]
        _, schema = lower_query(ctx.b, [x.node for x in cs])
        (read,), (cell,) = _read_cols(schema, "read"), _read_cols(schema, "cell")
        v = certify(Model(s, ctx, schema, {"i": 0x20, read: 5, cell: 7}, 0), cs)
        assert not v and v.failing == (0,)
        assert certify(Model(s, ctx, schema, {"i": 0x21, read: 5, cell: 7}, 0), cs)
        # two reads at one index with unequal read columns
        ctx = smt.set_context(smt.Context())
        A = Array("A", 256, 256)
        i, j = BVS("i", 256), BVS("j", 256)
        cs = [A[i] == BVV(5, 256), A[j] == BVV(6, 256)]
        _, schema = lower_query(ctx.b, [x.node for x in cs])
        ri, rj = _read_cols(schema, "read")
        bad = Model(s, ctx, schema, {"i": 9, "j": 9, ri: 5, rj: 6}, 0)
        assert bad.eval_many(cs, True) == [True, True]
        v = certify(bad, cs)
        assert not v and v.failing == (1,)
        assert certify(Model(s, ctx, schema, {"i": 9, "j": 10, ri: 5, rj: 6}, 0), cs)
        # two keccak reads with one image under an inverse constraint
        ctx, cs, schema, kx, ky = _kread_case(s)
        bad = Model(s, ctx, schema, {"x": 1, "y": 2, kx: 0x1000, ky: 0x1000}, 0)
        assert bad.eval_many(cs, True) == [True] * 5
        v = certify(bad, cs)
        assert not v and "maps" in v.reason
        assert certify(Model(s, ctx, schema, {"x": 1, "y": 2, kx: 0x1000, ky: 0x2000}, 0), cs)
    finally:
        s.close()


def test_unrelated_wide_symbol_does_not_fail_certification(gpu_ctx):
    """A function over 1024 bits declared in the session's context (no table can hold its keys:
    mh_tables_create refuses four key words) and forty other arrays: only the tables the
    constraints look up are uploaded, so the query certifies as without them."""
    from mythril_amd.smt import Concat, Function

    s = Sieve()
    try:
        ctx = smt.set_context(smt.Context())
        big = BVS("big", 256)
        Function("keccak256_1024", 1024, 256)(Concat(big, big, big, big))
        for k in range(40):
            Array("pad%d" % k, 256, 256)[BVV(k, 256)]
        A = Array("A", 256, 256)
        i, j = BVS("i", 256), BVS("j", 256)
        cs = [A[i] == BVV(5, 256), A[j] == BVV(6, 256)]
        _, schema = lower_query(ctx.b, [x.node for x in cs])
        ri, rj = _read_cols(schema, "read")
        assert certify(Model(s, ctx, schema, {"i": 9, "j": 10, ri: 5, rj: 6}, 0), cs)
        v = certify(Model(s, ctx, schema, {"i": 9, "j": 9, ri: 5, rj: 6}, 0), cs)
        assert not v and v.failing == (1,)
    finally:
        s.close()


def test_front_end_certifies_a_real_query(gpu_ctx):
    from tests.laser_like import queries

    frontend.reset()
    try:
        frontend.configure(certify=True, fallback=lambda *a: "z3")
        qctx, qs = queries()
        smt.set_context(qctx)
        st = SolverStatistics()
        before = (st.sieve_hits, st.sieve_rejected, st.sieve_uncertified)
        # (the keccak queries' inverses have a 512-bit range: one table per 256-bit slice)
        names = ("killbilly", "keccak_mapping", "ether_thief")
        for name in names:
            assert isinstance(frontend.get_model(tuple(dict(qs)[name])), Model), name
        assert (st.sieve_hits, st.sieve_rejected, st.sieve_uncertified) == \
            (before[0] + len(names), before[1], before[2])
    finally:
        frontend.reset()
