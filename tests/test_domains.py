"""mh_domains_build / mh_domains_create (csrc/domains.cpp): the domain analysis is sound against
brute force on the random 4-bit family, reads the stated shapes exactly, and the constructor
refuses every malformed array.  Host only: no device."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from mythril_amd import native, smt
from mythril_amd.smt import Not, Or, UGE, UGT, ULE, ULT, symbol_factory
from tests import decide_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAT = native.ROWS_SATURATED
TOP = (1 << 256) - 1


def build(ctx, cs):
    """The domains of the whole query as one group (the root tape), with the column names."""
    cq = native.TermMirror.of(ctx.b).build(ctx.b, [c.node for c in cs])
    return native.domains_build(cq.tapes[0], cq.consts, cq.widths, range(len(cq.names))), cq.names


def values_of(d, j):
    if d.kind[j] == native.DOMAIN_LIST:
        return set(d.lists[j])
    return set(range(d.lo[j], d.lo[j] + d.size[j]))


def test_domains_are_supersets_on_random_conjunctions():
    """Every satisfying assignment of a random conjunction over three 4-bit symbols (all 4096
    enumerated with the oracle) has every column inside its domain; the family does narrow
    domains and does produce empty ones."""
    narrowed = empty = 0
    for ctx, cs, sat in decide_cases.truth(decide_cases.SEED, decide_cases.COUNT):
        try:
            d, names = build(ctx, cs)
        except native.SieveError:
            continue
        doms = {names[c]: values_of(d, j) for j, c in enumerate(d.cols)}
        narrowed += any(len(v) < 16 for v in doms.values())
        empty += d.rows == 0
        for env in sat:
            for n, v in doms.items():
                assert env[n] in v, (n, env, sorted(v), [str(c) for c in cs])
        prod = 1
        for v in doms.values():
            prod *= len(v)
        assert d.rows == prod
        d.close()
    assert narrowed >= 80 and empty >= 5


def one(width, make):
    """The domain of column x for the conjuncts make(x, const) builds."""
    ctx = smt.set_context(smt.Context())
    x = symbol_factory.BitVecSym("x", width)
    cs = make(x, lambda v: symbol_factory.BitVecVal(v, width))
    d, names = build(ctx, cs)
    j = d.cols.index(names.index("x"))
    out = (d.kind[j], d.size[j], d.lo[j], d.lists[j], d.rows)
    d.close()
    return out


I, L = native.DOMAIN_INTERVAL, native.DOMAIN_LIST

SHAPES = [
    ("pin", 8, lambda x, c: [x == c(5)], (I, 1, 5, [])),
    ("pin mirrored", 8, lambda x, c: [c(5) == x], (I, 1, 5, [])),
    ("or of three", 8, lambda x, c: [Or(x == c(9), x == c(2), x == c(200))], (L, 3, 0, [2, 9, 200])),
    ("or with a duplicate", 8, lambda x, c: [Or(x == c(9), x == c(2), c(9) == x)],
     (L, 2, 0, [2, 9])),
    ("ult", 8, lambda x, c: [ULT(x, c(10))], (I, 10, 0, [])),
    ("ult mirrored", 8, lambda x, c: [ULT(c(10), x)], (I, 245, 11, [])),
    ("ugt and ule", 8, lambda x, c: [UGT(x, c(3)), ULE(x, c(7))], (I, 4, 4, [])),
    ("uge mirrored", 8, lambda x, c: [UGE(c(7), x)], (I, 8, 0, [])),
    ("negated bounds", 8, lambda x, c: [Not(ULT(x, c(4))), Not(UGT(x, c(5000 % 256)))],
     (I, 5000 % 256 - 4 + 1, 4, [])),
    ("negated ule form", 8, lambda x, c: [Not(ULE(x, c(4)))], (I, 251, 5, [])),
    ("list and interval", 8, lambda x, c: [Or(x == c(1), x == c(5), x == c(9)), UGT(x, c(1)),
                                           ULT(x, c(9))], (L, 1, 0, [5])),
    ("two lists", 8, lambda x, c: [Or(x == c(1), x == c(5), x == c(9)), Or(x == c(9), x == c(5))],
     (L, 2, 0, [5, 9])),
    ("ne on a list", 8, lambda x, c: [Or(x == c(1), x == c(5)), Not(x == c(5))], (L, 1, 0, [1])),
    ("ne at interval ends", 8, lambda x, c: [ULT(x, c(10)), Not(x == c(0)), Not(x == c(9)),
                                             Not(x == c(8)), Not(x == c(4))], (I, 7, 1, [])),
    ("contradicting pins", 8, lambda x, c: [x == c(1), x == c(2)], (I, 0, 0, [])),
    ("pin outside a list", 8, lambda x, c: [Or(x == c(1), x == c(5)), x == c(4)], (L, 0, 0, [])),
    ("below zero", 8, lambda x, c: [ULT(x, c(0))], (I, 0, 0, [])),
    ("above the top", 256, lambda x, c: [UGT(x, c(TOP))], (I, 0, 0, [])),
    ("pin at the top", 256, lambda x, c: [x == c(TOP)], (I, 1, TOP, [])),
    ("list at the top", 256, lambda x, c: [Or(x == c(TOP), x == c(TOP - 1))],
     (L, 2, 0, [TOP - 1, TOP])),
    ("uge near the top", 256, lambda x, c: [UGE(x, c(TOP - 2))], (I, 3, TOP - 2, [])),
    ("untouched wide column", 256, lambda x, c: [ULT(x + c(1), c(9))], (I, SAT, 0, [])),
    ("exactly 2^64 - 1 values saturate", 256, lambda x, c: [ULT(x, c((1 << 64) - 1))],
     (I, SAT, 0, [])),
    ("2^64 - 2 values do not", 256, lambda x, c: [ULT(x, c((1 << 64) - 2))],
     (I, (1 << 64) - 2, 0, [])),
    ("other shapes contribute nothing", 8, lambda x, c: [ULT(x + c(1), c(3)), Not(Or(x == c(1),
                                                                                      x == c(2)))],
     (I, 256, 0, [])),
]


@pytest.mark.parametrize("name,width,make,want", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes(name, width, make, want):
    kind, size, lo, lst, rows = one(width, make)
    assert (kind, size, lo, lst) == want
    assert rows == size


def test_product_and_saturation():
    ctx = smt.set_context(smt.Context())
    xs = [symbol_factory.BitVecSym(n, 64) for n in "abc"]
    c = lambda v: symbol_factory.BitVecVal(v, 64)  # noqa: E731
    d, _ = build(ctx, [ULT(xs[0], c(3)), Or(xs[1] == c(4), xs[1] == c(8)), ULT(xs[2], c(5)),
                       xs[0] + xs[1] == xs[2] * c(3)])
    assert sorted(d.size) == [2, 3, 5] and d.rows == 30
    d.close()
    ctx = smt.set_context(smt.Context())
    xs = [symbol_factory.BitVecSym(n, 64) for n in "abc"]
    d, _ = build(ctx, [ULT(x, c(1 << 40)) for x in xs] + [xs[0] + xs[1] == xs[2] * c(3)])
    assert d.size == [1 << 40] * 3 and d.rows == SAT  # 2^120 saturates
    d.close()
    # an empty column makes the product empty even beside a saturated one
    ctx = smt.set_context(smt.Context())
    x, y = symbol_factory.BitVecSym("x", 256), symbol_factory.BitVecSym("y", 256)
    c = lambda v: symbol_factory.BitVecVal(v, 256)  # noqa: E731
    d, _ = build(ctx, [ULT(x, c(4)), UGT(x, c(5)), x + y == c(1)])
    assert 0 in d.size and SAT in d.size and d.rows == 0
    d.close()


def test_group_columns_select_the_domains():
    ctx = smt.set_context(smt.Context())
    x, y = symbol_factory.BitVecSym("x", 8), symbol_factory.BitVecSym("y", 8)
    cs = [x == symbol_factory.BitVecVal(3, 8), ULT(y, symbol_factory.BitVecVal(4, 8)),
          x + y == symbol_factory.BitVecVal(5, 8)]
    cq = native.TermMirror.of(ctx.b).build(ctx.b, [c.node for c in cs])
    iy = cq.names.index("y")
    d = native.domains_build(cq.tapes[0], cq.consts, cq.widths, [iy])
    assert d.cols == [iy] and d.size == [4] and d.rows == 4
    d.close()
    d = native.domains_build(cq.tapes[0], cq.consts, cq.widths, [])  # a ground group
    assert d.cols == [] and d.rows == 1  # the one empty row
    d.close()


def test_build_refuses_bad_arguments():
    ctx = smt.set_context(smt.Context())
    x = symbol_factory.BitVecSym("x", 8)
    cq = native.TermMirror.of(ctx.b).build(ctx.b, [(x == symbol_factory.BitVecVal(3, 8)).node])
    nodes, consts, widths = cq.tapes[0], cq.consts, cq.widths
    with pytest.raises(native.SieveError):  # a group column outside the widths
        native.domains_build(nodes, consts, widths, [len(widths)])
    with pytest.raises(native.SieveError):  # a VAR outside the widths
        native.domains_build(nodes, consts, widths[:0])
    with pytest.raises(native.SieveError):  # a root that is not Bool
        native.domains_build(nodes[:-1], consts, widths)
    bad = nodes.copy()
    bad["a"][-1] = len(bad)  # an operand that is not an earlier node
    with pytest.raises(native.SieveError):
        native.domains_build(bad, consts, widths)
    lib = native.load()
    h = C.c_void_p()
    assert lib.mh_domains_build(None, 0, None, 0, None, 0, None, 0, C.byref(h)) \
        == native.MH_E_INVALID
    assert lib.mh_domains_info(None, None) == native.MH_E_INVALID
    assert lib.mh_domains_free(None) == native.MH_OK


GOOD = dict(cols=[1, 3], kinds=[I, L], sizes=[4, 2], los=[250, 0], lists=[[], [7, 9]],
            widths=[8, 8, 8, 8])
BAD = [
    ("columns not ascending", dict(cols=[3, 1])),
    ("column outside the widths", dict(cols=[1, 4])),
    ("list not ascending", dict(lists=[[], [9, 7]])),
    ("list with a repeat", dict(lists=[[], [7, 7]])),
    ("list value beyond the width", dict(lists=[[], [7, 256]])),
    ("list size is not its length", dict(sizes=[4, 3])),
    ("interval with list values", dict(lists=[[5], [7, 9]], sizes=[4, 2])),
    ("lo beyond the width", dict(los=[256, 0])),
    ("lo + size - 1 beyond the width", dict(sizes=[7, 2])),
    ("unknown kind", dict(kinds=[2, L])),
]


def test_create_accepts_the_good_arrays():
    d = native.domains_create(**GOOD)
    assert (d.cols, d.kind, d.size, d.lo, d.lists, d.rows) == (
        [1, 3], [I, L], [4, 2], [250, 0], [[], [7, 9]], 8)
    d.close()
    d = native.domains_create(**dict(GOOD, sizes=[6, 2]))  # lo + size - 1 == 2^w - 1 exactly
    assert d.rows == 12
    d.close()


@pytest.mark.parametrize("name,change", BAD, ids=[b[0] for b in BAD])
def test_create_refuses(name, change):
    with pytest.raises(native.SieveError) as e:
        native.domains_create(**dict(GOOD, **change))
    assert e.value.code == native.MH_E_INVALID


def test_create_refuses_null_and_empty():
    lib = native.load()
    h = C.c_void_p()
    assert lib.mh_domains_create(None, None, None, None, None, None, 1, None, 0, C.byref(h)) \
        == native.MH_E_INVALID
    with pytest.raises(native.SieveError):
        native.domains_create([], [], [], [], [], [8])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_shape_cases_under_sanitizers(tmp_path):
    """tests/native/domains_replay.cpp: domains.cpp built stand-alone with AddressSanitizer and
    UBSan, run over hand-built tapes of the shape cases (nothing is loaded into Python)."""
    exe = str(tmp_path / "domains_replay")
    src = [os.path.join(ROOT, "tests", "native", "domains_replay.cpp"),
           os.path.join(ROOT, "mythril_amd", "csrc", "domains.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g1", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-I", os.path.join(ROOT, "mythril_amd", "csrc"), *src,
                    "-o", exe], check=True, timeout=600)
    # (the runtime is linked in statically; a library the host environment preloads must not
    # make it refuse to start)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "domains_replay ok" in r.stdout
