"""Table shapes, probe keys and tapes for the D_LOOKUP tests (test helper): shared by the host
emulator test (tests/test_certify.py) and the device tests (tests/test_gpu_lookup.py), both
checked against tests/fake_tables.lookup_ref.

Tables of 0, 1, 2, 3, 64 and 65 entries with keys of 1, 2 and 3 words; keys that differ only in
limb 0 and only in the top limb of the top word (a compare that starts at the wrong end orders
them wrongly); probes below the first entry, above the last, equal to the first and the last and
between neighbours.
"""
import random

import numpy as np

from mythril_amd.tape import Op, TapeSet

SIZES = (0, 1, 2, 3, 64, 65)
WIDTHS = (8, 160, 256)


def make_table(rng, n, nw, width):
    """({key: value}, else value) with n entries, keys of nw 256-bit words."""
    bits = 256 * nw
    keys = set()
    if n >= 2:  # a pair that differs only in limb 0, a pair only in the top limb of the top word
        base = rng.getrandbits(bits) & ~0xFFFFFFFF & ~(0xFFFFFFFF << (bits - 32))
        keys.update((base | 5, base | 9))
        if n >= 4:
            keys.update((base | 5 | (3 << (bits - 32)), base | 5 | (2 << (bits - 32))))
    while len(keys) < n:
        keys.add(rng.getrandbits(bits) if rng.random() < 0.5 else rng.getrandbits(40))
    keys = sorted(keys)[:n] if len(keys) > n else sorted(keys)
    mask = (1 << width) - 1
    return {k: rng.getrandbits(256) & mask for k in keys}, rng.getrandbits(256) & mask


def probes(rng, table, nw, n_rows):
    """n_rows keys: the edges and neighbours of `table`'s keys first, then random hits / misses;
    every row a different key where the key space allows."""
    top = (1 << (256 * nw)) - 1
    ks = sorted(table)
    out = [0, top]
    if ks:
        out += [ks[0], ks[-1], max(ks[0] - 1, 0), min(ks[-1] + 1, top)]
        out += rng.sample(ks, min(len(ks), max(n_rows // 4, 1)))  # hits in the middle
        for a, b in zip(ks, ks[1:]):
            out += [a + (b - a) // 2, a + 1, b - 1]
        out += [k ^ 1 for k in ks[:8]] + [k ^ (1 << (256 * nw - 1)) for k in ks[:8]]
    seen, uniq = set(), []
    for k in out:
        if k not in seen:
            seen.add(k)
            uniq.append(k)
    while len(uniq) < n_rows:
        k = rng.choice(ks) if ks and rng.random() < 0.5 else rng.getrandbits(256 * nw)
        if k not in seen or len(seen) >= top:
            seen.add(k)
            uniq.append(k)
    uniq = uniq[:n_rows]  # the edges and the hits come first in the list
    rng.shuffle(uniq)
    return uniq


def key_soa(keys, nw):
    """[nw, 8, rows] u32: column w = key word w (low word first)."""
    soa = np.zeros((nw, 8, len(keys)), dtype=np.uint32)
    for r, k in enumerate(keys):
        for j in range(8 * nw):
            soa[j // 8, j % 8, r] = (k >> (32 * j)) & 0xFFFFFFFF
    return soa


def key_node(b, nw):
    cols = [b.var("k%d" % w, 256) for w in range(nw)]
    key = cols[0]
    for c in cols[1:]:
        key = b.op(Op.CONCAT, c, key)
    return key, cols


def lookup_tapeset(nw, width, live=0, table=0):
    """Tapes over columns k0..k{nw-1}: [0] the value form, [1] the hit form, [2] the value mixed
    with `live` products of k0 that are all read twice (they stay live across the lookup: the
    tape needs about `live` more registers)."""
    ts = TapeSet()
    b = ts.builder()
    key, cols = key_node(b, nw)
    val = b.lookup(table, key, width)
    ts.add(b.finish(val))
    ts.add(b.finish(b.lookup(table, key, width, hit=True)))
    v256 = val if width == 256 else b.op(Op.ZEXT, val, imm0=256 - width)
    if live:
        vs = [b.op(Op.BVMUL, cols[0], b.const(0x9E3779B97F4A7C15 + 2 * i, 256))
              for i in range(live)]
        s1 = vs[0]
        for v in vs[1:]:
            s1 = b.op(Op.BVADD, s1, v)
        s2 = v256
        for v in vs:
            s2 = b.op(Op.BVXOR, b.op(Op.BVMUL, s2, v), v)
        v256 = b.op(Op.BVXOR, s1, s2)
    ts.add(b.finish(v256))
    return ts


def mixed_tapeset(width=256):
    """[0] LOOKUP with the keccak default: ite(hit, value, (keccak(k0) >> 139) << 6);
    [1] LOOKUP mixed with a division: value / (k0 | 1) + value % 7."""
    ts = TapeSet()
    b = ts.builder()
    key, cols = key_node(b, 1)
    val = b.lookup(0, key, 256)
    hit = b.lookup(0, key, 256, hit=True)
    h = b.op(Op.BVSHL, b.op(Op.BVLSHR, b.op(Op.KECCAK, key), b.const(139, 256)), b.const(6, 256))
    ts.add(b.finish(b.op(Op.ITE, hit, val, h)))
    d = b.op(Op.BVUDIV, val, b.op(Op.BVOR, cols[0], b.const(1, 256)))
    ts.add(b.finish(b.op(Op.BVADD, d, b.op(Op.BVUREM, val, b.const(7, 256)))))
    return ts


def case_rng(*parts):
    return random.Random(hash(parts) & 0xFFFFFFFF)


def device_values(ctx, ts, tapes, tabs, soa, native):
    """Root values [tape][row] of `tapes` of `ts` over tables `tabs` and the rows of `soa`, on
    the device (mh_eval_values_tables), and the compiled tapes' info."""
    ct = ctx.compile(ts)
    a = ctx.assignments(ts.n_vars, soa.shape[2])
    tb = native.tables_create(ctx, tabs)
    try:
        a.upload(soa)
        out = native.eval_values_tables(ctx, ct, tb, tapes, a, 0, soa.shape[2])
        info = ct.info()
    finally:
        tb.close()
        a.close()
        ct.close()
    vals = [[sum(int(out[i, k, r]) << (32 * k) for k in range(8)) for r in range(soa.shape[2])]
            for i in range(len(tapes))]
    return vals, info


def check_shapes(ctx, native, nws=(1, 2, 3), sizes=SIZES, widths=WIDTHS, rows=65):
    """Every table shape, value and hit forms, against lookup_ref; returns the lookups checked."""
    from tests.fake_tables import lookup_ref

    n_checked = 0
    for nw in nws:
        for n in sizes:
            for width in widths:
                rng = case_rng(nw, n, width)
                table, els = make_table(rng, n, nw, width)
                keys = probes(rng, table, nw, rows)
                ts = lookup_tapeset(nw, width)
                got, _ = device_values(ctx, ts, [0, 1], [(table, els, 256 * nw)],
                                       key_soa(keys, nw), native)
                for tape, hit in ((0, False), (1, True)):
                    want = [lookup_ref(table, els, k, hit, width) for k in keys]
                    assert got[tape] == want, (nw, n, width, hit)
                    n_checked += len(keys)
    return n_checked
