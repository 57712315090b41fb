"""Jobs for the batched round's parity check (mh_query_round_many against mh_query_round, job by
job): the tape sets, guides and job list tests/test_gpu_round_many.py runs in the default library
and tests/noasm_round_many_check.py in the C++ step() library.

One batch of 17 jobs covers: counts 1 / 63 / 64 / 65 / 4096; column counts 1, 5 (columns past the
four preloaded ones are loaded by LOADVAR) and 40; a one-tape set and a 70-tape set (two LDS
chunks); tapes above 64 instructions (a window change) and above 2048 (streamed from global
memory); register classes NR 7 / 9 / 15; feature classes asm-only / complex / keccak / EVM; a
tape_first > 0 sub-range; both modes; a job with no hit and one whose only hit is in the last
partial wave; a global_base above 2^32; guides of all three generator forms
(tests/guide_cases.py).  coverage() states what the compiled sets really are, so a case that
stopped being what its name says fails the test instead of weakening it.
"""
from __future__ import annotations

import random
from typing import Dict, List

import numpy as np

from mythril_amd import native
from mythril_amd.tape import Op, TapeSet
from tests import guide_cases
from tests.fuzz import TapeFuzzer, tree_tape

SEED = 0xBA7C4ED
M64 = (1 << 64) - 1
# dev_isa.h feature bits
F_KECCAK, F_EVM, F_CPLX = 2, 4, 8


class HostGuide:
    """What query_round needs of a guide (GuideHandle.guide) over arrays built on the host."""

    def __init__(self, arrays: Dict):
        self.arrays_ = arrays
        self.guide, self._keep = native._guide_struct(arrays)

    def arrays(self) -> Dict:
        return self.arrays_


def flat_guide(n_cols: int) -> Dict:
    """Every column 256 bits wide, no pool value and no set: each row's columns are the
    generator's base values."""
    return guide_cases._arrays([256] * n_cols, [0] * (n_cols + 1), [[0] * 8], [0], [], [0], [],
                               [])


def one_tape_set() -> TapeSet:
    """One asm-only tape over one column."""
    ts = TapeSet()
    b = ts.builder()
    ts.add(b.finish(b.op(Op.BVULT, b.var("x0"), b.const(1 << 255, 256))))
    return ts


def tree_set() -> TapeSet:
    """70 asm-only tapes over three columns in all three register classes (tests/fuzz.py
    tree_tape: depth + 3 registers), in mixed order."""
    ts = TapeSet()
    b = ts.builder()
    for v in range(3):
        b.var("v%d" % v, 256)
    depths = [2, 3, 5, 2, 8, 3, 6, 2, 3, 9]
    for i in range(70):
        tree_tape(ts, b, depths[i % len(depths)], salt=i)
    return ts


def conjunction_set(last_only: int) -> TapeSet:
    """Long conjunctions over five columns with overflow predicates (complex ops): 12, 150 and
    300 conjuncts -- above 64 instructions, and above 2048 -- each ending in a never / half /
    always conjunct; and a tape only the value `last_only` of x0 satisfies."""
    from tests.test_gpu_interp_core import _conjunction

    rng = random.Random(9100)
    ts = TapeSet()
    b = ts.builder()
    xs = [b.var("x%d" % i) for i in range(5)]
    never = b.op(Op.EQ, xs[0], b.const(rng.getrandbits(256), 256))
    half = b.op(Op.BVULT, xs[1], b.const(1 << 255, 256))
    always = b.op(Op.NOT, b.op(Op.BVULT, xs[2], b.const(0, 256)))
    for n in (12, 150, 300):
        for newest in (never, half, always):
            ts.add(b.finish(_conjunction(b, rng, xs, n, newest)))
    ts.add(b.finish(b.op(Op.AND, b.op(Op.EQ, xs[0], b.const(last_only, 256)),
                         b.op(Op.BVADD_NOOVFL_U, b.op(Op.BVAND, xs[4], b.const(M64, 256)),
                              b.op(Op.BVAND, xs[3], b.const(M64, 256))))))
    return ts


def fuzz_set(seed: int, keccak: bool, evm: bool, n: int = 10) -> TapeSet:
    """Random Bool tapes over 40 columns with keccak applications and / or the EVM helpers."""
    ts = TapeSet()
    fz = TapeFuzzer(random.Random(seed), ts, n_vars=40, allow_keccak=keccak, allow_evm=evm,
                    max_depth=4)
    b = fz.b
    for i in range(n):
        # a conjunct of the feature itself, so the set has the class whatever the fuzzer drew
        x, y = b.var("v%d" % (3 * i % 40), 256), b.var("v%d" % ((3 * i + 7) % 40), 256)
        if evm:
            f = b.op(Op.EVM_BYTE, b.const(31, 256), b.op(Op.BVXOR, x, y))
        else:
            f = b.op(Op.KECCAK, b.op(Op.BVXOR, x, y))
        ts.add(b.finish(b.op(Op.AND, fz.boolean(3),
                             b.op(Op.BVULT, f, b.const((1 << 256) - (1 << 250), 256)))))
    return ts


LAST_ONLY_COUNT = 65      # row 64 alone is the last, partial wave
LAST_ONLY_BASE = 977


def last_only_value() -> int:
    """Column 0 of row 64 of the flat five-column guide's rows at LAST_ONLY_BASE."""
    rows = guide_cases.oracle_rows(SEED + 11, LAST_ONLY_BASE, flat_guide(5), [LAST_ONLY_COUNT - 1])
    return int.from_bytes(rows[0, :, 0].astype("<u4").tobytes(), "little")


def build(ctx) -> List[Dict]:
    """The 17 jobs, each with a buffer of its own (query_round_many's job dicts plus "name")."""
    sets = {
        "one": one_tape_set(),
        "tree": tree_set(),
        "conj": conjunction_set(last_only_value()),
        "kec": fuzz_set(41, keccak=True, evm=False),
        "evm": fuzz_set(42, keccak=True, evm=True),
    }
    cts = {k: ctx.compile(v) for k, v in sets.items()}
    guides = {
        "flat1": HostGuide(flat_guide(1)),
        "flat5": HostGuide(flat_guide(5)),
        "staged7": HostGuide(guide_cases.guide("small_staged_7x60")),
        "lds96": HostGuide(guide_cases.guide("small_lds_96x420")),
        "plain272": HostGuide(guide_cases.guide("small_plain_272x12")),
        "staged5": HostGuide(guide_cases.guide("staged_5x400")),
    }
    C, F = native.MODE_COUNT_ALL, native.MODE_FIRST_HIT
    #        name              set     guide       count mode base             tape range
    spec = [("one_1",          "one",  "flat1",    1,    C, 0,               None),
            ("one_4096",       "one",  "flat1",    4096, F, 5,               None),
            ("tree_63",        "tree", "staged7",  63,   C, 1 << 24,         None),
            ("tree_64",        "tree", "lds96",    64,   F, 2 << 24,         None),
            ("tree_65_sub",    "tree", "plain272", 65,   C, 3 << 24,         (3, 60)),
            ("tree_4096",      "tree", "staged7",  4096, F, 4 << 24,         None),
            ("tree_4096_cnt",  "tree", "staged7",  4096, C, (1 << 40) + 12345, None),
            ("conj_4096",      "conj", "staged5",  4096, C, 6 << 24,         None),
            ("conj_65_first",  "conj", "staged5",  65,   F, 7 << 24,         None),
            ("conj_last_only", "conj", "flat5",    LAST_ONLY_COUNT, F, LAST_ONLY_BASE, (9, 1)),
            ("conj_no_hit",    "conj", "flat5",    4096, F, 8 << 24,         (0, 1)),
            ("conj_sub_big",   "conj", "lds96",    63,   C, (9 << 24) + 1,   (2, 7)),
            ("kec_64",         "kec",  "lds96",    64,   C, 10 << 24,        None),
            ("kec_4096",       "kec",  "plain272", 4096, F, 11 << 24,        None),
            ("evm_65",         "evm",  "lds96",    65,   C, 12 << 24,        None),
            ("evm_1",          "evm",  "plain272", 1,    F, (1 << 33) + 7,   None),
            ("evm_4096_sub",   "evm",  "lds96",    4096, C, 13 << 24,        (4, 5))]
    jobs = []
    for i, (name, s, g, count, mode, base, rng) in enumerate(spec):
        ts, guide = sets[s], guides[g]
        n_guide = len(guide.arrays()["width"])
        assign = ctx.assignments(max(ts.n_vars, n_guide), count)
        job = dict(name=name, tapes=cts[s], assign=assign, guide=guide, seed=SEED + i,
                   global_base=base, count=count, n_cols=ts.n_vars, mode=mode)
        if name in ("conj_last_only",):
            job["seed"] = SEED + 11
        if rng is not None:
            job["tape_first"], job["tape_count"] = rng
        jobs.append(job)
    return jobs


def coverage(jobs: List[Dict]) -> None:
    """The batch is what the module's docstring says (read off the compiled sets)."""
    by = {j["name"]: j for j in jobs}
    infos = {j["name"]: j["tapes"].info() for j in jobs}
    classes, feats = set(), set()
    for j in jobs:
        tf = j.get("tape_first", 0)
        tc = j.get("tape_count", j["tapes"].n_tapes - tf)
        for t in infos[j["name"]][tf:tf + tc]:
            n, f = int(t["n_regs"]), int(t["features"])
            classes.add(0 if n <= 7 else 1 if n <= 9 else 2)
            feats.add(3 if f & F_EVM else 2 if f & F_KECCAK else 1 if f & F_CPLX else 0)
    assert classes == {0, 1, 2}, classes
    assert feats == {0, 1, 2, 3}, feats
    assert {j["count"] for j in jobs} == {1, 63, 64, 65, 4096}
    assert {j["n_cols"] for j in jobs} == {1, 3, 5, 40}
    assert by["one_1"]["tapes"].n_tapes == 1 and by["tree_63"]["tapes"].n_tapes == 70
    insns = [int(t["n_insns"]) for t in infos["conj_4096"]][:9]  # the long conjunctions
    assert min(insns) > 64 and max(insns) > 2048, insns
    assert any(j["global_base"] >> 32 for j in jobs)
    assert {guide_cases.generator_form(j["guide"].arrays()) for j in jobs} == \
        {"staged", "lds", "plain"}
    assert {j["mode"] for j in jobs} == {native.MODE_COUNT_ALL, native.MODE_FIRST_HIT}


def run_sequential(ctx, jobs: List[Dict]):
    """Per job: query_round's results and a download of the buffer's rows [0, count)."""
    out = []
    for j in jobs:
        kw = {k: j[k] for k in ("tape_first", "tape_count", "mode") if k in j}
        fh, hc, rows = native.query_round(ctx, j["tapes"], j["assign"], j["guide"], j["seed"],
                                          j["global_base"], j["count"], j["n_cols"], **kw)
        out.append((fh.copy(), hc.copy(), rows.copy(), j["assign"].download(0, j["count"])))
    return out


def run_batched(ctx, jobs: List[Dict]):
    """The same from one query_round_many, over buffers overwritten first."""
    for j in jobs:
        j["assign"].generate(0xDEAD, 99)
    res = native.query_round_many(ctx, jobs)
    return [(fh.copy(), hc.copy(), rows.copy(), j["assign"].download(0, j["count"]))
            for (fh, hc, rows), j in zip(res, jobs)]


def hit_count_is_defined(job: Dict) -> bool:
    """MH_MODE_FIRST_HIT skips a wave once a smaller witness is known, so with more than one
    workgroup per tape (more than 64 rows) its hit_count depends on the order the workgroups
    ran in -- in mh_query_round as in the batch.  Everywhere else it is compared bitwise."""
    return job.get("mode", native.MODE_FIRST_HIT) == native.MODE_COUNT_ALL or job["count"] <= 64


def assert_equal(jobs: List[Dict], want, got) -> int:
    """Bitwise equality per job; returns the number of jobs with a hit."""
    hits = 0
    for j, w, g in zip(jobs, want, got):
        assert np.array_equal(w[0], g[0]), (j["name"], "first_hit", w[0], g[0])
        if hit_count_is_defined(j):
            assert np.array_equal(w[1], g[1]), (j["name"], "hit_count", w[1], g[1])
        assert np.array_equal(w[2], g[2]), (j["name"], "rows_out")
        assert np.array_equal(w[3], g[3]), (j["name"], "buffer contents")
        hits += bool(np.any(w[0] != native.NO_HIT))
    return hits


def check(ctx) -> str:
    """The whole parity check on `ctx`; returns a one-line summary."""
    jobs = build(ctx)
    try:
        coverage(jobs)
        want = run_sequential(ctx, jobs)
        by = {j["name"]: w for j, w in zip(jobs, want)}
        # the cases that are about where the hit is
        assert np.all(by["conj_no_hit"][0] == native.NO_HIT)
        assert by["conj_last_only"][0].tolist() == [LAST_ONLY_BASE + LAST_ONLY_COUNT - 1]
        got = run_batched(ctx, jobs)
        hits = assert_equal(jobs, want, got)
        assert hits >= 12, hits
        for n in (1, 2):  # the smallest batches: the last n jobs of the list... and the first
            for part in (jobs[:n], jobs[5:5 + n]):
                assert_equal(part, [want[jobs.index(j)] for j in part], run_batched(ctx, part))
        return "round_many ok: %d jobs equal mh_query_round, %d with a hit" % (len(jobs), hits)
    finally:
        for j in jobs:
            j["assign"].close()
        for ct in {id(j["tapes"]): j["tapes"] for j in jobs}.values():
            ct.close()
