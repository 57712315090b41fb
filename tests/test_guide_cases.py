"""The guides of tests/test_gpu_generator.py are what they claim to be (CPU, the reference alone):
each named case takes its intended generator kernel, the all-value and copy-first guides lead with
the sets they should, the collision guide overwrites every column several times per row, and
every entry of the directed copy guide is applied and changes its destination."""
import numpy as np
import pytest

from mythril_amd import native
from oracle import smt_eval
from oracle.guided_gen import COPY_FLAG, SALT_SET, generate_row
from tests import guide_cases as gc

KB = 1024
THRESHOLD = 64 * KB  # the staged form's LDS limit (generate.hip kGenLds)


@pytest.mark.parametrize("name", list(gc.CASES))
def test_case_takes_its_form(name):
    arrays = gc.guide(name)
    want = gc.CASES[name][1]
    n_cols, n_sets = len(arrays["width"]), len(arrays["set_off"]) - 1
    staged = gc.staged_bytes(arrays)
    print("%-26s %3d columns %4d sets  staged %6d B  leading value sets %4d  -> %s"
          % (name, n_cols, n_sets, staged, gc.leading_value_sets(arrays),
             gc.generator_form(arrays)))
    assert gc.generator_form(arrays) == want
    # no case sits by accident on the 64 KB threshold between the staged form and the others
    assert abs(staged - THRESHOLD) >= 4 * KB, staged
    if want == "lds":
        assert n_cols <= 192
    if want == "plain":
        assert n_cols > 192


def test_forms_are_each_covered_twice():
    forms = [gc.generator_form(gc.guide(n)) for n in gc.FORM_CASES + gc.ALL_VALUE_CASES
             + gc.COPY_FIRST_CASES]
    for f in ("staged", "lds", "plain"):
        assert forms.count(f) >= 2, (f, forms)
    assert sorted(gc.generator_form(gc.guide(n)) for n in gc.SMALL_CASES) == \
        ["lds", "plain", "staged"]
    # the column limit of the LDS form, on both sides
    assert len(gc.guide("lds_192x600")["width"]) * 256 == 48 * KB
    assert len(gc.guide("plain_193x600")["width"]) == 193
    # more than 192 columns and still an LDS form
    assert gc.generator_form(gc.guide("staged_193x100")) == "staged"


def test_generator_form_rule():
    """generator_form on hand-made sizes around both limits (the rule of launch_generate_guided)."""
    def sized(n_cols, n_entries):  # one set, one alternative, n_entries value entries
        return dict(width=np.full(n_cols, 32, dtype=np.uint16),
                    set_off=np.array([0, 1], dtype=np.uint32),
                    alt_off=np.array([0, n_entries], dtype=np.uint32))

    # span_words = 2 + 1 + n_entries + 2
    fit = (THRESHOLD - 256 * 100) // 4 - 5
    assert gc.staged_bytes(sized(100, fit)) == THRESHOLD
    assert gc.generator_form(sized(100, fit)) == "staged"
    assert gc.generator_form(sized(100, fit + 1)) == "lds"
    assert gc.generator_form(sized(192, 1 << 14)) == "lds"
    assert gc.generator_form(sized(193, 1 << 14)) == "plain"
    assert gc.generator_form(sized(193, 16)) == "staged"
    assert gc.generator_form(sized(256, 0)) == "plain"  # 256 B per column alone pass 64 KB
    assert gc.generator_form(sized(0, 0)) == "plain"


def test_make_guide_uses_its_whole_range():
    """One mid-sized guide holds everything make_guide promises: every width, pools of 0 to 3
    values, sets without alternatives, alternatives without entries, probabilities 0 and 255,
    copy offsets up to 255 and copies of 256 bits."""
    a = gc.make_guide(np.random.default_rng(5), 64, 600, 0.5)
    assert set(int(w) for w in a["width"]) == set(gc.WIDTHS)
    assert set(np.diff(a["pool_off"].astype(np.int64))) == {0, 1, 2, 3}
    assert 0 in np.diff(a["set_off"].astype(np.int64))
    assert 0 in np.diff(a["alt_off"].astype(np.int64))
    assert {0, 255} <= set(int(p) for p in a["set_prob"])
    copies = a["entry_val"][(a["entry_col"] & COPY_FLAG) != 0]
    assert len(copies) > 200
    for col in (1, 2):  # dst_lo, src_lo
        assert copies[:, col].min() == 0 and copies[:, col].max() == 255
        assert np.count_nonzero(copies[:, col] % 32 == 0) > 20
    assert copies[:, 3].min() == 1 and copies[:, 3].max() == 256
    assert np.all(copies[:, 0] < 64)


@pytest.mark.parametrize("name", gc.COPY_FIRST_CASES)
def test_copy_first_guides_lead_with_a_copy(name):
    assert gc.leading_value_sets(gc.guide(name)) == 0


@pytest.mark.parametrize("name", gc.ALL_VALUE_CASES)
def test_all_value_guides_hold_no_copy(name):
    a = gc.guide(name)
    assert gc.leading_value_sets(a) == len(a["set_off"]) - 1
    assert not np.any(a["entry_col"] & COPY_FLAG)


def test_mixed_guides_have_both_phases():
    """The copy_p 0.2 cases go on in memory from their first copy set, and most of them lead
    with a few value sets (a copy set comes first with probability 0.2)."""
    leading = {name: gc.leading_value_sets(gc.guide(name)) for name in gc.FORM_CASES}
    for name, n in leading.items():
        assert n < len(gc.guide(name)["set_off"]) - 2, name
    assert sum(n > 0 for n in leading.values()) >= 4, leading


def test_collision_guide_overwrites_every_column():
    """The 5-column, 400-set, all-value guide: in at least 90 % of 200 rows every column is
    written by two or more applied sets (the LDS forms' atomic max decides between them)."""
    a = gc.guide(gc.COLLISION_CASE)
    seed, base, rows = 0xC0111DE, (1 << 32) - 100, 200
    set_off, alt_off, e_col = a["set_off"], a["alt_off"], a["entry_col"]
    good = 0
    for r in range(rows):
        writers = [set() for _ in a["width"]]
        for j in range(len(set_off) - 1):
            s = smt_eval.gen_limb(seed ^ SALT_SET, j, base + r, 0)
            n_alt = int(set_off[j + 1]) - int(set_off[j])
            if (s & 0xFF) < int(a["set_prob"][j]) and n_alt:
                alt = int(set_off[j]) + (s >> 8) % n_alt
                for e in range(int(alt_off[alt]), int(alt_off[alt + 1])):
                    writers[int(e_col[e])].add(j)
        good += all(len(w) >= 2 for w in writers)
    print("collision guide: every column written by >= 2 applied sets in %d of %d rows"
          % (good, rows))
    assert good >= 0.9 * rows


def test_directed_copy_guide_covers_the_edges():
    ents = gc.directed_copy_entries()
    assert 24 <= len(ents) <= 64
    W = gc.DIRECTED_WIDTHS
    assert {d for _, _, d, _, _ in ents} >= set(gc.EDGE_OFFSETS)
    assert {s for _, _, _, s, _ in ents} >= set(gc.EDGE_OFFSETS)
    assert {n for _, _, _, _, n in ents} >= set(gc.EDGE_NBITS)
    assert any(d % 32 == 0 and s % 32 == 0 for _, _, d, s, _ in ents)
    assert any(d % 32 == 0 and s % 32 != 0 for _, _, d, s, _ in ents)
    assert any(d % 32 != 0 and s % 32 == 0 for _, _, d, s, _ in ents)
    assert any(d % 32 != 0 and s % 32 != 0 for _, _, d, s, _ in ents)
    assert any(s + n > 256 for _, _, _, s, n in ents)
    assert any(d + n > 256 for _, _, d, _, n in ents)
    assert any(dst == src for dst, src, _, _, _ in ents)
    assert any(W[dst] == 8 for dst, _, _, _, _ in ents)
    assert any(W[dst] == 1 for dst, _, _, _, _ in ents)
    assert any(d + n > W[dst] and W[dst] < 256 for dst, _, d, _, n in ents)
    # a chain: an entry reads the bits an earlier entry wrote
    assert any(ents[i][1] == ents[j][0] and ents[j][2] < ents[i][3] + ents[i][4]
               and ents[i][3] < ents[j][2] + ents[j][4]
               for i in range(len(ents)) for j in range(i))
    a = gc.directed_copy_guide()
    assert gc.generator_form(a) == "staged" and gc.leading_value_sets(a) == 0
    assert np.all(a["entry_col"] & COPY_FLAG) and np.all(a["set_prob"] == 255)


def test_directed_copy_entries_are_applied_and_change_their_column():
    """Every set of the directed guide applies in at least 95 % of rows (probability 255 of
    256), and for every entry some row's destination column differs before and after it."""
    a = gc.directed_copy_guide()
    ents = gc.directed_copy_entries()
    seed, base, rows = 0xD1EC7ED, (1 << 32) - 64, 128
    applied = np.zeros(len(ents), dtype=np.int64)
    changed = np.zeros(len(ents), dtype=np.int64)
    for r in range(rows):
        before = generate_row(seed, base + r, gc.truncated(a, 0))
        for j, (dst, _, _, _, _) in enumerate(ents):
            applied[j] += (smt_eval.gen_limb(seed ^ SALT_SET, j, base + r, 0) & 0xFF) < 255
            after = generate_row(seed, base + r, gc.truncated(a, j + 1))
            assert [v for c, v in enumerate(after) if c != dst] == \
                [v for c, v in enumerate(before) if c != dst]
            changed[j] += after[dst] != before[dst]
            before = after
    print("directed copy guide over %d rows: applied min %d, changed min %d (entry %d)"
          % (rows, applied.min(), changed.min(), int(changed.argmin())))
    assert applied.min() >= 0.95 * rows
    assert changed.min() >= 1, ents[int(changed.argmin())]


INDEX_BASES = [0, (1 << 32) - 1, (1 << 63) + 12345]
INDEX_SEEDS = [0, (1 << 64) - 1, 0x8000000000000001]


def test_gen_limb_agrees_at_large_indices_and_seeds():
    """oracle.smt_eval.gen_limb against the library's mh_gen_limb where an index crosses 2^32 or
    has its top bit set and a seed has its top bit set, with the generator's salts applied: the
    oracle reduces modulo 2^64 as the u64 arithmetic of the library does."""
    from oracle.guided_gen import SALT_MODE

    for base in INDEX_BASES + [(1 << 32) - 100, (1 << 64) - 3]:
        for seed in INDEX_SEEDS:
            for salt in (0, SALT_MODE, SALT_SET):
                for var, limb in ((0, 0), (6, 1), (1099, 0), (259, 7)):
                    for row in (0, 1, 63, 150):
                        idx = (base + row) & ((1 << 64) - 1)
                        want = smt_eval.gen_limb(seed ^ salt, var, idx, limb)
                        assert 0 <= want < 1 << 32
                        assert native.gen_limb(seed ^ salt, var, idx, limb) == want
    # an unreduced index gives the same limb: the oracle masks, it does not rely on its caller
    assert smt_eval.gen_limb(7, 3, (1 << 64) + 5, 2) == smt_eval.gen_limb(7, 3, 5, 2)


def test_oracle_rows_layout():
    a = gc.guide("small_staged_7x60")
    got = gc.oracle_rows(11, (1 << 32) - 2, a, range(4))
    assert got.shape == (7, 8, 4) and got.dtype == np.uint32
    for i in range(4):
        want = generate_row(11, (1 << 32) - 2 + i, a)
        assert [sum(int(got[v, k, i]) << (32 * k) for k in range(8)) for v in range(7)] == want
