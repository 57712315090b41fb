"""Guides for the guided generator's parity tests (device-free: numpy and the oracle only).

mh_assign_generate_guided has three kernels on the device (mythril_amd/csrc/generate.hip,
launch_generate_guided): the staged LDS form, the LDS form and the plain one, chosen by the size
of the guide.  make_guide builds random guides in mh_guide order with knobs for what those kernels
treat differently (how many value-only sets lead, copy entries over the whole range stage_guide
accepts, empty sets and alternatives, probabilities 0 and 255); CASES names the guides the tests
use, one or more per form; directed_copy_guide walks the copy entry's limb arithmetic on purpose.
tests/test_guide_cases.py shows on the CPU that every case is what its name says;
tests/test_gpu_generator.py runs them on the device against oracle/guided_gen.py.
"""
from __future__ import annotations

import functools
from typing import Dict, Iterable, List, Tuple

import numpy as np

from oracle.guided_gen import COPY_FLAG, generate_row

WIDTHS = (1, 8, 31, 32, 33, 160, 255, 256)
EDGE_OFFSETS = (0, 1, 31, 32, 33, 224, 255)
EDGE_NBITS = (1, 31, 32, 33, 64, 255, 256)
_M64 = (1 << 64) - 1


def _offset(rng, width: int) -> int:
    """A copy entry's bit offset: anywhere stage_guide accepts, inside the column, limb-aligned,
    or next to a limb boundary."""
    mode = int(rng.integers(0, 4))
    if mode == 0:
        return int(rng.integers(0, 256))
    if mode == 1:
        return int(rng.integers(0, width))
    if mode == 2:
        return 32 * int(rng.integers(0, 8))
    return int(rng.choice(EDGE_OFFSETS))


def _nbits(rng) -> int:
    mode = int(rng.integers(0, 3))
    if mode == 0:
        return int(rng.integers(1, 257))
    if mode == 1:
        return int(rng.integers(1, 65))
    return int(rng.choice(EDGE_NBITS))


def _arrays(width, pool_off, pool, set_off, prob, alt_off, e_col, e_val) -> Dict:
    return dict(width=np.asarray(width, dtype=np.uint16),
                pool_off=np.asarray(pool_off, dtype=np.uint32),
                pool=np.asarray(pool, dtype=np.uint64).astype(np.uint32).reshape(-1, 8),
                set_off=np.array(set_off, dtype=np.uint32),
                set_prob=np.array(prob or [0], dtype=np.uint8),
                alt_off=np.array(alt_off, dtype=np.uint32),
                entry_col=np.array(e_col or [0], dtype=np.uint32),
                entry_val=np.array(e_val or [[0] * 8], dtype=np.uint64).astype(np.uint32))


def make_guide(rng, n_cols: int, n_sets: int, copy_p: float, copy_first: bool = False,
               empty_p: float = 1 / 16, max_alts: int = 3, max_entries: int = 5) -> Dict:
    """Random guide arrays in mh_guide order.  A set is a copy set (every entry a copy) with
    probability copy_p; copy_first makes set 0 a copy set with an entry in every alternative, so
    that no value-only set leads.  A set has no alternative, and an alternative no entry, with
    probability empty_p each (stage_guide allows both).  Copy entries use the whole accepted
    range (offsets 0..255, 1..256 bits) as well as offsets inside the columns."""
    width = rng.choice(WIDTHS, size=n_cols).astype(np.uint16)
    pool_n = rng.integers(0, 4, size=n_cols)
    pool_off = np.concatenate([[0], np.cumsum(pool_n)])
    pool = rng.integers(0, 1 << 32, size=(max(int(pool_off[-1]), 1), 8), dtype=np.uint64)
    set_off, alt_off, e_col, e_val, prob = [0], [0], [], [], []
    for j in range(n_sets):
        forced = copy_first and j == 0
        copy = forced or rng.random() < copy_p
        n_alt = 0 if (not forced and rng.random() < empty_p) else int(rng.integers(1, max_alts + 1))
        for _ in range(n_alt):
            n_ent = (0 if (not forced and rng.random() < empty_p)
                     else int(rng.integers(1, max_entries + 1)))
            for _ in range(n_ent):
                c = int(rng.integers(0, n_cols))
                if copy:
                    src = int(rng.integers(0, n_cols))
                    e_col.append(c | COPY_FLAG)
                    e_val.append([src, _offset(rng, int(width[c])), _offset(rng, int(width[src])),
                                  _nbits(rng), 0, 0, 0, 0])
                else:
                    e_col.append(c)
                    e_val.append([int(x) for x in rng.integers(0, 1 << 32, size=8)])
            alt_off.append(len(e_col))
        set_off.append(len(alt_off) - 1)
        u = rng.random()
        prob.append(0 if u < 0.1 else 255 if u < 0.35 else int(rng.integers(1, 255)))
    return _arrays(width, pool_off, pool, set_off, prob, alt_off, e_col, e_val)


def staged_bytes(arrays: Dict) -> int:
    """LDS bytes of the staged form: the last-entry slots (64 rows x 4 B per column) and the
    set_prob | set_off | alt_off | entry_col span stage_guide packs back to back."""
    n_cols = len(arrays["width"])
    n_sets = len(arrays["set_off"]) - 1
    n_alts = int(arrays["set_off"][n_sets])
    n_entries = int(arrays["alt_off"][n_alts])
    span_words = 2 * n_sets + n_alts + n_entries + 2
    return 256 * n_cols + 4 * span_words


def generator_form(arrays: Dict) -> str:
    """Which kernel launch_generate_guided (mythril_amd/csrc/generate.hip) takes for this guide:
    a restatement of its rule, to be edited together with it."""
    n_cols = len(arrays["width"])
    if n_cols and staged_bytes(arrays) <= 64 * 1024:
        return "staged"
    if n_cols and 256 * n_cols <= 48 * 1024:
        return "lds"
    return "plain"


def leading_value_sets(arrays: Dict) -> int:
    """The number of leading sets without a copy entry (the n_value_sets scan of stage_guide,
    mythril_amd/csrc/capi.cpp): the sets the LDS forms resolve in LDS."""
    set_off, alt_off, e_col = arrays["set_off"], arrays["alt_off"], arrays["entry_col"]
    n = 0
    for j in range(len(set_off) - 1):
        lo, hi = int(alt_off[int(set_off[j])]), int(alt_off[int(set_off[j + 1])])
        if any(int(e_col[e]) & COPY_FLAG for e in range(lo, hi)):
            break
        n += 1
    return n


def truncated(arrays: Dict, n_sets: int) -> Dict:
    """The guide with only its first n_sets sets (the oracle reads no alternative past them)."""
    return dict(arrays, set_off=arrays["set_off"][: n_sets + 1],
                set_prob=arrays["set_prob"][: max(n_sets, 1)])


def oracle_rows(seed: int, global_base: int, arrays: Dict, rows: Iterable[int]) -> np.ndarray:
    """oracle/guided_gen.py's rows as the device lays them out: u32 [n_cols, 8, len(rows)]."""
    rows = list(rows)
    out = np.zeros((len(arrays["width"]), 8, len(rows)), dtype=np.uint32)
    for i, r in enumerate(rows):
        vals = generate_row(seed, (global_base + r) & _M64, arrays)
        limbs = np.frombuffer(b"".join(val.to_bytes(32, "little") for val in vals), dtype="<u4")
        out[:, :, i] = limbs.reshape(-1, 8)
    return out


# Column widths of directed_copy_guide: four full-word destinations (0..3), the narrow ones (4..7),
# four full words nothing writes (8..11: a copy of 256 bits from an edge offset leaves a column
# nearly constant, so the entries draw their source bits from these), and three that only their
# own src == dst entry touches (12..14).
DIRECTED_WIDTHS = (256, 256, 256, 256, 8, 1, 33, 160, 256, 256, 256, 256, 256, 256, 256)


def directed_copy_entries() -> List[Tuple[int, int, int, int, int]]:
    """(dst, src, dst_lo, src_lo, nbits) of directed_copy_guide's sets, one entry per set."""
    ents = []
    # each edge offset as dst_lo against three of them as src_lo, the bit counts in rotation
    for i, dlo in enumerate(EDGE_OFFSETS):
        for step in (0, 2, 5):
            slo = EDGE_OFFSETS[(i + step) % len(EDGE_OFFSETS)]
            nb = EDGE_NBITS[(2 * i + step) % len(EDGE_NBITS)]
            ents.append((len(ents) % 4, 8 + (len(ents) + step) % 4, dlo, slo, nb))
    ents += [
        (0, 8, 32, 224, 32),     # both offsets limb-aligned, one limb
        (1, 9, 224, 0, 32),      # ... into the top limb
        (2, 10, 0, 32, 256),     # ... the word from limb 1 up (runs past the source's bit 256)
        (3, 11, 64, 33, 64),     # only the destination aligned
        (0, 9, 31, 96, 33),      # only the source aligned
        (1, 10, 0, 255, 256),    # src_lo + nbits > 256: one real bit, zeros above it
        (2, 11, 255, 0, 256),    # dst_lo + nbits > 256: one bit lands
        (3, 8, 224, 224, 64),    # both run past bit 256
        (12, 12, 33, 0, 64),     # src == dst, moved up
        (13, 13, 0, 31, 255),    # src == dst, moved down
        (14, 14, 32, 64, 32),    # src == dst, limb to limb
        (4, 8, 0, 33, 8),        # a destination of width 8, filled
        (4, 9, 1, 224, 31),      # ... the copy wider than the column
        (4, 10, 0, 32, 256),
        (5, 11, 0, 31, 1),       # a destination of width 1
        (5, 8, 0, 255, 33),
        (6, 9, 1, 1, 64),        # width 33: one bit into limb 1
        (7, 10, 33, 224, 255),   # width 160
        (0, 4, 224, 0, 32),      # a narrow source: 8 bits and 24 zeros
        (1, 11, 1, 224, 31),     # a chain: column 1 takes column 11's top limb,
        (2, 1, 33, 1, 31),       # column 2 takes those bits from column 1,
        (3, 2, 64, 33, 31),      # and column 3 takes them from column 2
    ]
    return ents


def directed_copy_guide() -> Dict:
    """A guide whose sets each apply one copy entry with probability 255 (directed_copy_entries):
    the edge offsets and bit counts of apply_entry / extract_bits (mythril_amd/csrc/guided_dev.h),
    limb-aligned and not, copies past bit 256, src == dst, narrow destinations and a chain."""
    ents = directed_copy_entries()
    n = len(ents)
    return _arrays(DIRECTED_WIDTHS, [0] * (len(DIRECTED_WIDTHS) + 1), [[0] * 8],
                   list(range(n + 1)), [255] * n, list(range(n + 1)),
                   [dst | COPY_FLAG for dst, _, _, _, _ in ents],
                   [[src, dlo, slo, nb, 0, 0, 0, 0] for _, src, dlo, slo, nb in ents])


# name -> (make_guide arguments, the form the case is meant to take).  The forms cases of the
# issue's table first (copy_p 0.2), then their all-value and copy-first variants, then the small
# guides of the row-window and launch-geometry tests (one per form: many alternatives per set make
# the span large while a row applies one of them, so the oracle stays cheap).
CASES: Dict[str, Tuple[Dict, str]] = {
    "lds_150x1100": (dict(n_cols=150, n_sets=1100, copy_p=0.2), "lds"),
    "lds_192x600": (dict(n_cols=192, n_sets=600, copy_p=0.2), "lds"),
    "plain_193x600": (dict(n_cols=193, n_sets=600, copy_p=0.2), "plain"),
    "plain_260x120": (dict(n_cols=260, n_sets=120, copy_p=0.2), "plain"),
    "staged_193x100": (dict(n_cols=193, n_sets=100, copy_p=0.2), "staged"),
    "staged_5x400": (dict(n_cols=5, n_sets=400, copy_p=0.2), "staged"),
    "staged_5x400_values": (dict(n_cols=5, n_sets=400, copy_p=0.0), "staged"),
    "lds_150x1100_values": (dict(n_cols=150, n_sets=1100, copy_p=0.0), "lds"),
    "lds_192x600_copyfirst": (dict(n_cols=192, n_sets=600, copy_p=0.2, copy_first=True), "lds"),
    "plain_193x600_copyfirst": (dict(n_cols=193, n_sets=600, copy_p=0.2, copy_first=True),
                                "plain"),
    "small_staged_7x60": (dict(n_cols=7, n_sets=60, copy_p=0.2), "staged"),
    "small_lds_96x420": (dict(n_cols=96, n_sets=420, copy_p=0.2, max_alts=16, max_entries=4),
                         "lds"),
    "small_plain_272x12": (dict(n_cols=272, n_sets=12, copy_p=0.3), "plain"),
    "copies_9x60": (dict(n_cols=9, n_sets=60, copy_p=1.0), "staged"),
}
FORM_CASES = ["lds_150x1100", "lds_192x600", "plain_193x600", "plain_260x120", "staged_193x100",
              "staged_5x400"]
ALL_VALUE_CASES = ["staged_5x400_values", "lds_150x1100_values"]
COPY_FIRST_CASES = ["lds_192x600_copyfirst", "plain_193x600_copyfirst"]
SMALL_CASES = ["small_staged_7x60", "small_lds_96x420", "small_plain_272x12"]
COLLISION_CASE = "staged_5x400_values"
# lds_192x600 sits on the column limit (256 * 192 = 49152) on purpose; no case is meant to sit on
# the 64 KB threshold of the staged form


@functools.lru_cache(maxsize=None)
def guide(name: str) -> Dict:
    """The named case's arrays (the same every time: the generator is seeded by the name's
    position in CASES)."""
    kw, _ = CASES[name]
    rng = np.random.default_rng(0x6D1DE + list(CASES).index(name))
    return make_guide(rng, **kw)
