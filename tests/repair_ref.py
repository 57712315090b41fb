"""CPU reference of the repair step (include/mythril_hip.h mh_repair_*, csrc/repair.hip), and its
stand-in for tests of Sieve's repair policy without a GPU (test infrastructure only).

``score`` / ``select`` / ``mutate`` restate the device's three steps bit for bit on the oracles:
the tape evaluator (oracle/smt_eval.py) for the per-row conjunct masks, the counter-based generator
(smt_eval.gen_limb) for the picks, and the guided generator (oracle/guided_gen.py) for a mutated
conjunct's columns -- its base values through ``generate_row`` itself, its set draws by the same
rule applied to the elite's row instead of a fresh one.  The GPU tests (tests/test_gpu_repair.py)
pin the device against them.

``install(monkeypatch)`` layers native.repair_open / repair_score / repair_select / repair_mutate
over tests/fake_device.install.
"""
import numpy as np

from mythril_amd import native
from oracle import smt_eval as E
from oracle.guided_gen import COPY_FLAG, SALT_SET, _limbs_to_int, generate_row

SALT_PICK = 0x3C6EF372FE94F82B
NONE = native.NO_CONJUNCT


def score(tapes, pool, rows):
    """fails[r][c] = row r fails conjunct tape c; `rows` = per row the column values."""
    return [[not bool(E.evaluate(t, pool, row)) for t in tapes] for row in rows]


def select(fails, row_first, k, seed):
    """The min(k, rows) rows with the smallest (fail_count, row) as (row, fail_count, pick):
    row = row_first + index; pick = the (h mod fail_count)-th failing conjunct, h =
    gen_limb(seed ^ SALT_PICK, 0, row, 0), or NONE for a row that fails nothing."""
    order = sorted(range(len(fails)), key=lambda r: (sum(fails[r]), r))[:k]
    out = []
    for r in order:
        failing = [c for c, f in enumerate(fails[r]) if f]
        row = row_first + r
        pick = NONE
        if failing:
            pick = failing[E.gen_limb(seed ^ SALT_PICK, 0, row, 0) % len(failing)]
        out.append((row, len(failing), pick))
    return out


def _base_values(seed, g, arrays):
    """Every column's base value for draw index g: the generator's row of the guide without its
    sets."""
    bare = dict(arrays, set_off=np.zeros(1, dtype=np.uint32))
    return generate_row(seed, g, bare)


def mutate(src_row, elites, arrays, set_conj, conj_cols, per, flags, seed, global_base):
    """The children of `elites` ([(row, fail_count, pick)]): dst row s * per + c as a list of
    column values.  src_row(row) gives the src buffer's row (every buffer column)."""
    width = [int(x) for x in arrays["width"]]
    set_off, prob = arrays["set_off"], arrays["set_prob"]
    alt_off, e_col, e_val = arrays["alt_off"], arrays["entry_col"], arrays["entry_val"]
    n_sets = len(set_off) - 1
    out = []
    for s, (row, _, t) in enumerate(elites):
        parent = [int(x) for x in src_row(row)]
        for c in range(per):
            child = list(parent)
            out.append(child)
            if c == 0 or t == NONE:
                continue
            g = global_base + s * per + c
            mine = [j for j in range(n_sets) if int(set_conj[j]) == t]
            if (flags & native.MUTATE_REDRAW) or not mine:
                base = _base_values(seed, g, arrays)
                for v in conj_cols[t]:
                    child[v] = base[v]
            for j in mine:
                d = E.gen_limb(seed ^ SALT_SET, j, g, 0)
                n_alt = int(set_off[j + 1]) - int(set_off[j])
                if (d & 0xFF) >= int(prob[j]) or not n_alt:
                    continue
                alt = int(set_off[j]) + (d >> 8) % n_alt
                for e in range(int(alt_off[alt]), int(alt_off[alt + 1])):
                    col = int(e_col[e])
                    if col & COPY_FLAG:
                        dcol = col & ~COPY_FLAG
                        sc, dlo, slo, nb = (int(x) for x in e_val[e][:4])
                        m = ((1 << nb) - 1) << dlo
                        bits = ((child[sc] >> slo) << dlo) & m
                        child[dcol] = ((child[dcol] & ~m) | bits) & ((1 << width[dcol]) - 1)
                    else:
                        child[col] = _limbs_to_int(e_val[e]) & ((1 << width[col]) - 1)
    return out


# ---- the stand-in ---------------------------------------------------------------------------------
class FakeRepair:
    def __init__(self, ctx, max_conjuncts, max_rows, max_elites):
        self.max_conjuncts, self.max_rows, self.max_elites = max_conjuncts, max_rows, max_elites
        self.fails = None
        self.row_first = 0
        self.elites = None

    def close(self):
        pass


def fake_repair_open(ctx, max_conjuncts, max_rows, max_elites):
    return FakeRepair(ctx, max_conjuncts, max_rows, max_elites)


def fake_repair_score(rep, tapes, assign, *, tape_first=0, tape_count=None, row_first=0,
                      row_count=None, counts=False):
    tc = tapes.n_tapes - tape_first if tape_count is None else tape_count
    rc = assign.capacity - row_first if row_count is None else row_count
    assert 1 <= tc <= rep.max_conjuncts and 1 <= rc <= rep.max_rows
    rep.fails = score(tapes.tapes[tape_first:tape_first + tc], tapes.pool,
                      [assign.rows[row_first + r] for r in range(rc)])
    rep.row_first, rep.elites = row_first, None
    return np.array([sum(f) for f in rep.fails], dtype=np.uint32) if counts else None


def fake_repair_select(rep, k, seed):
    assert rep.fails is not None and 1 <= k <= rep.max_elites
    rep.elites = select(rep.fails, rep.row_first, k, seed)
    return np.array(rep.elites, dtype=native.ELITE_DTYPE)


def fake_repair_mutate(rep, src, dst, guide, set_conj, col_off, cols, per, *, flags=0, seed=0,
                       global_base=0):
    assert rep.elites is not None and dst is not src
    assert len(rep.elites) * per <= dst.capacity
    arrays = guide.arrays() if hasattr(guide, "arrays") else guide
    conj_cols = [[int(x) for x in cols[int(col_off[t]):int(col_off[t + 1])]]
                 for t in range(len(col_off) - 1)]
    rows = mutate(lambda r: src.rows[r], rep.elites, arrays, set_conj, conj_cols, per, flags, seed,
                  global_base)
    for i, row in enumerate(rows):
        dst.rows[i] = row


def install(monkeypatch):
    from tests import fake_device

    fake_device.install(monkeypatch)
    monkeypatch.setattr(native, "repair_open", fake_repair_open)
    monkeypatch.setattr(native, "repair_score", fake_repair_score)
    monkeypatch.setattr(native, "repair_select", fake_repair_select)
    monkeypatch.setattr(native, "repair_mutate", fake_repair_mutate)
