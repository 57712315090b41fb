"""CPU stand-ins for the table-set calls of mythril_amd.native (mh_tables_create,
mh_eval_values_tables), beside tests/fake_device.py, plus the Python restatement of the device's
table lookup that the emulator and the GPU tests are checked against (test infrastructure only).

``install(monkeypatch)`` installs fake_device's stand-ins and these.  Tapes are evaluated with
``oracle.smt_eval.evaluate(..., extra=...)``; ``Op.LOOKUP`` is handled in ``extra``.
"""
import numpy as np

from mythril_amd import native
from oracle import smt_eval as E
from oracle.keccak import keccak256
from tests import fake_device

LOOKUP = 85  # mythril_amd.tape.Op.LOOKUP, restated
M256 = (1 << 256) - 1


def lookup_ref(table, else_value, key, hit=False, width=256):
    """What MH_OP_LOOKUP computes: `table` ({key: value}) at `key`, else `else_value`, masked to
    `width` bits; with `hit`, whether the key is in the table."""
    if hit:
        return int(key in table)
    return table.get(key, else_value) & ((1 << width) - 1)


def lookup_extra(tables):
    """``extra`` for oracle.smt_eval.evaluate over `tables` [(table, else, key bits)]."""
    def extra(op, nd, vals):
        if op != LOOKUP:
            raise ValueError("unknown op %d" % op)
        tab, els, _ = tables[int(nd["imm0"])]
        return lookup_ref(tab, els, vals[int(nd["a"])], hit=bool(int(nd["imm1"])),
                          width=int(nd["width"]) or 1)
    return extra


class FakeTables:
    def __init__(self, ctx, tables):
        packed = native.pack_tables(tables)  # the real packing runs (sorting, limb cutting)
        # ... and what mh_tables_create refuses about a set's shape (compile.cpp pack_tables)
        if len(tables) > 1 << 14 or any(not 1 <= int(nw) <= 3 for nw in packed[1][:len(tables)]):
            raise native.SieveError(native.MH_E_INVALID, "mh_tables_create: key words outside "
                                    "1..3 or more tables than a lookup can name")
        self.tables = [(dict(t), int(e), int(kb)) for t, e, kb in tables]

    def close(self):
        pass


def fake_tables_create(ctx, tables):
    return FakeTables(ctx, tables)


def fake_eval_values_tables(ctx, tapes, tables, ids, assign, row_first=0, row_count=1):
    out = np.zeros((max(len(ids), 1), 8, max(row_count, 1)), dtype=np.uint32)
    extra = lookup_extra(tables.tables)
    for i, t in enumerate(ids):
        for r in range(row_count):
            v = int(E.evaluate(tapes.tapes[t], tapes.pool, assign.rows[row_first + r],
                               extra=extra))
            for k in range(8):
                out[i, k, r] = (v >> (32 * k)) & 0xFFFFFFFF
    return out[:len(ids), :, :row_count]


def install(monkeypatch):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(native, "tables_create", fake_tables_create)
    monkeypatch.setattr(native, "eval_values_tables", fake_eval_values_tables)


def oracle_functions(ext, b):
    """{name: callable} for oracle.term_eval.evaluate_term with the meaning of `ext`
    (certify.ExtModel): the table, then the constant default or the keccak rule
    ``H(x) = base + ((keccak256(x) >> 139) << 6)``."""
    from mythril_amd.certify import KeccakRule

    out = {}
    for name, (tab, dflt) in ext.functions.items():
        if isinstance(dflt, KeccakRule):
            nbytes = b.symbols.functions[name][1] // 8

            def f(x, tab=tab, base=dflt.base, nbytes=nbytes):
                if x in tab:
                    return tab[x]
                h = int.from_bytes(keccak256(x.to_bytes(nbytes, "big")), "big")
                return (base + ((h >> 139) << 6)) & M256
        else:
            def f(x, tab=tab, dflt=dflt):
                return tab.get(x, dflt)
        out[name] = f
    return out


def oracle_value(ext, ctx, node):
    """oracle.term_eval.evaluate_term of the ORIGINAL term `node` under `ext`."""
    from oracle.term_eval import evaluate_term

    b = ctx.b
    names = [n for n, _ in sorted(b.var_index.items(), key=lambda kv: kv[1])]
    tape = b.finish(node)
    return evaluate_term(tape.nodes, b.pool.values, names, b.symbols.array_names,
                         b.symbols.function_names, ext.scalars, ext.arrays,
                         oracle_functions(ext, b))
