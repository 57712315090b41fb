"""Decision by enumeration: the Python restatement of the enumerating generator
and the eligibility rule of the sieve's decision step.

``enumerate_rows`` states bit for bit what mh_assign_enumerate (csrc/enumerate.hip) writes; it
is the kernel's test reference and what the CPU stand-in of the tests runs.
"""
from __future__ import annotations

from typing import List, Sequence

from . import native

MASK256 = (1 << 256) - 1
OP_KECCAK = 60  # MH_OP_KECCAK
# MH_COL_* kinds a decided group may hold: var, cell, ufcell, read, ufread
_KEPT_KINDS = frozenset(native.COLUMN_KINDS.index(k)
                        for k in ("var", "cell", "ufcell", "read", "ufread"))


def digits(domains, g: int) -> List[int]:
    """The digit of each domain column at global row g: (g / stride_j) mod size_j with
    stride_0 = 1 and stride_{j+1} = stride_j * size_j."""
    out = []
    stride = 1
    for size in domains.size:
        out.append((g // stride) % size)
        stride *= size
    return out


def enumerate_rows(domains, base: int, count: int) -> List[List[int]]:
    """Rows base .. base + count - 1 of the cross product of ``domains`` (a native.Domains, or
    anything with its kind / size / lo / lists / rows): per row the value of each domain
    column in the domains' column order, list_j[d] or lo_j + d."""
    if base < 0 or count < 0 or base + count > domains.rows:
        raise ValueError("rows %d..%d outside the product's %d" % (base, base + count,
                                                                  domains.rows))
    rows = []
    for g in range(base, base + count):
        row = []
        for j, d in enumerate(digits(domains, g)):
            if domains.kind[j] == native.DOMAIN_LIST:
                row.append(domains.lists[j][d])
            else:
                row.append((domains.lo[j] + d) & MASK256)
        rows.append(row)
    return rows


def eligible(keccak_reads: bool, keccak_table: bool, col_kinds: Sequence[int],
             group_cols: Sequence[int], nodes) -> bool:
    """Whether UNSAT of one lowered group implies UNSAT of the caller's constraints (DESIGN §3
    "what a decided UNSAT may rest on"): every lowering step on the way to the group's tape must
    take a model of the constraints to a model of the tape.  The keccak lowering does not -- it
    fixes one interpretation H(x) of the hash, and the read mode adds injectivity -- so a query
    with a keccak table, a session in keccak-read mode, a group with a keccak read column and a
    tape with a keccak node are all ineligible.  Variables, array and function cells and
    Ackermann reads only drop freedom no model uses; the else columns, which no lowered query
    reads, have no argument made for them and are ineligible too."""
    if keccak_reads or keccak_table:
        return False
    if any(col_kinds[c] not in _KEPT_KINDS for c in group_cols):
        return False
    return not bool((nodes["op"] == OP_KECCAK).any())
