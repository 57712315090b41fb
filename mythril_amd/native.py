"""ctypes binding of libmythril_hip (include/mythril_hip.h).

The reference reaches its native solver (z3) in-process through ctypes as well
(z3-solver's ``z3core``); this module is the analogous binding for the sieve.  The
library is loaded from the package directory (built in-tree by ``__graft_entry__.build()``
or ``make -C mythril_amd/csrc``); a missing library raises ``NativeUnavailable`` — there is
no CPU fallback on the product path.

One HIP runtime per process: torch ships its own ``libamdhip64`` (same SONAME as ROCm's).  A
process that also uses torch on the GPU (bench.py, the GPU tests) imports torch and initialises
CUDA before this library loads, so both bind to torch's copy; the library's RCCL (mh_comm_*) is
ROCm's, opened with RTLD_DEEPBIND and bound to that same runtime.
"""
from __future__ import annotations

import ctypes as C
import os
from itertools import chain
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .tape import NODE_DTYPE, TapeSet

LIB_NAME = "libmythril_hip.so"
LIB_PATH = os.environ.get("MYTHRIL_HIP_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

MH_OK = 0
MH_E_INVALID = -1
MH_E_UNSUPPORTED = -2
MH_E_DEVICE = -3
MH_E_NOMEM = -4
MH_E_NODEVICE = -5

MODE_FIRST_HIT = 0
MODE_COUNT_ALL = 1
NO_HIT = 0xFFFFFFFFFFFFFFFF

# every symbol include/mythril_hip.h declares: name -> (restype, argtypes)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_vp = C.c_void_p
SIGNATURES = {
    "mh_version": (C.c_int32, [_u32p, _u32p, _u32p]),
    "mh_last_error": (C.c_char_p, []),
    "mh_device_count": (C.c_int32, [C.POINTER(C.c_int32)]),
    "mh_ctx_create": (C.c_int32, [C.c_int32, C.POINTER(_vp)]),
    "mh_ctx_destroy": (C.c_int32, [_vp]),
    "mh_ctx_set_stream": (C.c_int32, [_vp, _vp]),
    "mh_ctx_synchronize": (C.c_int32, [_vp]),
    "mh_ctx_clear_cache": (C.c_int32, [_vp]),
    "mh_tapes_compile": (C.c_int32, [_vp, _vp, _u64p, C.c_uint32, _u32p, C.c_uint32, C.c_uint32,
                                     C.POINTER(_vp)]),
    "mh_tapes_compile_async": (C.c_int32, [_vp, _vp, _u64p, C.c_uint32, _u32p, C.c_uint32,
                                           C.c_uint32]),
    "mh_tapes_compile_wait": (C.c_int32, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_double)]),
    "mh_tapes_destroy": (C.c_int32, [_vp]),
    "mh_tapes_info": (C.c_int32, [_vp, _vp, C.c_uint32]),
    "mh_tapes_spills": (C.c_int32, [_vp, _vp, C.c_uint32]),
    "mh_tapes_split_info": (C.c_int32, [_vp, _u32p, _u32p, _vp, C.c_uint32]),
    "mh_assign_create": (C.c_int32, [_vp, C.c_uint32, C.c_uint64, C.POINTER(_vp)]),
    "mh_assign_destroy": (C.c_int32, [_vp]),
    "mh_assign_upload": (C.c_int32, [_vp, _u32p, C.c_uint64, C.c_uint64]),
    "mh_assign_download": (C.c_int32, [_vp, _u32p, C.c_uint64, C.c_uint64]),
    "mh_assign_generate": (C.c_int32, [_vp, C.c_uint64, C.c_uint64]),
    "mh_gen_limb": (C.c_uint32, [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32]),
    "mh_assign_generate_guided": (C.c_int32, [_vp, C.c_uint64, C.c_uint64, C.c_uint64,
                                              C.c_uint64, _vp]),
    "mh_results_reset": (C.c_int32, [_vp, _vp, _vp, C.c_uint32]),
    "mh_run": (C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, _vp, C.c_uint64, C.c_uint64,
                           C.c_uint64, C.c_uint32, _u64p, _u64p]),
    "mh_run_rows": (C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, _vp, C.c_uint64, C.c_uint64,
                                C.c_uint64, C.c_uint32, _u64p, _u64p, C.c_uint32, _u32p]),
    "mh_query_round": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64,
                                   C.c_uint32, C.c_uint32, C.c_uint32, _u64p, _u64p, C.c_uint32,
                                   _u32p]),
    "mh_query_round_many": (C.c_int32, [_vp, _vp, C.c_uint32]),
    "mh_run_async": (C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, _vp, C.c_uint64, C.c_uint64,
                                 C.c_uint64, C.c_uint32, _vp, _vp]),
    "mh_eval_values": (C.c_int32, [_vp, _vp, C.c_uint32, _vp, C.c_uint64, C.c_uint64, _u32p]),
    "mh_microbench_valu": (C.c_int32, [_vp, C.c_uint32, C.POINTER(C.c_double)]),
    "mh_microbench_issue": (C.c_int32, [_vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]),
    "mh_microbench_gather": (C.c_int32, [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), _u64p]),
    "mh_eval_values_many": (C.c_int32, [_vp, _vp, _u32p, C.c_uint32, _vp, C.c_uint64, _u32p]),
    "mh_ctx_eval_launches": (C.c_int32, [_vp, _u64p]),
    "mh_tables_create": (C.c_int32, [_vp, C.c_uint32, _u32p, _u32p, _u64p, _u32p, C.c_uint64,
                                     _u64p, _u32p, C.c_uint64, _u32p, C.POINTER(_vp)]),
    "mh_tables_destroy": (C.c_int32, [_vp]),
    "mh_eval_values_tables": (C.c_int32, [_vp, _vp, _vp, _u32p, C.c_uint32, _vp, C.c_uint64,
                                          C.c_uint64, _u32p]),
    "mh_tables_create_many": (C.c_int32, [_vp, C.c_uint32, _u32p, _u32p, _u32p, _u64p, _u32p,
                                          C.c_uint64, _u64p, _u32p, C.c_uint64, _u32p,
                                          C.POINTER(_vp)]),
    "mh_eval_values_jobs": (C.c_int32, [_vp, _vp, C.c_uint32]),
    "mh_tapes_jit": (C.c_int32, [_vp, C.c_uint32, C.c_uint32]),
    "mh_tapes_jit_info": (C.c_int32, [_vp, _vp]),
    "mh_tapes_jit_code_id": (C.c_int32, [_vp, _u64p]),
    "mh_jit_code_id": (C.c_int32, [_vp, _u64p, C.c_uint32, _u32p, C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_uint32, _u64p]),
    "mh_tapes_jitted": (C.c_int32, [_vp, C.POINTER(C.c_uint8), C.c_uint32]),
    "mh_jit_eval_all": (C.c_int32, [_vp, _vp, _vp, C.c_uint64, C.c_uint64, _u32p]),
    "mh_comm_unique_id": (C.c_int32, [_vp]),
    "mh_comm_init": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32]),
    "mh_comm_allreduce_results": (C.c_int32, [_vp, _vp, _vp, C.c_uint32]),
    "mh_comm_destroy": (C.c_int32, [_vp]),
    "mh_ctx_enable_timing": (C.c_int32, [_vp, C.c_int32]),
    "mh_ctx_kernel_time": (C.c_int32, [_vp, C.POINTER(C.c_double), _u64p]),
    "mh_guide_harvest": (C.c_int32, [_vp, C.c_uint32, _u32p, C.c_uint32, C.POINTER(C.c_uint16),
                                     C.c_uint32, _u32p, _u32p, C.c_uint32, C.POINTER(_vp), _vp]),
    "mh_guide_harvest_inc": (C.c_int32, [_vp, C.c_uint32, _u32p, C.c_uint32,
                                         C.POINTER(C.c_uint16), C.c_uint32, _u32p, _u32p,
                                         C.c_uint32, C.POINTER(_vp), _vp]),
    "mh_harvest_free": (C.c_int32, [_vp]),
    "mh_harvester_create": (C.c_int32, [C.POINTER(_vp)]),
    "mh_harvester_destroy": (C.c_int32, [_vp]),
    "mh_harvester_stats": (C.c_int32, [_vp, _u64p]),
    "mh_guide_harvest_with": (C.c_int32, [_vp, _vp, C.c_uint32, _u32p, C.c_uint32,
                                          C.POINTER(C.c_uint16), C.c_uint32, _u32p, _u32p,
                                          C.c_uint32, C.POINTER(_vp), _vp]),
    "mh_smtlib_create": (C.c_int32, [C.POINTER(_vp)]),
    "mh_smtlib_destroy": (C.c_int32, [_vp]),
    "mh_smtlib_read": (C.c_int32, [_vp, C.c_char_p, C.c_uint64, _vp]),
    "mh_smtlib_commit": (C.c_int32, [_vp, C.POINTER(C.c_int64), C.c_uint64]),
    "mh_smtlib_rollback": (C.c_int32, [_vp]),
    "mh_smtlib_size": (C.c_uint64, [_vp]),
    "mh_terms_create": (C.c_int32, [C.POINTER(_vp)]),
    "mh_terms_destroy": (C.c_int32, [_vp]),
    "mh_terms_set_options": (C.c_int32, [_vp, C.c_uint32]),
    "mh_terms_append": (C.c_int32, [_vp, _vp, C.c_uint64, _u32p, C.c_uint64, C.c_char_p,
                                    C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]),
    "mh_terms_sizes": (C.c_int32, [_vp, _u64p]),
    "mh_query_build": (C.c_int32, [_vp, _u32p, C.c_uint32, C.POINTER(_vp), _vp]),
    "mh_query_free": (C.c_int32, [_vp]),
    "mh_conjuncts_build": (C.c_int32, [_vp, C.c_uint32, _u32p, C.c_uint32, C.c_uint32,
                                       C.POINTER(_vp), _vp]),
    "mh_conjuncts_free": (C.c_int32, [_vp]),
    "mh_harvest_set_conjuncts": (C.c_int32, [_vp, _u32p, C.c_uint32]),
    "mh_repair_create": (C.c_int32, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    "mh_repair_destroy": (C.c_int32, [_vp]),
    "mh_repair_score": (C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, _vp, C.c_uint64,
                                    C.c_uint64, _u32p]),
    "mh_repair_select": (C.c_int32, [_vp, C.c_uint32, C.c_uint64, _vp, _u32p]),
    "mh_repair_mutate": (C.c_int32, [_vp, _vp, _vp, _vp, _u32p, _u32p, _u32p, C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]),
    "mh_domains_build": (C.c_int32, [_vp, C.c_uint32, _u32p, C.c_uint32, C.POINTER(C.c_uint16),
                                     C.c_uint32, _u32p, C.c_uint32, C.POINTER(_vp)]),
    "mh_domains_create": (C.c_int32, [_u32p, _u32p, _u64p, _u32p, _u32p, _u32p, C.c_uint32,
                                      C.POINTER(C.c_uint16), C.c_uint32, C.POINTER(_vp)]),
    "mh_domains_info": (C.c_int32, [_vp, _vp]),
    "mh_domains_free": (C.c_int32, [_vp]),
    "mh_assign_enumerate": (C.c_int32, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64]),
    "mh_query_enumerate": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_uint64, C.c_uint64, C.c_uint32,
                                       C.c_uint32, _u64p, _u64p, C.c_uint32, _u32p]),
    "mh_run_hits": (C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, _vp, C.c_uint64, C.c_uint64,
                                C.c_uint64, C.c_uint32, _u64p, _u32p, _u64p, C.c_uint32, _u32p]),
    "mh_assign_scatter": (C.c_int32, [_vp, C.c_uint64, C.c_uint32, _u32p, C.c_uint32, _u32p]),
    "mh_query_round_hits": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64,
                                        C.c_uint32, C.c_uint32, _vp, C.c_uint32, _u64p, _u32p,
                                        _u64p, C.c_uint32, _u32p]),
    "mh_query_round_hits_many": (C.c_int32, [_vp, _vp, C.c_uint32]),
}
HITS_MAX = 64          # MH_HITS_MAX
HITS_MAX_ROWS = 65536  # MH_HITS_MAX_ROWS

# mh_smt_record / mh_smt_result (include/mythril_hip.h)
SMT_RECORD_DTYPE = np.dtype([("op", "u1"), ("pad0", "u1"), ("pad1", "<u2"), ("width", "<u4"),
                             ("a", "<i8"), ("b", "<i8"), ("c", "<i8"), ("imm0", "<u4"),
                             ("imm1", "<u4"), ("name_off", "<u4"), ("name_len", "<u4"),
                             ("const_off", "<u4"), ("pad2", "<u4")])
SMT_RESULT_DTYPE = np.dtype([("kind", "<u4"), ("pad", "<u4"), ("node", "<i8")])
assert SMT_RECORD_DTYPE.itemsize == 56 and SMT_RESULT_DTYPE.itemsize == 16
SMT_ASSERT, SMT_MINIMIZE, SMT_MAXIMIZE = 0, 1, 2


class SmtBatch(C.Structure):
    _fields_ = [("records", _vp), ("n_records", C.c_uint64), ("const_limbs", _vp),
                ("names", _vp), ("results", _vp), ("n_results", C.c_uint64)]


# mh_microbench_issue kinds (include/mythril_hip.h)
MB_KINDS = ("add_co_chain", "mad_u64_u32", "add_u32", "xor_b32", "alignbit_b32", "cndmask_b32",
            "or3_b32", "readlane_b32", "mov_b32", "add_co_nocarryin", "sub_co_vcc_chain",
            "cndmask_e32_vcc", "cmp_eq_e32", "xor_literal", "lshlrev_b32", "add3_u32", "fma_f64",
            "xnor_b32", "and_b32", "or_b32", "not_b32", "xor_exec32", "alignbit_exec32",
            "xor_exec16", "xor_exec_alt", "dep_mad_u64_u32", "dep_add_u32", "dep_addc_vcc",
            "dep_mad_2chains", "dep_mad_carry", "dep_cmp_cndmask", "mix_mad_add", "mix_addc_xor",
            "mix_mad2_add2", "bitop3_b32", "mix_bitop3_alignbit", "cmp_lt_u64", "cmp_eq_u64",
            "lshl_add_u64", "mul_lo_u32", "mul_hi_u32", "mul_u32_u24", "sub_co_e64_sgpr",
            "cmp_lt_u32_e64", "lt256_via_u64")


class NativeUnavailable(RuntimeError):
    """libmythril_hip.so is missing or cannot be loaded."""


class SieveError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("mythril_hip error %d: %s" % (code, msg))
        self.code = code


class Unsupported(SieveError):
    """The tape uses something the device path does not cover: fall back to z3."""


class TapeInfo(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_uint32),
        ("n_insns", C.c_uint32),
        ("n_regs", C.c_uint32),
        ("features", C.c_uint32),
        ("alg_ops", C.c_uint64),
    ]


class JitInfo(C.Structure):
    """mh_jit_info (include/mythril_hip.h)."""

    _fields_ = [
        ("n_jitted", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_modules", C.c_uint32),
        ("max_vgpr", C.c_uint32),
        ("code_bytes", C.c_uint64),
        ("valu_static", C.c_uint64),
        ("valu_wide_static", C.c_uint64),
        ("build_ms", C.c_double),
    ]


JIT_VALUES = 1
JIT_FULL_EVAL = 2


class Guide(C.Structure):
    """mh_guide (include/mythril_hip.h)."""

    _fields_ = [
        ("n_cols", C.c_uint32),
        ("col_width", C.POINTER(C.c_uint16)),
        ("pool_off", _u32p),
        ("pool", _u32p),
        ("n_sets", C.c_uint32),
        ("set_prob", C.POINTER(C.c_uint8)),
        ("set_off", _u32p),
        ("alt_off", _u32p),
        ("entry_col", _u32p),
        ("entry_val", _u32p),
    ]


class RoundJob(C.Structure):
    """mh_round_job (include/mythril_hip.h)."""

    _fields_ = [
        ("ts", _vp), ("as_", _vp), ("guide", C.POINTER(Guide)),
        ("seed", C.c_uint64), ("global_base", C.c_uint64), ("count", C.c_uint64),
        ("tape_first", C.c_uint32), ("tape_count", C.c_uint32), ("mode", C.c_uint32),
        ("n_cols", C.c_uint32),
        ("first_hit", _u64p), ("hit_count", _u64p), ("rows_out", _u32p),
    ]


ROUND_MANY_MAX = 256  # MH_ROUND_MANY_MAX


class ValuesJob(C.Structure):
    """mh_values_job (include/mythril_hip.h)."""

    _fields_ = [
        ("ts", _vp), ("tables", _vp), ("tapes", _u32p), ("n", C.c_uint32), ("as_", _vp),
        ("row", C.c_uint64), ("out", _u32p),
    ]


VALUES_JOBS_MAX = 256  # MH_VALUES_JOBS_MAX

_lib: Optional[C.CDLL] = None


def _limb_rows(vals) -> np.ndarray:
    """[n, 8] u32 limbs of 256-bit values."""
    buf = b"".join((int(v) & ((1 << 256) - 1)).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u4").reshape(-1, 8).copy()


def _guide_struct(arrays: dict):
    """An mh_guide over guide arrays (candidates.Guide.arrays()), and the arrays it points into
    (the caller keeps them alive for the call)."""
    dts = dict(width=np.uint16, set_prob=np.uint8)
    a = {k: np.ascontiguousarray(v, dtype=dts.get(k, np.uint32)) for k, v in arrays.items()}
    n_cols = len(a["width"])
    n_sets = len(a["set_off"]) - 1
    g = Guide(n_cols, a["width"].ctypes.data_as(C.POINTER(C.c_uint16)), _ptr(a["pool_off"]),
              _ptr(a["pool"]), n_sets, a["set_prob"].ctypes.data_as(C.POINTER(C.c_uint8)),
              _ptr(a["set_off"]), _ptr(a["alt_off"]), _ptr(a["entry_col"]),
              _ptr(a["entry_val"]))
    return g, a


def _guide_arrays(g: "Guide") -> dict:
    """The arrays of an mh_guide the library owns, copied (one memcpy each)."""
    def arr(p, n, dt=np.uint32):
        dt = np.dtype(dt)
        return np.frombuffer(C.string_at(C.cast(p, C.c_void_p), n * dt.itemsize), dtype=dt)

    n_cols, n_sets = g.n_cols, g.n_sets
    pool_off = arr(g.pool_off, n_cols + 1)
    set_off = arr(g.set_off, n_sets + 1)
    alt_off = arr(g.alt_off, int(set_off[-1]) + 1)
    n_entries = max(int(alt_off[-1]), 1)
    return dict(
        width=arr(g.col_width, n_cols, np.uint16), pool_off=pool_off,
        pool=arr(g.pool, 8 * max(int(pool_off[-1]), 1)).reshape(-1, 8), set_off=set_off,
        set_prob=arr(g.set_prob, max(n_sets, 1), np.uint8), alt_off=alt_off,
        entry_col=arr(g.entry_col, n_entries), entry_val=arr(g.entry_val, 8 * n_entries).reshape(-1, 8))


class GuideHandle:
    """A harvested guide left in the library (mh_harvest): query_round hands its mh_guide to the
    generator as it is; arrays() copies it out (tests, the CPU stand-in of the device)."""

    def __init__(self, lib, h: C.c_void_p, g: "Guide"):
        self.lib, self.h, self.guide = lib, h, g

    def arrays(self) -> dict:
        return _guide_arrays(self.guide)

    def set_conjuncts(self) -> np.ndarray:
        """Per set of the guide: the root-tape node id of the conjunct that contributed it, or
        NO_CONJUNCT for the parent, hint and shared interval sets (mh_harvest_set_conjuncts)."""
        n = int(self.guide.n_sets)
        out = np.zeros(max(n, 1), dtype=np.uint32)
        _check(self.lib.mh_harvest_set_conjuncts(self.h, _ptr(out), n))
        return out[:n]

    def close(self) -> None:
        if self.h:
            self.lib.mh_harvest_free(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def harvest_guide(nodes: np.ndarray, consts: np.ndarray, widths: Sequence[int],
                  parent: Sequence[Tuple[int, int]] = (), session: "Optional[GuideSession]" = None,
                  keep: bool = False, parent_eval: bool = False):
    """mh_guide_harvest: the guide of one lowered query tape (root last, VAR imm0 = column,
    CONST imm0 = row of `consts`), as the arrays candidates.Guide.arrays() gives -- the same
    values (tests/test_harvest.py).  `parent` = the parent witness as (column, value) pairs in
    the witness's order.  With `session` (a GuideSession) the harvest reuses the session's memo
    when the tape extends the last one (mh_guide_harvest_with; the same arrays).  keep=True
    returns a GuideHandle instead (the guide stays in the library for query_round).  Host-only:
    no device is touched."""
    lib = load()
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    consts = np.ascontiguousarray(consts, dtype=np.uint32).reshape(-1, 8)
    w = np.ascontiguousarray(widths, dtype=np.uint16)
    pc = np.ascontiguousarray([c for c, _ in parent], dtype=np.uint32)
    pv = _limb_rows([v for _, v in parent]) if len(parent) else np.zeros((1, 8), np.uint32)
    h = C.c_void_p()
    g = Guide()
    args = (nodes.ctypes.data, len(nodes), _ptr(consts), len(consts),
            w.ctypes.data_as(C.POINTER(C.c_uint16)), len(w), _ptr(pc), _ptr(pv), len(pc),
            C.byref(h), C.byref(g))
    if parent_eval:  # mh_guide_harvest_inc: operands the parent fixes count as known
        if session is not None:
            raise ValueError("parent_eval harvests are stateless")
        _check(lib.mh_guide_harvest_inc(*args))
    elif session is None:
        _check(lib.mh_guide_harvest(*args))
    else:
        _check(lib.mh_guide_harvest_with(session.h, *args))
    handle = GuideHandle(lib, h, g)
    if keep:
        return handle
    try:
        return handle.arrays()
    finally:
        handle.close()


class GuideSession:
    """An mh_harvester: guide harvests that reuse the memo of the path's earlier queries."""

    def __init__(self):
        self.lib = load()
        h = C.c_void_p()
        _check(self.lib.mh_harvester_create(C.byref(h)))
        self.h = h

    def stats(self) -> Tuple[int, int, int]:
        """(harvests that extended the last tape, harvests that started afresh, arena bytes)."""
        out = (C.c_uint64 * 3)()
        _check(self.lib.mh_harvester_stats(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def close(self) -> None:
        if self.h:
            self.lib.mh_harvester_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass


class SmtlibSession:
    """An SMT-LIB reader session (mh_smtlib): reads z3-printed text into a term builder,
    handing over only the nodes the builder does not have yet (include/mythril_hip.h)."""

    def __init__(self):
        self.lib = load()
        h = C.c_void_p()
        _check(self.lib.mh_smtlib_create(C.byref(h)))
        self.h = h

    def close(self) -> None:
        if self.h:
            self.lib.mh_smtlib_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    def size(self) -> int:
        return int(self.lib.mh_smtlib_size(self.h))

    def read(self, text: str, b) -> List[Tuple[int, int]]:
        """Parse `text` into builder `b`; [(SMT_ASSERT / MINIMIZE / MAXIMIZE, node)]."""
        data = text.encode()
        batch = SmtBatch()
        _check(self.lib.mh_smtlib_read(self.h, data, len(data), C.byref(batch)))
        n = int(batch.n_records)
        ids: List[int] = []
        if n:
            try:
                ids = self._merge(batch, n, b)
            except Exception:
                self.lib.mh_smtlib_rollback(self.h)
                raise
            arr = (C.c_int64 * n)(*ids)
            _check(self.lib.mh_smtlib_commit(self.h, arr, n))
        out = []
        nr = int(batch.n_results)
        if nr:
            res = np.frombuffer((C.c_char * (nr * 16)).from_address(batch.results),
                                dtype=SMT_RESULT_DTYPE)
            for kind, _, node in res.tolist():
                out.append((kind, node if node >= 0 else ids[-node - 1]))
        return out

    @staticmethod
    def _merge(batch, n: int, b) -> List[int]:
        """Build the batch's records in builder `b` (TapeBuilder._add's bookkeeping inlined for
        the plain ops: the reader checked their sorts with TapeBuilder.op's rules)."""
        from .tape import ARITY, F_HOST

        recs = np.frombuffer((C.c_char * (n * 56)).from_address(batch.records),
                             dtype=SMT_RECORD_DTYPE).tolist()
        nl = max((r[9] + r[10] for r in recs), default=0)
        names = C.string_at(batch.names, nl).decode() if nl else ""
        nc = max((r[11] + 8 for r in recs if r[0] == 0), default=0)
        cbuf = C.string_at(batch.const_limbs, 4 * nc) if nc else b""
        arity = _ARITY_BY_INT or _arity_table(ARITY)
        from .tape import NODE_PACK

        memo, nodes, widths, flags, packed = b._memo, b.nodes, b.widths, b.flags, b.node_bytes
        ids = [0] * n
        for k, (op, _, _, w, a, bb, c, i0, i1, noff, nlen, coff, _) in enumerate(recs):
            if a < 0:
                a = ids[-a - 1]
            if bb < 0:
                bb = ids[-bb - 1]
            if c < 0:
                c = ids[-c - 1]
            if 2 <= op < 80:  # plain ops (TRUE / FALSE included): TapeBuilder._add
                key = (op, w, a, bb, c, i0, i1)
                h = memo.get(key)
                if h is None:
                    ar = arity[op]
                    if op == 30 and widths[a] > 256:
                        f = F_HOST
                    elif ar:
                        f = (flags[a] | (flags[bb] if ar > 1 else 0)
                             | (flags[c] if ar > 2 else 0)) & F_HOST
                    else:
                        f = 0
                    h = len(nodes)
                    nodes.append(key)
                    widths.append(w)
                    flags.append(f)
                    packed += NODE_PACK(op, f, w, a, bb, c, i0, i1)
                    memo[key] = h
            elif op == 0:  # CONST (<= 256 bits; wider ones arrive as CONCATs)
                h = b.const(int.from_bytes(cbuf[4 * coff:4 * coff + 32], "little"), w)
            elif op == 1:
                h = b.user_var(names[noff:noff + nlen], w)
            elif op == 80:
                h = b.array(names[noff:noff + nlen], i1, w)
            elif op == 81:
                h = b.const_array(i1, a)
            elif op == 82:
                h = b.store(a, bb, c)
            elif op == 83:
                h = b.select(a, bb)
            else:
                h = b.apply(names[noff:noff + nlen], i1, w, a)
            ids[k] = h
        return ids


# mh_query_column / mh_query_table (include/mythril_hip.h)
QUERY_COLUMN_DTYPE = np.dtype([("name_off", "<u4"), ("name_len", "<u4"), ("symbol_off", "<u4"),
                               ("symbol_len", "<u4"), ("width", "<u4"), ("kind", "<u4"),
                               ("key_off", "<u4"), ("pad", "<u4")])
QUERY_TABLE_DTYPE = np.dtype([("kind", "<u4"), ("name_off", "<u4"), ("name_len", "<u4"),
                              ("limb_off", "<u4"), ("n_items", "<u4"), ("pad", "<u4")])
assert QUERY_COLUMN_DTYPE.itemsize == 32 and QUERY_TABLE_DTYPE.itemsize == 24
COLUMN_KINDS = ("var", "cell", "else", "ufcell", "ufelse", "read", "ufread", "kread")  # MH_COL_*
TERMS_KECCAK_READS = 1  # mh_terms_set_options
TABLE_CELLS, TABLE_UF_CELLS, TABLE_KECCAK = 0, 1, 2
QUERY_DEFINITIONS = 1
QUERY_REFUTED = 2
QUERY_INCREMENTAL = 4  # diagnostic: built from the session's state, not afresh
QUERY_KEY_LIMBS = 36


class QueryInfo(C.Structure):
    """mh_query_info (include/mythril_hip.h)."""

    _fields_ = [("nodes", _vp), ("tape_off", _u64p), ("consts", _u32p), ("columns", _vp),
                ("names", _vp), ("key_limbs", _u32p), ("group_cols", _u32p),
                ("group_off", _u32p), ("tables", _vp), ("table_limbs", _u32p),
                ("n_tapes", C.c_uint32), ("n_consts", C.c_uint32), ("n_columns", C.c_uint32),
                ("names_len", C.c_uint32), ("n_groups", C.c_uint32), ("n_tables", C.c_uint32),
                ("flags", C.c_uint32), ("n_keys", C.c_uint32), ("n_table_entries", C.c_uint32),
                ("n_defs", C.c_uint32), ("def_cols", _u32p), ("parent_len", C.c_uint32),
                ("root_ends", _u32p), ("n_root_ends", C.c_uint32)]


class CompiledQuery:
    """What mh_query_build returns, copied out of the library: the tapes (tape 0 the root; with
    several groups, tapes 1.. the groups'), the query constants, the column names and widths,
    each group's column indices and the flags; ``columns`` [(name, width, kind, symbol, key)] and
    ``tables`` [(kind, name, items)] are decoded on first use (a witness's schema is read only
    when a model is evaluated, mythril/laser/smt/model.py:45-59)."""

    __slots__ = ("tapes", "consts", "names", "widths", "groups", "flags", "nodes", "tape_off",
                 "defs", "def_tapes", "parent_len", "root_ends", "_raw", "_columns", "_tables")

    def __init__(self, info: QueryInfo):
        def raw(p, nbytes):
            return C.string_at(p, nbytes) if nbytes else b""

        nd = info.n_defs
        nt = info.n_tapes - nd  # the root and group tapes; the definitions' tapes follow
        off = np.frombuffer(raw(info.tape_off, 8 * (info.n_tapes + 1)),
                            dtype=np.uint64).tolist()
        nodes = np.frombuffer(raw(info.nodes, 24 * off[-1]), dtype=NODE_DTYPE)
        self.nodes, self.tape_off = nodes, off[:nt + 1]  # root and group tapes back to back
        self.tapes = [nodes[off[i]:off[i + 1]] for i in range(nt)]
        # MH_QUERY_DEFINITIONS: column index of each defined symbol, and the tape of its term
        self.defs = np.frombuffer(raw(info.def_cols, 4 * nd), dtype=np.uint32).tolist()
        self.def_tapes = [nodes[off[nt + i]:off[nt + i + 1]] for i in range(nd)]
        self.consts = np.frombuffer(raw(info.consts, 32 * info.n_consts),
                                    dtype=np.uint32).reshape(-1, 8)
        names = raw(info.names, info.names_len).decode()
        cols = np.frombuffer(raw(info.columns, 32 * info.n_columns), dtype=QUERY_COLUMN_DTYPE)
        no, nl = cols["name_off"].tolist(), cols["name_len"].tolist()
        self.names = [names[o:o + n] for o, n in zip(no, nl)]
        self.widths = cols["width"]
        ng = info.n_groups
        goff = np.frombuffer(raw(info.group_off, 4 * (ng + 1)), dtype=np.uint32).tolist()
        gcols = np.frombuffer(raw(info.group_cols, 4 * goff[-1]), dtype=np.uint32).tolist()
        self.groups = [gcols[goff[g]:goff[g + 1]] for g in range(ng)]
        self.flags = int(info.flags)
        self.parent_len = int(info.parent_len)  # root-tape nodes of the query minus its last root
        # root_ends[d - 1]: root-tape nodes of the query's first d roots
        self.root_ends = np.frombuffer(raw(info.root_ends, 4 * info.n_root_ends),
                                       dtype=np.uint32).tolist()
        kb = 4 * QUERY_KEY_LIMBS
        self._raw = (names, cols, raw(info.key_limbs, kb * info.n_keys),
                     raw(info.tables, 24 * info.n_tables),
                     raw(info.table_limbs, kb * info.n_table_entries))
        self._columns = self._tables = None

    @staticmethod
    def _ints(data: bytes) -> List[int]:
        k = 4 * QUERY_KEY_LIMBS
        return [int.from_bytes(data[i:i + k], "little") for i in range(0, len(data), k)]

    @property
    def columns(self) -> List[tuple]:
        if self._columns is None:
            names, cols, key_limbs, _, _ = self._raw
            keys = self._ints(key_limbs)
            self._columns = [(names[no:no + nl], w, COLUMN_KINDS[k], names[so:so + sl],
                              None if ko == 0xFFFFFFFF else keys[ko])
                             for no, nl, so, sl, w, k, ko, _ in cols.tolist()]
        return self._columns

    def column_kinds(self) -> List[int]:
        """MH_COL_* per column, without decoding the columns."""
        return self._raw[1]["kind"].tolist()

    def has_keccak_table(self) -> bool:
        """Whether the lowering made an MH_TABLE_KECCAK table, without decoding the tables."""
        return bool((np.frombuffer(self._raw[3], dtype=QUERY_TABLE_DTYPE)["kind"]
                     == TABLE_KECCAK).any())

    @property
    def tables(self) -> List[tuple]:
        if self._tables is None:
            names, _, _, tabs, limbs = self._raw
            vals = self._ints(limbs)
            self._tables = [
                (k, names[no:no + nl], vals[lo:lo + (2 * n + 1 if k == TABLE_KECCAK else n)])
                for k, no, nl, lo, n, _ in np.frombuffer(tabs, dtype=QUERY_TABLE_DTYPE).tolist()]
        return self._tables


def _ints(rows: np.ndarray) -> List[int]:
    """[n, k] u32 limbs -> n ints."""
    rows = np.ascontiguousarray(rows, dtype="<u4")
    data, k = rows.tobytes(), 4 * rows.shape[1]
    return [int.from_bytes(data[k * i:k * i + k], "little") for i in range(len(rows))]


class TermMirror:
    """An mh_terms session mirroring one TapeBuilder (tape.py): each sync hands the library the
    nodes, constants and names the builder made since the last one; build() compiles a query
    (mh_query_build).  One per builder and lowering mode, kept on it (``TermMirror.of``);
    ``keccak_reads``: keccak applications as read columns (MH_TERMS_KECCAK_READS, lower_query's
    keyword of that name)."""

    def __init__(self, keccak_reads: bool = False):
        import threading

        self.lib = load()
        h = C.c_void_p()
        _check(self.lib.mh_terms_create(C.byref(h)))
        self.h = h
        self.keccak_reads = keccak_reads
        if keccak_reads:
            _check(self.lib.mh_terms_set_options(h, TERMS_KECCAK_READS))
        self.n = [0, 0, 0, 0, 0]  # nodes, constants, variables, arrays, functions sent
        # one session per builder, used by one thread at a time (query.cpp keeps scratch and the
        # last query's state on it): sieves of several threads over one builder take turns
        self.lock = threading.Lock()

    @classmethod
    def of(cls, b, keccak_reads: bool = False) -> "TermMirror":
        attr = "_term_mirror_kr" if keccak_reads else "_term_mirror"
        m = b.__dict__.get(attr)
        if m is None:  # setdefault: two threads racing here end up with the same session
            m = b.__dict__.setdefault(attr, cls(keccak_reads))
        return m

    def close(self) -> None:
        if self.h:
            self.lib.mh_terms_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    def sync(self, b) -> None:
        n0, c0, v0, a0, f0 = self.n
        n1 = len(b.nodes)
        pool = b.pool
        c1 = len(pool.values)
        v1 = len(b.var_index)
        sym = b.symbols
        a1, f1 = len(sym.array_names), len(sym.function_names)
        if [n1, c1, v1, a1, f1] == self.n:
            return
        if n1 > n0:
            k = n1 - n0
            packed = getattr(b, "node_bytes", None)
            if packed is not None and len(packed) == 24 * n1:
                # the builder's packed mh_node records (the slice is a copy: nothing of the
                # builder's stays exported)
                nodes = np.frombuffer(bytes(packed[24 * n0:24 * n1]), dtype=NODE_DTYPE)
            else:
                rows = np.fromiter(chain.from_iterable(b.nodes[n0:n1]), np.int64, 7 * k).reshape(k, 7)
                nodes = np.empty(k, dtype=NODE_DTYPE)
                nodes["op"] = rows[:, 0]
                nodes["flags"] = np.fromiter(b.flags[n0:n1], np.uint8, k)
                nodes["width"] = rows[:, 1]
                for j, f in enumerate(("a", "b", "c", "imm0", "imm1")):
                    nodes[f] = rows[:, 2 + j]
        else:
            nodes = np.zeros(1, dtype=NODE_DTYPE)
        consts = (np.ascontiguousarray(pool.to_array()[c0:c1]) if c1 > c0
                  else np.zeros((1, 8), dtype=np.uint32))

        def names(seq) -> bytes:
            return b"".join(s.encode() + b"\0" for s in seq)

        vn = names(list(b.var_index)[v0:v1]) if v1 > v0 else b""
        an = names(sym.array_names[a0:a1]) if a1 > a0 else b""
        fn = names(sym.function_names[f0:f1]) if f1 > f0 else b""
        _check(self.lib.mh_terms_append(self.h, nodes.ctypes.data, n1 - n0, _ptr(consts), c1 - c0,
                                        vn, v1 - v0, an, a1 - a0, fn, f1 - f0))
        self.n = [n1, c1, v1, a1, f1]

    def build(self, b, roots: Sequence[int]) -> CompiledQuery:
        """mh_query_build of the conjunction of `roots` (after a sync with `b`)."""
        r = np.ascontiguousarray(roots, dtype=np.uint32)
        with self.lock:
            self.sync(b)
            h = C.c_void_p()
            info = QueryInfo()
            _check(self.lib.mh_query_build(self.h, _ptr(r), len(r), C.byref(h), C.byref(info)))
            try:
                return CompiledQuery(info)
            finally:
                self.lib.mh_query_free(h)


_ARITY_BY_INT: List[int] = []


def _arity_table(arity) -> List[int]:
    _ARITY_BY_INT[:] = [arity.get(o, 2) for o in range(256)]
    return _ARITY_BY_INT


def load(path: str = LIB_PATH) -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NativeUnavailable(
            "%s not built; run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
    try:
        lib = C.CDLL(path)
    except OSError as e:  # pragma: no cover - depends on the ROCm runtime
        raise NativeUnavailable("cannot load %s: %s" % (path, e)) from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(code: int) -> None:
    if code != MH_OK:
        msg = load().mh_last_error().decode(errors="replace")
        if code == MH_E_UNSUPPORTED:
            raise Unsupported(code, msg)
        raise SieveError(code, msg)


def _ptr(a: np.ndarray, t=C.c_uint32):
    return a.ctypes.data_as(C.POINTER(t))


def version() -> Tuple[int, int, int]:
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(load().mh_version(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def device_count() -> int:
    n = C.c_int32()
    _check(load().mh_device_count(C.byref(n)))
    return n.value


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """A fresh RCCL unique id (rank 0 creates it; every rank passes it to Context.comm_init)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(load().mh_comm_unique_id(C.cast(buf, C.c_void_p)))
    return bytes(buf)


_CODE_IDS = {}


def jit_code_id(tapeset: TapeSet, short_circuit: bool = True, max_vgpr: int = 0) -> str:
    """Identifier of the native code mh_tapes_jit would build for `tapeset` (mh_jit_code_id):
    a hash of the emitted module texts, computed on the host without a device or the assembler.
    Equal to CompiledTapes.code_id() after CompiledTapes.jit() with the same options."""
    nodes, offs, consts = tapeset.flatten()
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    consts = np.ascontiguousarray(consts, dtype=np.uint32)
    out = C.c_uint64()
    _check(load().mh_jit_code_id(nodes.ctypes.data_as(C.c_void_p), _ptr(offs, C.c_uint64),
                                 len(tapeset.tapes), _ptr(consts), len(tapeset.pool.values),
                                 tapeset.n_vars, 0 if short_circuit else JIT_FULL_EVAL, max_vgpr,
                                 C.byref(out)))
    return "%016x" % out.value


def _elf_section(path: str, name: bytes) -> bytes:
    """The bytes of one section of a 64-bit little-endian ELF file."""
    import struct

    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:
        raise ValueError("%s: not a 64-bit little-endian ELF" % path)
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)

    def sh(i):  # (name offset, offset, size)
        b = shoff + i * shentsize
        nm, = struct.unpack_from("<I", data, b)
        off, size = struct.unpack_from("<QQ", data, b + 0x18)
        return nm, off, size

    _, stroff, _ = sh(shstrndx)
    for i in range(shnum):
        nm, off, size = sh(i)
        end = data.index(b"\0", stroff + nm)
        if data[stroff + nm:end] == name:
            return data[off:off + size]
    raise ValueError("%s: no section %r" % (path, name))


def interp_code_id() -> str:
    """Identifier of the interpreter's and the generator's device code: a hash of the code objects
    libmythril_hip.so embeds (its .hip_fatbin section: sieve_kernels.hip, generate.hip and the
    micro-benchmarks), so a host-only edit leaves it unchanged."""
    import hashlib

    return hashlib.sha256(_elf_section(LIB_PATH, b".hip_fatbin")).hexdigest()[:16]


def codegen_id(engine: str = "jit", variant: str = "plain", short_circuit: bool = True) -> str:
    """Identifier of the code one engine runs on bench.py's workload ("jit": the native code
    emitted for the config-5 tape set of `variant`, jit_code_id; "interp": the device code objects
    of the library, interp_code_id).  Profiles that price this code (profiles/pmc_summary.json,
    profiles/alg_work.json) record it, and bench.py uses a profile only for the code it runs."""
    key = (engine, variant, short_circuit)
    if key not in _CODE_IDS:
        if engine == "interp":
            _CODE_IDS[key] = interp_code_id()
        else:
            from . import synth

            ts = synth.generate(None, keccak=variant == "keccak")
            _CODE_IDS[key] = jit_code_id(ts, short_circuit=short_circuit)
    return _CODE_IDS[key]


def gen_limb(seed: int, var: int, index: int, limb: int) -> int:
    return int(load().mh_gen_limb(seed, var, index, limb))


class Context:
    """One GPU + one stream (mh_ctx)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = C.c_void_p()
        _check(self.lib.mh_ctx_create(device, C.byref(h)))
        self.h = h
        self.device = device

    def set_stream(self, stream_ptr: Optional[int]) -> None:
        _check(self.lib.mh_ctx_set_stream(self.h, C.c_void_p(stream_ptr or 0)))

    def synchronize(self) -> None:
        _check(self.lib.mh_ctx_synchronize(self.h))

    def clear_cache(self) -> None:
        """Drop the compiled tapes mh_tapes_compile keeps by content (mh_ctx_clear_cache)."""
        _check(self.lib.mh_ctx_clear_cache(self.h))

    def close(self) -> None:
        if self.h:
            self.lib.mh_ctx_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def compile(self, tapeset: TapeSet) -> "CompiledTapes":
        return CompiledTapes(self, tapeset)

    def compile_async(self, tapeset: TapeSet) -> "PendingCompile":
        """mh_tapes_compile_async: the compile runs on the context's worker thread; the caller
        does host-only work meanwhile (no other call on this context) and then .wait()s."""
        return PendingCompile(self, tapeset)

    def assignments(self, n_vars: int, capacity: int) -> "Assignments":
        return Assignments(self, n_vars, capacity)

    def enable_timing(self, on: bool = True) -> None:
        _check(self.lib.mh_ctx_enable_timing(self.h, 1 if on else 0))

    def kernel_time(self) -> Tuple[float, int]:
        """(summed ms, launches) of the sieve launches timed since the last call."""
        ms, n = C.c_double(), C.c_uint64()
        _check(self.lib.mh_ctx_kernel_time(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def comm_init(self, unique_id: bytes, rank: int, world: int) -> None:
        """One RCCL communicator for this ctx (mh_comm_init)."""
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(self.lib.mh_comm_init(self.h, C.cast(buf, C.c_void_p), rank, world))

    def comm_allreduce(self, d_first_hit: int, d_hit_count: int, n: int) -> None:
        """MIN of first witnesses, SUM of counts over the ranks, in place (device buffers)."""
        _check(self.lib.mh_comm_allreduce_results(self.h, C.c_void_p(d_first_hit),
                                                  C.c_void_p(d_hit_count), n))

    def comm_destroy(self) -> None:
        _check(self.lib.mh_comm_destroy(self.h))

    def microbench(self, kind: int, waves_per_simd: int = 8) -> float:
        """Sustained lane-ops/s of one instruction kind (mh_microbench_issue; MB_KINDS)."""
        v = C.c_double()
        _check(self.lib.mh_microbench_issue(self.h, kind, waves_per_simd, C.byref(v)))
        return v.value


def _compile_args(tapeset: TapeSet):
    nodes, offs, consts = tapeset.flatten()
    return (np.ascontiguousarray(nodes, dtype=NODE_DTYPE), np.ascontiguousarray(offs, dtype=np.uint64),
            np.ascontiguousarray(consts, dtype=np.uint32))


class PendingCompile:
    """A compile on the context's worker thread (Context.compile_async); its input arrays are
    held here until wait() returns the CompiledTapes."""

    def __init__(self, ctx: Context, tapeset: TapeSet):
        import time

        self.ctx, self.tapeset = ctx, tapeset
        t0 = time.perf_counter()
        args = _compile_args(tapeset)
        nodes, offs, consts = args
        self.t1 = time.perf_counter()
        self.flatten_s = self.t1 - t0
        _check(ctx.lib.mh_tapes_compile_async(
            ctx.h, nodes.ctypes.data_as(C.c_void_p), _ptr(offs, C.c_uint64), len(tapeset.tapes),
            _ptr(consts), len(tapeset.pool.values), tapeset.n_vars))
        # held from here on, and only once the compile is queued: a refused call (another
        # compile pending) leaves nothing for __del__ to collect -- it would take the other's
        self.args = args

    def wait(self) -> "CompiledTapes":
        import time

        h, secs = C.c_void_p(), C.c_double()
        try:
            _check(self.ctx.lib.mh_tapes_compile_wait(self.ctx.h, C.byref(h), C.byref(secs)))
        finally:
            self.args = None
        # timing: host flatten, the compile's own seconds on the worker (it overlapped the
        # caller's work; the wait itself is what the caller paid for it)
        self.wait_s = time.perf_counter() - self.t1
        return CompiledTapes(self.ctx, self.tapeset, _handle=h,
                             _timing=(self.flatten_s, secs.value))

    def __del__(self):  # dropped without wait(): collect the compile (the worker still reads the
        # input arrays this object holds) and free its tapes
        if getattr(self, "args", None) is not None and getattr(self.ctx, "h", None):
            try:
                self.wait().close()
            except Exception:  # noqa: BLE001 - interpreter shutdown, a failed compile
                pass


class CompiledTapes:
    """mh_tapeset: tapes lowered to device code, resident in HBM."""

    def __init__(self, ctx: Context, tapeset: TapeSet, _handle=None, _timing=None):
        import time

        self.ctx = ctx
        if _handle is not None:  # from PendingCompile.wait
            self.h = _handle
            self.timing = _timing
            self.n_tapes = len(tapeset.tapes)
            self.n_vars = tapeset.n_vars
            return
        t0 = time.perf_counter()
        nodes, offs, consts = _compile_args(tapeset)
        h = C.c_void_p()
        t1 = time.perf_counter()
        _check(ctx.lib.mh_tapes_compile(
            ctx.h, nodes.ctypes.data_as(C.c_void_p), _ptr(offs, C.c_uint64), len(tapeset.tapes),
            _ptr(consts), len(tapeset.pool.values), tapeset.n_vars, C.byref(h)))
        self.h = h
        # host flatten / native compile+upload seconds (per-stage latency reports)
        self.timing = (t1 - t0, time.perf_counter() - t1)
        self.n_tapes = len(tapeset.tapes)
        self.n_vars = tapeset.n_vars

    def jit(self, values: bool = False, max_vgpr: int = 0, short_circuit: bool = True) -> dict:
        """Compile the tapes the JIT covers to native gfx950 code (mh_tapes_jit); later runs
        over the whole set use it.  short_circuit=False evaluates every conjunct of every row
        (MH_JIT_FULL_EVAL; same results).  Returns mh_tapes_jit_info as a dict."""
        flags = (JIT_VALUES if values else 0) | (0 if short_circuit else JIT_FULL_EVAL)
        _check(self.ctx.lib.mh_tapes_jit(self.h, flags, max_vgpr))
        return self.jit_info()

    def code_id(self) -> str:
        """Identifier of the native code jit() built (mh_tapes_jit_code_id; see jit_code_id)."""
        out = C.c_uint64()
        _check(self.ctx.lib.mh_tapes_jit_code_id(self.h, C.byref(out)))
        return "%016x" % out.value

    def jit_info(self) -> dict:
        ji = JitInfo()
        _check(self.ctx.lib.mh_tapes_jit_info(self.h, C.byref(ji)))
        return {f: getattr(ji, f) for f, _ in JitInfo._fields_}

    def jitted(self) -> np.ndarray:
        out = np.zeros(max(self.n_tapes, 1), dtype=np.uint8)
        _check(self.ctx.lib.mh_tapes_jitted(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            self.n_tapes))
        return out[: self.n_tapes]

    def jit_values(self, assign: "Assignments", row_first: int = 0,
                   row_count: Optional[int] = None) -> np.ndarray:
        """Root values of every jitted tape by the native code: u32 [n_tapes, 8, rows]."""
        rc = assign.capacity - row_first if row_count is None else row_count
        out = np.zeros((self.n_tapes, 8, max(rc, 1)), dtype=np.uint32)
        _check(self.ctx.lib.mh_jit_eval_all(self.ctx.h, self.h, assign.h, row_first, rc,
                                            _ptr(out)))
        return out[:, :, :rc]

    def info(self):
        arr = (TapeInfo * max(self.n_tapes, 1))()
        _check(self.ctx.lib.mh_tapes_info(self.h, C.cast(arr, C.c_void_p), self.n_tapes))
        return [dict(n_nodes=x.n_nodes, n_insns=x.n_insns, n_regs=x.n_regs,
                     features=x.features, alg_ops=x.alg_ops) for x in arr[: self.n_tapes]]

    def spills(self) -> np.ndarray:
        """Spill slots per tape (0: the tape's live values fit the interpreter's registers)."""
        out = np.zeros(max(self.n_tapes, 1), dtype=np.uint32)
        _check(self.ctx.lib.mh_tapes_spills(self.h, _ptr(out), self.n_tapes))
        return out[: self.n_tapes]

    def split_info(self) -> Tuple[int, int, np.ndarray]:
        """(split tapes, their parts in all, parts per tape: 0 for a tape that runs whole)
        (mh_tapes_split_info): what MH_SPLIT_INSNS made of the set at compile time."""
        n_split, n_parts = C.c_uint32(), C.c_uint32()
        out = np.zeros(max(self.n_tapes, 1), dtype=np.uint32)
        _check(self.ctx.lib.mh_tapes_split_info(self.h, C.byref(n_split), C.byref(n_parts),
                                                out.ctypes.data, self.n_tapes))
        return n_split.value, n_parts.value, out[: self.n_tapes]

    def close(self) -> None:
        if self.h:
            self.ctx.lib.mh_tapes_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class Assignments:
    """mh_assign: candidate assignments, SoA u32 limbs in HBM."""

    def __init__(self, ctx: Context, n_vars: int, capacity: int):
        self.ctx = ctx
        self.n_vars = n_vars
        self.capacity = capacity
        h = C.c_void_p()
        _check(ctx.lib.mh_assign_create(ctx.h, n_vars, capacity, C.byref(h)))
        self.h = h

    def upload(self, soa: np.ndarray, first: int = 0) -> None:
        """soa: u32 array shaped [n_vars, 8, count] (limb 0 least significant)."""
        soa = np.ascontiguousarray(soa, dtype=np.uint32)
        assert soa.shape[:2] == (self.n_vars, 8)
        _check(self.ctx.lib.mh_assign_upload(self.h, _ptr(soa), first, soa.shape[2]))

    def download(self, first: int, count: int) -> np.ndarray:
        out = np.zeros((self.n_vars, 8, count), dtype=np.uint32)
        _check(self.ctx.lib.mh_assign_download(self.h, _ptr(out), first, count))
        return out

    def generate(self, seed: int, global_base: int = 0) -> None:
        _check(self.ctx.lib.mh_assign_generate(self.h, seed, global_base))

    def generate_guided(self, seed: int, arrays: dict, global_base: int = 0, first: int = 0,
                        count: Optional[int] = None) -> None:
        """Rows [first, first+count) from a guide (mythril_amd.candidates.Guide.arrays())."""
        count = self.capacity - first if count is None else count
        g, _keep = _guide_struct(arrays)
        _check(self.ctx.lib.mh_assign_generate_guided(self.h, seed, global_base, first, count,
                                                      C.byref(g)))

    def scatter(self, first: int, cols: Sequence[int], values: np.ndarray) -> None:
        """values u32 [n_rows, len(cols), 8] into columns `cols` (strictly ascending) of rows
        [first, first + n_rows); the rows' other columns keep their content
        (mh_assign_scatter; queued on the ctx stream)."""
        cols, values = _scatter_arrays(cols, values)
        _check(self.ctx.lib.mh_assign_scatter(self.h, first, values.shape[0], _ptr(cols),
                                              len(cols), _ptr(values)))

    def enumerate(self, domains: "Domains", global_base: int = 0, first: int = 0,
                  count: Optional[int] = None) -> None:
        """Rows [first, first+count) get rows global_base.. of the domains' cross product
        (mh_assign_enumerate; decide.enumerate_rows restates it)."""
        count = self.capacity - first if count is None else count
        _check(self.ctx.lib.mh_assign_enumerate(self.h, domains.h, global_base, first, count))

    def close(self) -> None:
        if self.h:
            self.ctx.lib.mh_assign_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def run(ctx: Context, tapes: CompiledTapes, assign: Assignments, *, tape_first: int = 0,
        tape_count: Optional[int] = None, row_first: int = 0, row_count: Optional[int] = None,
        index_base: int = 0, mode: int = MODE_COUNT_ALL):
    """Blocking run; returns (first_hit[u64], hit_count[u64]) per tape."""
    tc = tapes.n_tapes - tape_first if tape_count is None else tape_count
    rc = assign.capacity - row_first if row_count is None else row_count
    fh = np.zeros(max(tc, 1), dtype=np.uint64)
    hc = np.zeros(max(tc, 1), dtype=np.uint64)
    _check(ctx.lib.mh_run(ctx.h, tapes.h, tape_first, tc, assign.h, row_first, rc, index_base,
                          mode, _ptr(fh, C.c_uint64), _ptr(hc, C.c_uint64)))
    return fh[:tc], hc[:tc]


def run_rows(ctx: Context, tapes: CompiledTapes, assign: Assignments, n_cols: int, *,
             tape_first: int = 0, tape_count: Optional[int] = None, row_first: int = 0,
             row_count: Optional[int] = None, index_base: int = 0, mode: int = MODE_FIRST_HIT):
    """Blocking run plus each tape's witness row (mh_run_rows): (first_hit, hit_count,
    rows u32 [tape, column < n_cols, limb]; zero for a tape without a hit)."""
    tc = tapes.n_tapes - tape_first if tape_count is None else tape_count
    rc = assign.capacity - row_first if row_count is None else row_count
    fh = np.zeros(max(tc, 1), dtype=np.uint64)
    hc = np.zeros(max(tc, 1), dtype=np.uint64)
    rows = np.zeros((max(tc, 1), max(n_cols, 1), 8), dtype=np.uint32)
    _check(ctx.lib.mh_run_rows(ctx.h, tapes.h, tape_first, tc, assign.h, row_first, rc,
                               index_base, mode, _ptr(fh, C.c_uint64), _ptr(hc, C.c_uint64),
                               n_cols, _ptr(rows)))
    return fh[:tc], hc[:tc], rows[:tc, :n_cols]


def query_round(ctx: Context, tapes: CompiledTapes, assign: "Assignments", guide: GuideHandle,
                seed: int, global_base: int, count: int, n_cols: int, *, tape_first: int = 0,
                tape_count: Optional[int] = None, mode: int = MODE_FIRST_HIT):
    """One guided round (mh_query_round): rows [0, count) generated from `guide`, then
    run_rows over them with index_base = global_base.  Returns (first_hit, hit_count, rows)."""
    tc = tapes.n_tapes - tape_first if tape_count is None else tape_count
    fh = np.zeros(max(tc, 1), dtype=np.uint64)
    hc = np.zeros(max(tc, 1), dtype=np.uint64)
    rows = np.zeros((max(tc, 1), max(n_cols, 1), 8), dtype=np.uint32)
    _check(ctx.lib.mh_query_round(ctx.h, tapes.h, assign.h, C.byref(guide.guide), seed,
                                  global_base, count, tape_first, tc, mode, _ptr(fh, C.c_uint64),
                                  _ptr(hc, C.c_uint64), n_cols, _ptr(rows)))
    return fh[:tc], hc[:tc], rows[:tc, :n_cols]


class Spares(C.Structure):
    """mh_spares"""
    _fields_ = [("n_rows", C.c_uint32), ("n_cols", C.c_uint32), ("cols", _u32p),
                ("values", _u32p)]


def _scatter_arrays(cols: Sequence[int], values: np.ndarray):
    cols = np.ascontiguousarray(cols, dtype=np.uint32).reshape(-1)
    values = np.ascontiguousarray(values, dtype=np.uint32)
    values = values.reshape(-1, len(cols), 8) if len(cols) else np.zeros((0, 0, 8), np.uint32)
    return cols, values


def _hits_out(tc: int, k: int, n_cols: int):
    k1 = max(k, 1)
    return (np.zeros((max(tc, 1), k1), dtype=np.uint64), np.zeros(max(tc, 1), dtype=np.uint32),
            np.zeros(max(tc, 1), dtype=np.uint64),
            np.zeros((max(tc, 1), k1, max(n_cols, 1), 8), dtype=np.uint32))


def run_hits(ctx: Context, tapes: CompiledTapes, assign: Assignments, k: int, n_cols: int, *,
             tape_first: int = 0, tape_count: Optional[int] = None, row_first: int = 0,
             row_count: Optional[int] = None, index_base: int = 0):
    """The k smallest satisfying rows of every tape (mh_run_hits): (hits [T, k] u64 global
    indices ascending, NO_HIT after the listed ones; n_hits [T] u32; hit_count [T] u64;
    rows [T, k, n_cols, 8] u32, zero for a slot without a hit)."""
    tc = tapes.n_tapes - tape_first if tape_count is None else tape_count
    rc = assign.capacity - row_first if row_count is None else row_count
    hits, nh, hc, rows = _hits_out(tc, k, n_cols)
    _check(ctx.lib.mh_run_hits(ctx.h, tapes.h, tape_first, tc, assign.h, row_first, rc, index_base,
                               k, _ptr(hits, C.c_uint64), _ptr(nh), _ptr(hc, C.c_uint64), n_cols,
                               _ptr(rows)))
    return hits[:tc], nh[:tc], hc[:tc], rows[:tc, :, :n_cols]


def query_round_hits(ctx: Context, tapes: CompiledTapes, assign: "Assignments",
                     guide: GuideHandle, seed: int, global_base: int, count: int, n_cols: int,
                     k: int, *, spares=None, tape_first: int = 0,
                     tape_count: Optional[int] = None):
    """One guided round with a listing (mh_query_round_hits): rows [0, count) generated from
    `guide`; `spares` = (cols, values [n, len(cols), 8]) scattered over rows [0, n); then
    run_hits over the rows with index_base = global_base.  Returns run_hits' tuple."""
    tc = tapes.n_tapes - tape_first if tape_count is None else tape_count
    hits, nh, hc, rows = _hits_out(tc, k, n_cols)
    sp = None
    if spares is not None:
        cols, values = _scatter_arrays(*spares)
        sp = C.byref(Spares(values.shape[0], len(cols), _ptr(cols), _ptr(values)))
    _check(ctx.lib.mh_query_round_hits(ctx.h, tapes.h, assign.h, C.byref(guide.guide), seed,
                                       global_base, count, tape_first, tc, sp, k,
                                       _ptr(hits, C.c_uint64), _ptr(nh), _ptr(hc, C.c_uint64),
                                       n_cols, _ptr(rows)))
    return hits[:tc], nh[:tc], hc[:tc], rows[:tc, :, :n_cols]


def query_round_many(ctx: Context, jobs: Sequence[dict]):
    """Many guided rounds in one device submission (mh_query_round_many).  Each job is a dict
    of query_round's arguments: tapes, assign, guide, seed, global_base, count, n_cols and
    optionally tape_first, tape_count, mode.  Returns per job (first_hit, hit_count, rows), each
    equal to what query_round returns for the job alone; lists beyond ROUND_MANY_MAX jobs go
    up in chunks."""
    out = []
    for lo in range(0, len(jobs), ROUND_MANY_MAX):
        chunk = jobs[lo:lo + ROUND_MANY_MAX]
        arr = (RoundJob * len(chunk))()
        res = []
        for k, j in enumerate(chunk):
            tapes, n_cols = j["tapes"], j["n_cols"]
            tf = j.get("tape_first", 0)
            tc = j.get("tape_count")
            tc = tapes.n_tapes - tf if tc is None else tc
            fh = np.zeros(max(tc, 1), dtype=np.uint64)
            hc = np.zeros(max(tc, 1), dtype=np.uint64)
            rows = np.zeros((max(tc, 1), max(n_cols, 1), 8), dtype=np.uint32)
            arr[k] = RoundJob(tapes.h, j["assign"].h, C.pointer(j["guide"].guide), j["seed"],
                              j["global_base"], j["count"], tf, tc,
                              j.get("mode", MODE_FIRST_HIT), n_cols, _ptr(fh, C.c_uint64),
                              _ptr(hc, C.c_uint64), _ptr(rows))
            res.append((fh, hc, rows, tc, n_cols))
        _check(ctx.lib.mh_query_round_many(ctx.h, arr, len(chunk)))
        out.extend((fh[:tc], hc[:tc], rows[:tc, :n_cols]) for fh, hc, rows, tc, n_cols in res)
    return out


class RoundHitsJob(C.Structure):
    """mh_round_hits_job (include/mythril_hip.h)."""

    _fields_ = [
        ("ts", _vp), ("as_", _vp), ("guide", C.POINTER(Guide)),
        ("seed", C.c_uint64), ("global_base", C.c_uint64), ("count", C.c_uint64),
        ("tape_first", C.c_uint32), ("tape_count", C.c_uint32), ("k", C.c_uint32),
        ("n_cols", C.c_uint32),
        ("spares", C.POINTER(Spares)),
        ("hits", _u64p), ("n_hits", _u32p), ("hit_count", _u64p), ("rows_out", _u32p),
    ]


ROUND_HITS_MANY_MAX_BYTES = 64 << 20  # MH_ROUND_HITS_MANY_MAX_BYTES


def query_round_hits_many(ctx: Context, jobs: Sequence[dict]):
    """Many listing rounds in one device submission (mh_query_round_hits_many).  Each job is a
    dict of query_round_hits' arguments: tapes, assign, guide, seed, global_base, count, n_cols,
    k and optionally spares, tape_first, tape_count.  Returns run_hits' tuple per job, each
    equal to what query_round_hits returns for the job alone; lists beyond ROUND_MANY_MAX jobs
    go up in chunks."""
    out = []
    for lo in range(0, len(jobs), ROUND_MANY_MAX):
        chunk = jobs[lo:lo + ROUND_MANY_MAX]
        arr = (RoundHitsJob * len(chunk))()
        res, keep = [], []
        for i, j in enumerate(chunk):
            tapes, n_cols, k = j["tapes"], j["n_cols"], j["k"]
            tf = j.get("tape_first", 0)
            tc = j.get("tape_count")
            tc = tapes.n_tapes - tf if tc is None else tc
            hits, nh, hc, rows = _hits_out(tc, k, n_cols)
            sp = None
            if j.get("spares") is not None:
                cols, values = _scatter_arrays(*j["spares"])
                sp = Spares(values.shape[0], len(cols), _ptr(cols), _ptr(values))
                keep.append((cols, values, sp))
                sp = C.pointer(sp)
            arr[i] = RoundHitsJob(tapes.h, j["assign"].h, C.pointer(j["guide"].guide), j["seed"],
                                  j["global_base"], j["count"], tf, tc, k, n_cols, sp,
                                  _ptr(hits, C.c_uint64), _ptr(nh), _ptr(hc, C.c_uint64),
                                  _ptr(rows))
            res.append((hits, nh, hc, rows, tc, n_cols))
        _check(ctx.lib.mh_query_round_hits_many(ctx.h, arr, len(chunk)))
        out.extend((hits[:tc], nh[:tc], hc[:tc], rows[:tc, :, :n_cols])
                   for hits, nh, hc, rows, tc, n_cols in res)
    return out


def run_async(ctx: Context, tapes: CompiledTapes, assign: Assignments, d_first_hit: int,
              d_hit_count: int, *, tape_first: int = 0, tape_count: Optional[int] = None,
              row_first: int = 0, row_count: Optional[int] = None, index_base: int = 0,
              mode: int = MODE_COUNT_ALL) -> None:
    """Enqueue on the ctx stream; results accumulate into caller device buffers (u64)."""
    tc = tapes.n_tapes - tape_first if tape_count is None else tape_count
    rc = assign.capacity - row_first if row_count is None else row_count
    _check(ctx.lib.mh_run_async(ctx.h, tapes.h, tape_first, tc, assign.h, row_first, rc,
                                index_base, mode, C.c_void_p(d_first_hit),
                                C.c_void_p(d_hit_count)))


def results_reset(ctx: Context, d_first_hit: int, d_hit_count: int, n: int) -> None:
    _check(ctx.lib.mh_results_reset(ctx.h, C.c_void_p(d_first_hit), C.c_void_p(d_hit_count), n))


def eval_values(ctx: Context, tapes: CompiledTapes, tape: int, assign: Assignments,
                row_first: int = 0, row_count: Optional[int] = None) -> np.ndarray:
    """Root value of `tape` per row: u32 [8, rows] (limb-major)."""
    rc = assign.capacity - row_first if row_count is None else row_count
    out = np.zeros((8, max(rc, 1)), dtype=np.uint32)
    _check(ctx.lib.mh_eval_values(ctx.h, tapes.h, tape, assign.h, row_first, rc, _ptr(out)))
    return out[:, :rc]


def eval_values_many(ctx: Context, tapes: CompiledTapes, ids: Sequence[int], assign: Assignments,
                     row: int = 0) -> np.ndarray:
    """Root values of the tapes `ids` at one row (mh_eval_values_many): u32 [len(ids), 8]."""
    ids_a = np.ascontiguousarray(ids, dtype=np.uint32)
    out = np.zeros((max(len(ids_a), 1), 8), dtype=np.uint32)
    _check(ctx.lib.mh_eval_values_many(ctx.h, tapes.h, _ptr(ids_a), len(ids_a), assign.h, row,
                                       _ptr(out)))
    return out[:len(ids_a)]


# ---- table sets (include/mythril_hip.h mh_tables_*; Op.LOOKUP) ---------------------------------
def _key_limbs(v: int, nw: int) -> List[int]:
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8 * nw)]


def pack_tables(tables: Sequence[Tuple[dict, int, int]]):
    """mh_tables_create's arrays for `tables`, a list of ({key: value}, else value, key bits):
    (counts, nws, key_offsets, keys, value_offsets, values, else_values), the keys of each table
    ascending.  Values and the else value are taken mod 2^256, keys mod 2^(256 nw)."""
    counts, nws, koffs, voffs, keys, vals, elses = [], [], [0], [0], [], [], []
    for tab, else_v, key_bits in tables:
        nw = max(1, (key_bits + 255) // 256)
        mask = (1 << (256 * nw)) - 1
        norm = {int(k) & mask: int(v) for k, v in tab.items()}
        counts.append(len(norm))
        nws.append(nw)
        for k in sorted(norm):
            keys.extend(_key_limbs(k, nw))
            vals.extend(_key_limbs(norm[k] & ((1 << 256) - 1), 1))
        koffs.append(len(keys))
        voffs.append(len(vals))
        elses.extend(_key_limbs(int(else_v) & ((1 << 256) - 1), 1))
    u32 = lambda x: np.ascontiguousarray(x if len(x) else [0], dtype=np.uint32)  # noqa: E731
    return (u32(counts), u32(nws), np.ascontiguousarray(koffs[:-1] or [0], dtype=np.uint64),
            u32(keys), np.ascontiguousarray(voffs[:-1] or [0], dtype=np.uint64), u32(vals),
            u32(elses), len(keys), len(vals))


class Tables:
    """mh_tables: a set of finite maps on the device, read by Op.LOOKUP tapes."""

    def __init__(self, ctx: "Context", tables: Sequence[Tuple[dict, int, int]]):
        self.ctx = ctx
        self.h = None
        counts, nws, koffs, keys, voffs, vals, elses, n_keys, n_vals = pack_tables(tables)
        h = C.c_void_p()
        _check(ctx.lib.mh_tables_create(ctx.h, len(tables), _ptr(counts), _ptr(nws),
                                        _ptr(koffs, C.c_uint64), _ptr(keys), n_keys,
                                        _ptr(voffs, C.c_uint64), _ptr(vals), n_vals,
                                        _ptr(elses), C.byref(h)))
        self.h = h

    def close(self) -> None:
        if self.h:
            self.ctx.lib.mh_tables_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def tables_create(ctx: "Context", tables: Sequence[Tuple[dict, int, int]]) -> Tables:
    return Tables(ctx, tables)


def eval_values_tables(ctx: "Context", tapes: "CompiledTapes", tables: Tables,
                       ids: Sequence[int], assign: "Assignments", row_first: int = 0,
                       row_count: int = 1) -> np.ndarray:
    """Root values of the tapes `ids`, which may hold Op.LOOKUP over `tables`, at rows
    [row_first, row_first + row_count) (mh_eval_values_tables): u32 [len(ids), 8, row_count]."""
    ids_a = np.ascontiguousarray(ids, dtype=np.uint32)
    out = np.zeros((max(len(ids_a), 1), 8, max(row_count, 1)), dtype=np.uint32)
    _check(ctx.lib.mh_eval_values_tables(ctx.h, tapes.h, tables.h, _ptr(ids_a), len(ids_a),
                                         assign.h, row_first, row_count, _ptr(out)))
    return out[:len(ids_a), :, :row_count]


def tables_create_many(ctx: "Context",
                       sets: Sequence[Sequence[Tuple[dict, int, int]]]) -> List[Tables]:
    """One Tables per entry of `sets` (each what tables_create takes), in one device allocation
    and one copy (mh_tables_create_many).  Every handle closes on its own; the device block goes
    with the last.  One invalid set creates none."""
    if not sets:
        return []
    flat = [t for s in sets for t in s]
    counts, nws, koffs, keys, voffs, vals, elses, n_keys, n_vals = pack_tables(flat)
    per_set = np.ascontiguousarray([len(s) for s in sets], dtype=np.uint32)
    hs = (C.c_void_p * len(sets))()
    _check(ctx.lib.mh_tables_create_many(ctx.h, len(sets), _ptr(per_set), _ptr(counts), _ptr(nws),
                                         _ptr(koffs, C.c_uint64), _ptr(keys), n_keys,
                                         _ptr(voffs, C.c_uint64), _ptr(vals), n_vals,
                                         _ptr(elses), hs))
    out = []
    for h in hs:
        tb = Tables.__new__(Tables)
        tb.ctx = ctx
        tb.h = C.c_void_p(h)
        out.append(tb)
    return out


def eval_values_jobs(ctx: "Context", jobs: Sequence[tuple]) -> List[np.ndarray]:
    """Root values of many jobs in one device submission (mh_eval_values_jobs).  A job is
    (tapes, tables or None, ids, assign, row): what eval_values_tables(ctx, tapes, tables, ids,
    assign, row, 1) takes, or eval_values_many when tables is None; jobs may share one `assign`.
    Returns per job u32 [len(ids), 8], equal to the single call's.  Lists beyond VALUES_JOBS_MAX
    jobs go up in chunks."""
    out: List[np.ndarray] = []
    for lo in range(0, len(jobs), VALUES_JOBS_MAX):
        chunk = jobs[lo:lo + VALUES_JOBS_MAX]
        arr = (ValuesJob * len(chunk))()
        keep = []
        for k, (tapes, tables, ids, assign, row) in enumerate(chunk):
            ids_a = np.ascontiguousarray(ids, dtype=np.uint32)
            vals = np.zeros((max(len(ids_a), 1), 8), dtype=np.uint32)
            arr[k] = ValuesJob(tapes.h, tables.h if tables is not None else None,
                               _ptr(ids_a) if len(ids_a) else None, len(ids_a), assign.h, row,
                               _ptr(vals))
            keep.append((ids_a, vals))
        _check(ctx.lib.mh_eval_values_jobs(ctx.h, arr, len(chunk)))
        out.extend(vals[:len(ids_a)] for ids_a, vals in keep)
    return out


# ---- repair of near-miss rows (include/mythril_hip.h mh_conjuncts_* / mh_repair_*) -------------
NO_CONJUNCT = 0xFFFFFFFF
MUTATE_REDRAW = 1
ELITE_DTYPE = np.dtype([("row", "<u4"), ("fail_count", "<u4"), ("pick", "<u4")])  # mh_elite


class ConjunctsInfo(C.Structure):
    """mh_conjuncts_info (include/mythril_hip.h)."""

    _fields_ = [("nodes", _vp), ("tape_off", _u64p), ("leaf", _u32p), ("col_off", _u32p),
                ("cols", _u32p), ("n_conjuncts", C.c_uint32), ("pad", C.c_uint32)]


class ConjunctPlan:
    """mh_conjuncts_build's result, copied out: one tape per kept AND leaf of a root tape
    (``tapes``), each leaf's node id in the root tape (``leaf``) and the columns it reads
    (``cols`` ascending per conjunct; ``col_off`` / ``cols_flat`` as the library lays them out)."""

    def __init__(self, nodes: np.ndarray, group_cols: Sequence[int] = (),
                 max_conjuncts: int = 4096):
        lib = load()
        nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
        gc = np.ascontiguousarray(list(group_cols), dtype=np.uint32)
        h, info = C.c_void_p(), ConjunctsInfo()
        _check(lib.mh_conjuncts_build(nodes.ctypes.data, len(nodes), _ptr(gc), len(gc),
                                      max_conjuncts, C.byref(h), C.byref(info)))
        try:
            n = int(info.n_conjuncts)
            off = np.ctypeslib.as_array(info.tape_off, shape=(n + 1,)).copy()
            flat = np.frombuffer(C.string_at(info.nodes, int(off[-1]) * NODE_DTYPE.itemsize),
                                 dtype=NODE_DTYPE).copy()
            self.n = n
            self.tape_off = off
            self.nodes = flat
            self.tapes = [flat[int(off[i]):int(off[i + 1])] for i in range(n)]
            self.leaf = np.ctypeslib.as_array(info.leaf, shape=(n,)).copy()
            self.col_off = np.ctypeslib.as_array(info.col_off, shape=(n + 1,)).copy()
            nc = int(self.col_off[-1])
            self.cols_flat = np.ctypeslib.as_array(info.cols, shape=(max(nc, 1),)).copy()[:nc]
            self.cols = [self.cols_flat[int(self.col_off[i]):int(self.col_off[i + 1])].tolist()
                         for i in range(n)]
        finally:
            lib.mh_conjuncts_free(h)

    def set_ordinals(self, set_conj: np.ndarray) -> np.ndarray:
        """A guide's set tags (GuideHandle.set_conjuncts: root-tape leaf ids) as ordinals of
        this plan; NO_CONJUNCT for untagged sets and for leaves the plan did not keep."""
        first = {}
        for i, leaf in enumerate(self.leaf.tolist()):
            first.setdefault(leaf, i)
        return np.array([first.get(int(t), NO_CONJUNCT) for t in set_conj], dtype=np.uint32)


DOMAIN_INTERVAL = 0  # MH_DOMAIN_*
DOMAIN_LIST = 1
ROWS_SATURATED = 0xFFFFFFFFFFFFFFFF  # a domain size / row count of 2^64 - 1 reads "at least"


class DomainsDesc(C.Structure):
    """mh_domains_desc (include/mythril_hip.h)."""

    _fields_ = [("cols", _u32p), ("kind", _u32p), ("size", _u64p), ("lo", _u32p),
                ("list_off", _u32p), ("list_vals", _u32p), ("n_cols", C.c_uint32),
                ("pad", C.c_uint32), ("rows", C.c_uint64)]


class Domains:
    """mh_domains: per group column (``cols`` ascending) an interval (``lo``, ``size``) or an
    ascending value list (``lists``), and ``rows``, the product of the sizes (saturating).  Made
    by ``domains_build`` from a group's tape or ``domains_create`` from plain values; the handle
    stays open for the enumerating generator (Assignments.enumerate, query_enumerate) until
    close()."""

    def __init__(self, lib, h: C.c_void_p):
        self.lib, self.h = lib, h
        d = DomainsDesc()
        try:
            _check(lib.mh_domains_info(h, C.byref(d)))
            n = int(d.n_cols)

            def arr(p, k):  # (an empty vector's pointer may be null)
                return np.ctypeslib.as_array(p, shape=(k,)).copy() if k else np.zeros(0, p._type_)

            self.cols = arr(d.cols, n).tolist()
            self.kind = arr(d.kind, n).tolist()
            self.size = arr(d.size, n).tolist()
            self.lo = _ints(arr(d.lo, 8 * n).reshape(n, 8))
            off = arr(d.list_off, n + 1).tolist()
            vals = _ints(arr(d.list_vals, 8 * off[-1]).reshape(-1, 8))
            self.lists = [vals[off[j]:off[j + 1]] for j in range(n)]
            self.rows = int(d.rows)
        except BaseException:
            self.close()
            raise

    def close(self) -> None:
        if self.h:
            self.lib.mh_domains_free(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def domains_build(nodes: np.ndarray, consts: np.ndarray, widths: Sequence[int],
                  group_cols: Sequence[int] = ()) -> Domains:
    """The domains of the columns ``group_cols`` of one group's tape (mh_domains_build; host
    only).  No column: a ground group, whose product is the one empty row."""
    lib = load()
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    consts = np.ascontiguousarray(consts, dtype=np.uint32).reshape(-1, 8)
    w = np.ascontiguousarray(widths, dtype=np.uint16)
    gc = np.ascontiguousarray(list(group_cols), dtype=np.uint32)
    h = C.c_void_p()
    _check(lib.mh_domains_build(nodes.ctypes.data, len(nodes), _ptr(consts), len(consts),
                                _ptr(w, C.c_uint16), len(w), _ptr(gc), len(gc), C.byref(h)))
    return Domains(lib, h)


def domains_create(cols: Sequence[int], kinds: Sequence[int], sizes: Sequence[int],
                   los: Sequence[int], lists: Sequence[Sequence[int]],
                   widths: Sequence[int]) -> Domains:
    """A domain set from plain values (mh_domains_create validates them): per column its kind,
    size, an interval's ``lo`` and a list's values; ``widths`` by query column."""
    lib = load()
    n = len(cols)
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in lists])
    vals = _limb_rows([v for x in lists for v in x] or [0])
    h = C.c_void_p()
    _check(lib.mh_domains_create(
        _ptr(np.ascontiguousarray(cols, dtype=np.uint32)),
        _ptr(np.ascontiguousarray(kinds, dtype=np.uint32)),
        _ptr(np.ascontiguousarray(sizes, dtype=np.uint64), C.c_uint64),
        _ptr(_limb_rows(list(los) or [0])), _ptr(off), _ptr(vals), n,
        _ptr(np.ascontiguousarray(widths, dtype=np.uint16), C.c_uint16), len(widths),
        C.byref(h)))
    return Domains(lib, h)


def query_enumerate(ctx: Context, tapes: CompiledTapes, assign: "Assignments", domains: Domains,
                    global_base: int, count: int, n_cols: int, *, tape: int = 0,
                    mode: int = MODE_FIRST_HIT):
    """One enumeration window (mh_query_enumerate): rows [0, count) of `assign` get the cross
    product's rows global_base.., then tape `tape` runs over them with index_base = global_base.
    Returns (first_hit, hit_count, rows) as query_round does, for the one tape."""
    fh = np.zeros(1, dtype=np.uint64)
    hc = np.zeros(1, dtype=np.uint64)
    rows = np.zeros((1, max(n_cols, 1), 8), dtype=np.uint32)
    _check(ctx.lib.mh_query_enumerate(ctx.h, tapes.h, assign.h, domains.h, global_base, count,
                                      tape, mode, _ptr(fh, C.c_uint64), _ptr(hc, C.c_uint64),
                                      n_cols, _ptr(rows)))
    return fh, hc, rows[:, :n_cols]


class Repair:
    """mh_repair: the mask, score and elite buffers of the repair step, bound to a Context."""

    def __init__(self, ctx: Context, max_conjuncts: int, max_rows: int, max_elites: int):
        self.ctx = ctx
        self.max_conjuncts, self.max_rows, self.max_elites = max_conjuncts, max_rows, max_elites
        h = C.c_void_p()
        _check(ctx.lib.mh_repair_create(ctx.h, max_conjuncts, max_rows, max_elites, C.byref(h)))
        self.h = h

    def close(self) -> None:
        if self.h:
            self.ctx.lib.mh_repair_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def repair_open(ctx: Context, max_conjuncts: int, max_rows: int, max_elites: int) -> Repair:
    return Repair(ctx, max_conjuncts, max_rows, max_elites)


def repair_score(rep: Repair, tapes: CompiledTapes, assign: Assignments, *, tape_first: int = 0,
                 tape_count: Optional[int] = None, row_first: int = 0,
                 row_count: Optional[int] = None, counts: bool = False) -> Optional[np.ndarray]:
    """mh_repair_score: the conjunct tapes over the rows; with counts=True the per-row
    fail_count (u32 [row_count]) is copied out."""
    tc = tapes.n_tapes - tape_first if tape_count is None else tape_count
    rc = assign.capacity - row_first if row_count is None else row_count
    out = np.zeros(max(rc, 1), dtype=np.uint32) if counts else None
    _check(rep.ctx.lib.mh_repair_score(rep.h, tapes.h, tape_first, tc, assign.h, row_first, rc,
                                       _ptr(out) if counts else None))
    return out[:rc] if counts else None


def repair_select(rep: Repair, k: int, seed: int) -> np.ndarray:
    """mh_repair_select: the best min(k, rows) rows as an ELITE_DTYPE array."""
    out = np.zeros(max(k, 1), dtype=ELITE_DTYPE)
    n = C.c_uint32()
    _check(rep.ctx.lib.mh_repair_select(rep.h, k, seed, out.ctypes.data_as(C.c_void_p),
                                        C.byref(n)))
    return out[:n.value]


def repair_mutate(rep: Repair, src: Assignments, dst: Assignments, guide, set_conj, col_off,
                  cols, per: int, *, flags: int = 0, seed: int = 0, global_base: int = 0) -> None:
    """mh_repair_mutate: rows [0, elites * per) of dst from the selected elites' rows of src.
    `guide`: a GuideHandle or guide arrays; set_conj: conjunct ordinal per set of the guide
    (ConjunctPlan.set_ordinals); col_off / cols: ConjunctPlan.col_off / cols_flat."""
    if isinstance(guide, GuideHandle):
        g, keep = guide.guide, None
    else:
        g, keep = _guide_struct(guide)
    sc = np.ascontiguousarray(set_conj, dtype=np.uint32)
    co = np.ascontiguousarray(col_off, dtype=np.uint32)
    cc = np.ascontiguousarray(cols, dtype=np.uint32)
    if len(sc) != int(g.n_sets):
        raise ValueError("set_conj has %d entries for a guide of %d sets" % (len(sc), g.n_sets))
    _check(rep.ctx.lib.mh_repair_mutate(rep.h, src.h, dst.h, C.byref(g), _ptr(sc), _ptr(co),
                                        _ptr(cc), len(co) - 1, per, flags, seed, global_base))
    del keep


def eval_launches(ctx: Context) -> int:
    """Kernel launches mh_eval_values_many has made on `ctx`."""
    v = C.c_uint64()
    _check(ctx.lib.mh_ctx_eval_launches(ctx.h, C.byref(v)))
    return int(v.value)


def limbs_to_ints(arr: np.ndarray) -> Sequence[int]:
    """[8, n] u32 limbs -> Python ints."""
    out = []
    for j in range(arr.shape[1]):
        v = 0
        for k in range(8):
            v |= int(arr[k, j]) << (32 * k)
        out.append(v)
    return out


def microbench_gather(device: int, log2_rows: int, permille: int, layout: int,
                      reps: int = 5) -> Tuple[float, float, int]:
    """mh_microbench_gather: (median ms per launch, useful GB/s, survivors)."""
    ms, gbps, n = C.c_double(), C.c_double(), C.c_uint64()
    _check(load().mh_microbench_gather(device, log2_rows, permille, layout, reps, C.byref(ms),
                                       C.byref(gbps), C.byref(n)))
    return ms.value, gbps.value, int(n.value)
