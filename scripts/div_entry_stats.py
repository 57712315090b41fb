#!/usr/bin/env python3
"""Figures of the division subroutine's level-6 entries (jit.cpp op_div / div_routine,
MH_JIT_STAGE=6: the raw srem entry and the run-time width dispatch) for DESIGN §5.1, from the
host wave emulator on config-5 tapes x 128 generated rows.

Per build -- level 5, level 6, and level 6 with one layer at a time (MH_JIT_ENTRY=1 the raw srem
entry, 2 the width dispatch): executed VALU / half-rate / f64 per wave-evaluation, the VALU inside
the subroutine and at the division sites (the SSA division ops' own code), jit_mix's issue
cycles, executed calls, calls by tail (L_SREM / L_SDIV), entries of the new labels (L_SRAW the raw
entry, L_SCOLD its fallback into the legacy code, L_BGO<k> the dispatch into variant ny = k + 1,
L_BNO a wave the dispatch looked at and left to the legacy code) and the legacy entries.

    python scripts/div_entry_stats.py [n_tapes=300]
"""
import collections
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mythril_amd import synth  # noqa: E402
from oracle import smt_eval  # noqa: E402
from tests.conftest import build_emulator  # noqa: E402
from tests.emu import Emulator, jit_eval  # noqa: E402

LABELS = {1: "L_UNS", 3: "L_TOP3", 4: "L_CONV", 41: "L_SDIV", 42: "L_SREM", 43: "L_SMOD",
          50: "L_NARROW", 102: "L_YSLOW", 110: "L_F32", 111: "L_F32OK", 113: "L_SRAW",
          114: "L_SCOLD", 115: "L_BNO"}
LABELS.update({10 + j: "L_STEP%d" % j for j in range(8)})
LABELS.update({116 + k: "L_BGO%d" % k for k in range(1, 7)})
# (name, MH_JIT_STAGE, MH_JIT_ENTRY)
BUILDS = (("level5", "5", None), ("level6", "6", None), ("level6_raw_srem_only", "6", "1"),
          ("level6_width_dispatch_only", "6", "2"))


def counters(emu, name, n):
    f = getattr(emu.lib, name)
    f.restype = None
    f.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    buf = (C.c_uint64 * n)()
    f(buf, 1)
    return list(buf)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    emu = Emulator(build_emulator())
    ts = synth.generate(n)
    seed = synth.load_spec()["assignment_seed"]
    rows = 128
    soa = np.zeros((ts.n_vars, 8, rows), dtype=np.uint32)
    for r in range(rows):
        a = smt_eval.gen_assignment(seed, ts.n_vars, r)
        for v in range(ts.n_vars):
            for k in range(8):
                soa[v, k, r] = (a[v] >> (32 * k)) & 0xFFFFFFFF
    os.environ.pop("MH_JIT_DIV", None)
    out = dict(tapes=n, rows=rows, builds={})
    values = {}
    for name, stage, entry in BUILDS:
        os.environ["MH_JIT_STAGE"] = stage
        if entry is None:
            os.environ.pop("MH_JIT_ENTRY", None)
        else:
            os.environ["MH_JIT_ENTRY"] = entry
        tot = dict(valu=0, wide=0, f64=0, div_valu=0)
        m = 0
        counters(emu, "emu_jit_div_hist", 32)
        counters(emu, "emu_jit_div_labels", 128)
        counters(emu, "emu_jit_tag_valu", 512)
        labels = collections.Counter()
        vals = []
        for i in range(n):
            res = jit_eval(emu, ts, i, soa)
            lab = counters(emu, "emu_jit_div_labels", 128)
            calls_i = sum(counters(emu, "emu_jit_div_hist", 32))
            vals.append(res.values if res.ok else None)
            if not res.ok:
                continue
            m += 1
            for k in tot:
                tot[k] += res.dyn[k]
            for k, v in enumerate(lab):
                if v and k in LABELS:
                    labels[LABELS[k]] += v
            labels["calls"] += calls_i
        values[name] = vals
        tags = counters(emu, "emu_jit_tag_valu", 512)
        chunks = m * ((rows + 63) // 64)
        # the tape-body VALU of the ops that called the subroutine: their tags are the ones with
        # VALU counted inside it
        site = sum(tags[t] for t in range(255) if tags[256 + t])
        per = {k: v / m for k, v in tot.items()}
        per["div_site_valu"] = site / chunks
        cyc = (2.56 * (per["valu"] - per["wide"]) + 4.5 * (per["wide"] - per["f64"]) +
               6.1 * per["f64"])  # tests/tools/jit_mix.py's weights
        ex = dict(labels)
        out["builds"][name] = dict(
            tapes=m, per_wave_eval=per, issue_cycles=cyc, executed=ex,
            calls_per_1000_chunks=1000.0 * labels["calls"] / chunks,
            raw_srem_entries=labels["L_SRAW"], raw_srem_fallbacks=labels["L_SCOLD"],
            dispatch_entries=sum(labels["L_BGO%d" % k] for k in range(1, 7)),
            dispatch_left_to_legacy=labels["L_BNO"])
    base = out["builds"]["level5"]["per_wave_eval"]
    out["saved_valu_per_wave_eval"] = {
        name: base["valu"] - b["per_wave_eval"]["valu"] for name, b in out["builds"].items()}
    out["values_identical"] = all(v == values["level5"] for v in values.values())
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
