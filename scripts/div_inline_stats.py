#!/usr/bin/env python3
"""Per-level figures of the inline division paths (jit.cpp op_div, MH_JIT_DIV) for DESIGN §5.1,
from the host wave emulator on config-5 tapes x 128 generated rows: executed VALU / half-rate /
f64 per wave-evaluation and jit_mix's issue cycles, the share of division sites specialised
(counted in the emitted text: a site is a call, an inline site has the live-lane test in front of
it, a folded site has no code), and the share of the inline sites' wave-executions that fell back
to the call: an inline site executes one v_cmp_ne_u32 on the divisor's top limb in the tape body
(nothing else tagged as a division does), the sites still called run as often as at level 0, and
what the executed calls exceed them by are fallbacks (exact while no executed site is folded).

    python scripts/div_inline_stats.py [n_tapes=300]
"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mythril_amd import synth  # noqa: E402
from mythril_amd.tape import TapeSet  # noqa: E402
from oracle import smt_eval  # noqa: E402
from tests.conftest import build_emulator  # noqa: E402
from tests.emu import Emulator, jit_eval, jit_module  # noqa: E402

# the first instruction of each inline path's live-lane test (div_undecided)
P1_TEST = "s_andn2_b64 s[88:89], s[30:31], vcc"
P3_TEST = "s_andn2_b64 s[88:89], s[30:31], s[86:87]"


def counters(emu, name, n):
    f = getattr(emu.lib, name)
    f.restype = None
    f.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    buf = (C.c_uint64 * n)()
    f(buf, 1)
    return list(buf)


def machine_op(name):
    """Value of `name` in jit.h's enum Op."""
    src = open(os.path.join(ROOT, "mythril_amd", "csrc", "jit.h")).read()
    body = src[src.index("enum Op"):]
    body = re.sub(r"//[^\n]*|/\*.*?\*/", "", body[body.index("{") + 1:body.index("};")])
    return [e.strip() for e in body.split(",") if e.strip()].index(name)


def dop_range():
    """[D_UDIV_R, D_SMOD_C] of dev_isa.h's enum mh_dop."""
    src = open(os.path.join(ROOT, "mythril_amd", "csrc", "dev_isa.h")).read()
    body = src[src.index("enum mh_dop"):]
    body = re.sub(r"//[^\n]*", "", body[body.index("{") + 1:body.index("};")])
    names, nxt = {}, 0
    for ent in [e.strip() for e in body.split(",") if e.strip()]:
        if "=" in ent:
            nm, val = [x.strip() for x in ent.split("=")]
            nxt = int(val, 0) if val[0].isdigit() else names[val]
        else:
            nm = ent
        names[nm] = nxt
        nxt += 1
    return names["D_UDIV_R"], names["D_SMOD_C"]


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
    out = {}
    for level in ("0", "1", "2", "3"):
        os.environ["MH_JIT_DIV"] = level
        tot = dict(valu=0, wide=0, f64=0)
        m = 0
        counters(emu, "emu_jit_div_hist", 32)
        counters(emu, "emu_jit_tag_op", 256 * 128)
        for i in range(n):
            res = jit_eval(emu, ts, i, soa)
            if not res.ok:
                continue
            m += 1
            for k in tot:
                tot[k] += res.dyn[k]
        calls = sum(counters(emu, "emu_jit_div_hist", 32))
        tag_op = counters(emu, "emu_jit_tag_op", 256 * 128)
        lo, hi = dop_range()
        cmp_ne = machine_op("M_V_CMP_NE")
        inline_execs = sum(tag_op[128 * t + cmp_ne] for t in range(lo, hi + 1))
        per = {k: v / m for k, v in tot.items()}
        cyc = (2.56 * (per["valu"] - per["wide"]) + 4.5 * (per["wide"] - per["f64"]) +
               6.1 * per["f64"])  # tests/tools/jit_mix.py's weights
        # static: the sites in the text of every tape (one module per tape keeps the bodies apart
        # from the shared subroutine, which is printed once per module after them)
        sites = dict(call=0, p1=0, p3=0)
        for i in range(n):
            one = TapeSet(ts.var_names)
            one.pool = ts.pool
            one.tapes = [ts.tapes[i]]
            text, _, nj = jit_module(emu, one, assemble=False)
            if not nj:
                continue
            sites["call"] += len(re.findall(r"s_swappc_b64", text))
            sites["p1"] += text.count(P1_TEST)
            sites["p3"] += text.count(P3_TEST)
        out[level] = dict(tapes=m, per_wave_eval=per, issue_cycles=cyc, calls_executed=calls,
                          inline_site_executions=inline_execs, sites=sites)
    base = out["0"]
    for level, o in out.items():
        s = o["sites"]
        s["folded"] = base["sites"]["call"] - s["call"]
        s["specialised_share"] = (s["p1"] + s["p3"] + s["folded"]) / max(base["sites"]["call"], 1)
        called = base["calls_executed"] - o["inline_site_executions"]
        o["fallbacks"] = o["calls_executed"] - called
        o["fallback_share"] = o["fallbacks"] / max(o["inline_site_executions"], 1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
