#!/usr/bin/env python3
"""Figures of the division subroutine's width-specialised variants (jit.cpp op_div / div_routine,
MH_JIT_STAGE=5) for DESIGN §5.1, from the host wave emulator on config-5 tapes x 128 generated
rows.

The prize first, from the emitter's own widths: the sites that qualify by (ny, nx, const), read
back from the S_DIV_KIND immediates of the level-5 text (kind | (64 const + 8 ny + j0) << 3,
nx = ny + j0), and what the subroutine's labels say the calls execute at level 4.  Then, per
MH_JIT_STAGE 4 and 5: executed VALU / half-rate / f64 per wave-evaluation and jit_mix's issue
cycles, executed calls and legacy entries (label L_UNS), the variants' fallbacks -- exact on the
tapes all of whose sites are variant sites, where every L_UNS entry is one -- and the code object's
bytes and groups.

    python scripts/div_width_stats.py [n_tapes=300]
"""
import collections
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

LABELS = {1: "L_UNS", 3: "L_TOP3", 50: "L_NARROW", 100: "L_RLT", 102: "L_YSLOW", 110: "L_F32",
          111: "L_F32OK"}
LABELS.update({10 + j: "L_STEP%d" % j for j in range(8)})
KIND = re.compile(r"s_mov_b32 s80, (\S+)")


def counters(emu, name, n):
    f = getattr(emu.lib, name)
    f.restype = None
    f.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    buf = (C.c_uint64 * n)()
    f(buf, 1)
    return list(buf)


def sites_of(text):
    """[(kind, const, ny, nx) or (kind,)] of the division sites in a one-tape module's text."""
    body = text[:text.index("mh_div:")] if "mh_div:" in text else text
    out = []
    for m in KIND.finditer(body):
        v = int(m.group(1), 0)
        e = v >> 3
        out.append((v & 7, e >> 6, (e >> 3) & 7, ((e >> 3) & 7) + (e & 7)) if e else (v,))
    return out


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
    # static: every tape's sites at level 5
    os.environ["MH_JIT_STAGE"] = "5"
    shapes = collections.Counter()
    pure = set()
    n_sites = 0
    for i in range(n):
        one = TapeSet(ts.var_names)
        one.pool = ts.pool
        one.tapes = [ts.tapes[i]]
        text, _, nj = jit_module(emu, one, assemble=False)
        if not nj:
            continue
        st = sites_of(text)
        n_sites += len(st)
        for s in st:
            if len(s) == 4:
                shapes["ny=%d nx=%d %s" % (s[2], s[3], "const" if s[1] else "var")] += 1
        if st and all(len(s) == 4 for s in st):
            pure.add(i)
    out = dict(called_sites=n_sites, variant_sites=sum(shapes.values()),
               variant_sites_by_shape=dict(sorted(shapes.items())), levels={})
    for level in ("4", "5"):
        os.environ["MH_JIT_STAGE"] = level
        tot = dict(valu=0, wide=0, f64=0, div_valu=0)
        m = 0
        counters(emu, "emu_jit_div_hist", 32)
        counters(emu, "emu_jit_div_labels", 128)
        labels = collections.Counter()
        pure_uns = pure_calls = 0
        for i in range(n):
            res = jit_eval(emu, ts, i, soa)
            lab = counters(emu, "emu_jit_div_labels", 128)
            calls_i = sum(counters(emu, "emu_jit_div_hist", 32))
            if not res.ok:
                continue
            m += 1
            for k in tot:
                tot[k] += res.dyn[k]
            for k, v in enumerate(lab):
                if v and k in LABELS:
                    labels[LABELS[k]] += v
            labels["calls"] += calls_i
            if i in pure:
                pure_uns += lab[1]
                pure_calls += calls_i
        per = {k: v / m for k, v in tot.items()}
        cyc = (2.56 * (per["valu"] - per["wide"]) + 4.5 * (per["wide"] - per["f64"]) +
               6.1 * per["f64"])  # tests/tools/jit_mix.py's weights
        text, hsaco, _ = jit_module(emu, ts, assemble=True)
        out["levels"][level] = dict(
            tapes=m, per_wave_eval=per, issue_cycles=cyc, executed=dict(labels),
            variant_entries=labels["calls"] - labels["L_UNS"] if level == "5" else 0,
            pure_variant_tapes=dict(tapes=len(pure), calls=pure_calls, fallbacks=pure_uns,
                                    fallback_share=pure_uns / max(pure_calls, 1)),
            code_object_bytes=hsaco, groups=len(re.findall(r"^mh_g\d+:", text, re.M)))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
