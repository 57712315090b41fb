#!/usr/bin/env python3
"""Golden interpreter code of the LASER-shaped queries (tests/golden/interp_words.json).

For every query of tests/laser_like.py (queries() and hard_queries()) this records what the tape
compiler emits for the interpreter, through the test-only host emulator (no GPU):

* ``whole``: the query as one tape, through the retry ladder of Sieve.compile (the tape as
  lowered, then rematerialised at 8, 32, 256 nodes) up to the first size that compiles: per size
  either ``null`` (refused for register pressure) or the sha256 of ``emu.words`` and ``n_regs``;
* ``buckets``: the tape set the sieve builds (one tape per variable-disjoint bucket): the sha256
  of the set's words and every tape's ``n_regs``, or ``null`` when a tape is refused.

tests/test_spill_host.py recomputes the records and requires every tape that compiled when the
file was written to compile to the same words: a change to the allocator that only adds
capability (register spilling) leaves them alone.  Run it again, and commit the result, only with
a change that is meant to alter the interpreter's code.

    python scripts/interp_golden.py [--check]
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "interp_words.json")
SIZES = (0, 8, 32, 256)


def _sha(words) -> str:
    return hashlib.sha256(np.ascontiguousarray(words, dtype=np.uint32).tobytes()).hexdigest()


def _n_regs(emu, ts):
    row = np.zeros((max(ts.n_vars, 1), 8, 1), dtype=np.uint32)
    return [int(emu.eval(ts, t, row)[1]) for t in range(len(ts.tapes))]


def records(emu):
    """The records, computed on a thread of their own: the tape compiler starts with the attempt
    (rematerialisation size, held columns, order) that fitted the last tape compiled on its
    thread, so the code of a tape depends on what the thread compiled before; a new thread
    starts, like a new process, with the first attempt."""
    import threading

    box = {}

    def work():
        try:
            box["out"] = _records(emu)
        except BaseException as e:  # noqa: BLE001 - handed to the caller's thread
            box["err"] = e

    th = threading.Thread(target=work)
    th.start()
    th.join()
    if "err" in box:
        raise box["err"]
    return box["out"]


def _records(emu):
    from mythril_amd.lower import lower_query
    from mythril_amd.sieve import local_tape, rematerialize
    from mythril_amd.tape import Tape, TapeSet
    from tests import laser_like
    from tests.emu import EmuError

    out = {}
    for which in ("queries", "hard_queries"):
        n = len(getattr(laser_like, which)()[1])
        for qi in range(n):
            ctx, qs = getattr(laser_like, which)()
            name, cs = qs[qi]
            root, schema = lower_query(ctx.b, [c.node for c in cs])
            cols = list(schema.columns)
            nodes = local_tape(ctx.b, root, cols)
            ts = TapeSet(cols)
            ts.pool = ctx.b.pool
            whole = []
            for size in SIZES:
                ts.tapes[:] = [Tape(nodes if size == 0 else rematerialize(nodes, size))]
                try:
                    whole.append({"size": size, "sha": _sha(emu.words(ts)),
                                  "n_regs": _n_regs(emu, ts)})
                    break
                except EmuError as e:
                    if "register pressure" not in str(e):
                        raise
                    whole.append(None)
            bts, _, _ = laser_like.query_tapeset(ctx.b, cs)
            try:
                buckets = {"sha": _sha(emu.words(bts)), "n_regs": _n_regs(emu, bts)}
            except EmuError as e:
                if "register pressure" not in str(e):
                    raise
                buckets = None
            out["%s/%s" % (which, name)] = {"whole": whole, "buckets": buckets}
    return out


def main():
    from tests.conftest import build_emulator
    from tests.emu import Emulator

    got = records(Emulator(build_emulator()))
    if "--check" in sys.argv[1:]:
        with open(GOLDEN) as f:
            want = json.load(f)
        bad = [k for k in want if want[k] != got.get(k)]
        print("differs: %s" % bad if bad else "identical (%d queries)" % len(want))
        return 1 if bad else 0
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d queries)" % (GOLDEN, len(got)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
