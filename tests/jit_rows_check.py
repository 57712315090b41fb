"""The native kernel with several 64-row chunks per wave, against the C oracle.  Run in a process of
its own with MH_JIT_ROWS_PER_WG set (the library reads it once per process;
tests/test_gpu_run_partition.py::test_jit_chunk_loop_forced starts it):

    MH_JIT_ROWS_PER_WG=512 python -m tests.jit_rows_check

By default a workgroup of the native kernel takes 256 rows, one chunk per wave, until a run exceeds
2^19 rows, so the chunk loop of jit.cpp build_module only ever saw whole chunks.  With 512 or 1024
rows per workgroup the windows below end in a partial last chunk (3+511, 5+513, 37+700), in a
wave whose range is clipped to nothing or workgroups whose later waves start beyond the end (0+1,
9+1089, 7+4097), and at a whole workgroup (0+512).  Counts and first hits of the nv3 and nv6 sets
of tests/partition_cases.py, both modes, every window and the whole buffer.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    rows_per_wg = int(os.environ.get("MH_JIT_ROWS_PER_WG", "0"))
    assert rows_per_wg >= 512 and rows_per_wg % 256 == 0, rows_per_wg
    import numpy as np

    from mythril_amd import native
    from tests import partition_cases as pc

    native.load()
    ctx = native.Context(0)
    checked = 0
    for name in ("nv3", "nv6"):
        ts = pc.tape_set(name)
        ct = ctx.compile(ts)
        a = ctx.assignments(ts.n_vars, pc.N)
        info = ct.jit()
        jitted = ct.jitted()
        planted = pc.planted(name) + pc.planted_conjunctions(name)
        assert all(jitted[t] for t in planted), ("planted tapes not jitted", jitted)
        a.generate(pc.SEED, pc.BASE)
        for first, count in pc.JIT_WINDOWS + [(0, pc.N)]:
            cnt, hit = pc.oracle(name, first, count)
            for mode in (native.MODE_COUNT_ALL, native.MODE_FIRST_HIT):
                fh, hc = native.run(ctx, ct, a, row_first=first, row_count=count,
                                    index_base=pc.BASE, mode=mode)
                where = (name, first, count, mode)
                bad = [(t, int(fh[t]), int(hit[t])) for t in range(len(hit)) if fh[t] != hit[t]]
                assert np.array_equal(fh, hit), (where, "first_hit (tape, got, want)", bad)
                if mode == native.MODE_COUNT_ALL:
                    bad = [(t, int(hc[t]), int(cnt[t])) for t in range(len(cnt)) if hc[t] != cnt[t]]
                    assert np.array_equal(hc, cnt), (where, "hit_count (tape, got, want)", bad)
                checked += 1
        print("%s: %d of %d tapes jitted, %d with hits in the buffer"
              % (name, info["n_jitted"], len(ts.tapes), int(np.count_nonzero(cnt))))
        a.close()
        ct.close()
    ctx.close()
    print("jit rows ok: %d rows per workgroup, %d runs equal the oracle" % (rows_per_wg, checked))
    return 0


if __name__ == "__main__":
    sys.exit(main())
