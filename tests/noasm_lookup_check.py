"""D_LOOKUP in the C++ step() build of the interpreter (libmythril_hip_noasm.so: every op through
exec.h), against the Python restatement.  Run in its own process with MYTHRIL_HIP_LIB naming that
library (tests/test_gpu_lookup.py::test_cpp_step_library):

    MYTHRIL_HIP_LIB=mythril_amd/libmythril_hip_noasm.so python -m tests.noasm_lookup_check
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    lib_path = os.environ.get("MYTHRIL_HIP_LIB", "")
    assert lib_path.endswith("libmythril_hip_noasm.so"), lib_path
    from mythril_amd import native
    from oracle import smt_eval
    from tests import fake_tables, lookup_cases

    native.load()
    ctx = native.Context(0)
    try:
        n = lookup_cases.check_shapes(ctx, native, sizes=(0, 1, 3, 65), widths=(8, 256))
        # the lookup among live registers (NR 15) and mixed with keccak and a division
        rng = lookup_cases.case_rng(81)
        table, els = lookup_cases.make_table(rng, 65, 2, 160)
        keys = lookup_cases.probes(rng, table, 2, 65)
        ts = lookup_cases.lookup_tapeset(2, 160, live=10)
        tabs = [(table, els, 512)]
        got, _ = lookup_cases.device_values(ctx, ts, [2], tabs, lookup_cases.key_soa(keys, 2),
                                            native)
        extra = fake_tables.lookup_extra(tabs)
        assert got[0] == [int(smt_eval.evaluate(ts.tapes[2].nodes, ts.pool.values,
                                                [k & ((1 << 256) - 1), k >> 256], extra=extra))
                          for k in keys]
        table, els = lookup_cases.make_table(rng, 64, 1, 256)
        keys = lookup_cases.probes(rng, table, 1, 65)
        ts = lookup_cases.mixed_tapeset()
        tabs = [(table, els, 256)]
        got, _ = lookup_cases.device_values(ctx, ts, [0, 1], tabs, lookup_cases.key_soa(keys, 1),
                                            native)
        extra = fake_tables.lookup_extra(tabs)
        for i in range(2):
            assert got[i] == [int(smt_eval.evaluate(ts.tapes[i].nodes, ts.pool.values, [k],
                                                    extra=extra)) for k in keys], i
    finally:
        ctx.close()
    print("noasm lookup ok: %d lookups equal the restatement" % n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
