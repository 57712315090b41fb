"""mh_query_round_hits_many in the C++ step() build of the interpreter (libmythril_hip_noasm.so):
the batch compiled with MH_ASM_CORE=0 against that library's own mh_query_round_hits, job by job
(tests/round_hits_cases.py).  Run in its own process with MYTHRIL_HIP_LIB naming that library
(tests/test_gpu_round_hits_many.py::test_cpp_step_library):

    MYTHRIL_HIP_LIB=mythril_amd/libmythril_hip_noasm.so python -m tests.noasm_round_hits_many_check
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
    from tests import round_hits_cases

    native.load()
    ctx = native.Context(0)
    try:
        line = round_hits_cases.check(ctx)
    finally:
        ctx.close()
    print("noasm " + line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
