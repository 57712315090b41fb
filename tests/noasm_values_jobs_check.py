"""mh_eval_values_jobs in the C++ step() build of the interpreter (libmythril_hip_noasm.so), whose
batched table kernels are instantiations of their own: the mixed job list of
tests/values_jobs_cases.py against the single calls of the same library.  Run in its own process
with MYTHRIL_HIP_LIB naming that library (tests/test_gpu_values_jobs.py::test_cpp_step_library):

    MYTHRIL_HIP_LIB=mythril_amd/libmythril_hip_noasm.so python -m tests.noasm_values_jobs_check
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
    from tests import values_jobs_cases as cases

    native.load()
    ctx = native.Context(0)
    h = cases.Handles(ctx, native)
    try:
        jobs, seen = cases.mixed_jobs(h)
        assert len(seen) == 6, seen
        cases.check_jobs(ctx, native, jobs)
    finally:
        h.close()
        ctx.close()
    print("noasm values jobs ok: %d jobs equal their single calls" % len(jobs))
    return 0


if __name__ == "__main__":
    sys.exit(main())
