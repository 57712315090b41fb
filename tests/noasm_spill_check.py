"""The C++ step() build of the interpreter (libmythril_hip_noasm.so: every op through exec.h) on
spilled tapes: D_SPILL / D_FILL run through step()'s spill / fill hooks of the device machine
instead of the assembly driver.  Run in its own process with MYTHRIL_HIP_LIB naming that library
(tests/test_gpu_spill.py::test_cpp_step_library):

    MYTHRIL_HIP_LIB=mythril_amd/libmythril_hip_noasm.so python -m tests.noasm_spill_check
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
    from tests import spill_cases as sc
    from tests.test_gpu_spill import _want, check_counts

    native.load()
    ctx = native.Context(0)
    try:
        for n_cols in (4, 6):  # pinned columns; every column a D_LOADVAR
            check_counts(ctx, sc.mixed_set(n_cols), 209, 37, _want(n_cols))
    finally:
        ctx.close()
    print("noasm spill ok: 19 + 19 tapes x 209 rows equal the C oracle")
    return 0


if __name__ == "__main__":
    sys.exit(main())
