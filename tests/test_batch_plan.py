"""The planner of a batched query round (csrc/batch_plan.h, mh_query_round_many's host half) under
AddressSanitizer + UBSan: tests/native/batch_plan_check.cpp, a stand-alone program, checks that
the block tables cover every (job, row block, tape slice) exactly once for counts 1 / 63 / 64 / 65
/ 4096 and tape lists of 1 / 64 / 65 / 130, that jobs are grouped by register class and generator
form, and the 0-job and 256-job batches.  Host only: the header makes no HIP call."""
import os

from tests.test_host_sanitized import NATIVE, needs_gxx, replay, sanitized_build


@needs_gxx
def test_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "batch_plan_check")
    sanitized_build([os.path.join(NATIVE, "batch_plan_check.cpp")], exe)
    stats = replay(exe, "-")
    assert int(stats["cases"]) >= 25
