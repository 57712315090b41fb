"""The planner of a batched values submission (csrc/values_plan.h, mh_eval_values_jobs's host
half) under AddressSanitizer + UBSan: tests/native/values_plan_check.cpp, a stand-alone program,
checks that every job's listed positions appear exactly once, in the launch of their variant, that
a segment's ids ascend, that the block table covers every segment's slices exactly, and the 0-job,
1-job and 256-job submissions.  Host only: the header makes no HIP call."""
import os

from tests.test_host_sanitized import NATIVE, needs_gxx, replay, sanitized_build


@needs_gxx
def test_values_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "values_plan_check")
    sanitized_build([os.path.join(NATIVE, "values_plan_check.cpp")], exe)
    stats = replay(exe, "-")
    assert int(stats["cases"]) >= 15
