"""The bucketed id list and the planner of the interpreter's direct launches (csrc/launch_plan.h:
the host half of mh_run_async, mh_repair_score and the values entry points) under AddressSanitizer
+ UBSan: tests/native/launch_plan_check.cpp, a stand-alone program, checks that every id of a tape
range is in exactly one launch, that launches are contiguous runs of the id list inside one
register class, the merged and the unmerged variants, the spilling launches' regions and the
capacity verdict, for empty / one-id / bucket-aligned / whole ranges, merge and masks on and off,
1 / 64 / 65 / 4096 / 4097 rows and a stride below and at 2^30.  Host only: the header makes no HIP
call."""
import os

from tests.test_host_sanitized import NATIVE, needs_gxx, replay, sanitized_build


@needs_gxx
def test_launch_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "launch_plan_check")
    sanitized_build([os.path.join(NATIVE, "launch_plan_check.cpp")], exe)
    stats = replay(exe, "-")
    assert int(stats["cases"]) >= 5000
