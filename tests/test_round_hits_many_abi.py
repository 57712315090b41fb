"""mh_query_round_hits_many without a device: the refusals that read no handle come before any
handle is read or any device call is made (FAKE stands in for every handle, as in
tests/test_hits_abi.py), each with its code and a message that names the job and the constant."""
import ctypes as C
import os
import re

import pytest

from mythril_amd import native

FAKE = C.c_void_p(1)  # not a handle: every call below must fail on its arguments first
WHO = b"mh_query_round_hits_many: "


def _jobs(n, over=None):
    """n jobs over FAKE handles; `over` = {job index: {field: value}}."""
    over = over or {}
    arr = (native.RoundHitsJob * n)()
    keep = []
    g = native.Guide()
    for i in range(n):
        hits = (C.c_uint64 * 64)()
        nh = (C.c_uint32 * 1)()
        keep.append((hits, nh))
        arr[i] = native.RoundHitsJob(FAKE, FAKE, C.pointer(g), 1, 0, 64, 0, 1, 4, 0, None,
                                     hits, nh, None, None)
        for k, v in over.get(i, {}).items():
            setattr(arr[i], k, v)
    return arr, (keep, g)


def test_null_ctx_and_null_list():
    lib = native.load()
    arr, _keep = _jobs(1)
    assert lib.mh_query_round_hits_many(None, arr, 1) == native.MH_E_INVALID
    assert lib.mh_last_error().startswith(WHO) and b"null ctx" in lib.mh_last_error()
    assert lib.mh_query_round_hits_many(FAKE, None, 1) == native.MH_E_INVALID
    assert lib.mh_last_error().startswith(WHO) and b"null job list" in lib.mh_last_error()


def test_job_count_limits():
    lib = native.load()
    assert lib.mh_query_round_hits_many(FAKE, None, 0) == native.MH_OK  # nothing to do
    arr, _keep = _jobs(257)
    assert lib.mh_query_round_hits_many(FAKE, arr, 257) == native.MH_E_INVALID
    msg = lib.mh_last_error()
    assert msg.startswith(WHO) and b"257 jobs" in msg and b"MH_ROUND_MANY_MAX" in msg


@pytest.mark.parametrize("k", [0, 65])
def test_k_outside_its_range_names_the_job(k):
    lib = native.load()
    arr, _keep = _jobs(3, {2: {"k": k}})
    assert lib.mh_query_round_hits_many(FAKE, arr, 3) == native.MH_E_INVALID
    msg = lib.mh_last_error()
    assert msg.startswith(WHO + b"job 2: ") and b"k = %d" % k in msg and b"MH_HITS_MAX" in msg


def test_no_rows_names_the_job():
    lib = native.load()
    arr, _keep = _jobs(2, {1: {"count": 0}})
    assert lib.mh_query_round_hits_many(FAKE, arr, 2) == native.MH_E_INVALID
    msg = lib.mh_last_error()
    assert msg.startswith(WHO + b"job 1: ") and b"count = 0" in msg and b"MH_HITS_MAX_ROWS" in msg


def test_the_first_bad_job_is_named_before_any_handle_is_read():
    """Job 0 is fine but for its handles, job 1 has a bad k: the k of every job is checked first."""
    lib = native.load()
    arr, _keep = _jobs(2, {1: {"k": 0}})
    assert lib.mh_query_round_hits_many(FAKE, arr, 2) == native.MH_E_INVALID
    assert lib.mh_last_error().startswith(WHO + b"job 1: k = 0")


def test_struct_and_constants_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                             "include", "mythril_hip.h")).read()
    m = re.search(r"#define MH_ROUND_HITS_MANY_MAX_BYTES \((\d+)u << (\d+)\)", text)
    assert int(m.group(1)) << int(m.group(2)) == native.ROUND_HITS_MANY_MAX_BYTES
    body = re.search(r"typedef struct mh_round_hits_job \{(.*?)\} mh_round_hits_job;", text,
                     re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [n.rstrip("_") for n, _ in native.RoundHitsJob._fields_]
    assert C.sizeof(native.RoundHitsJob) == 3 * 8 + 3 * 8 + 4 * 4 + 5 * 8
