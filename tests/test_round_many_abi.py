"""mh_query_round_many's refusals that need no device: the list is validated before any device
call, so a GPU-less host reaches these checks (a fake ctx handle, never dereferenced past them,
stands in as in tests/test_native_abi.py).  The refusals that need real tape sets and buffers are
in tests/test_gpu_round_many.py; tests/test_native_abi.py checks the export itself in the header,
both libraries and the binding."""
import ctypes as C

from mythril_amd import native


def _err(lib) -> str:
    return lib.mh_last_error().decode()


def test_null_ctx_and_empty_list():
    lib = native.load()
    assert lib.mh_query_round_many(None, None, 0) == native.MH_E_INVALID
    assert "null ctx" in _err(lib)
    fake = C.c_void_p(1)  # not a ctx: every call below must return on its arguments first
    assert lib.mh_query_round_many(fake, None, 0) == native.MH_OK
    arr = (native.RoundJob * 1)()
    assert lib.mh_query_round_many(fake, arr, 0) == native.MH_OK


def test_job_limit_and_null_list():
    lib = native.load()
    fake = C.c_void_p(1)
    n = native.ROUND_MANY_MAX + 1
    arr = (native.RoundJob * n)()
    assert lib.mh_query_round_many(fake, arr, n) == native.MH_E_INVALID
    assert "MH_ROUND_MANY_MAX (256)" in _err(lib) and "257 jobs" in _err(lib)
    assert lib.mh_query_round_many(fake, None, 3) == native.MH_E_INVALID
    assert "null job list" in _err(lib)


def test_null_handles_name_the_job():
    lib = native.load()
    fake = C.c_void_p(1)
    for n in (1, 5, native.ROUND_MANY_MAX):
        arr = (native.RoundJob * n)()  # zeroed: every handle null
        assert lib.mh_query_round_many(fake, arr, n) == native.MH_E_INVALID
        assert "job 0: null handle" in _err(lib)


def test_wrapper_signature_and_struct_layout():
    """The binding's struct is the header's mh_round_job: 3 pointers, 3 u64, 4 u32, 3 pointers."""
    assert C.sizeof(native.RoundJob) == 3 * 8 + 3 * 8 + 4 * 4 + 3 * 8
    assert native.RoundJob.count.offset == 40 and native.RoundJob.first_hit.offset == 64
    assert native.SIGNATURES["mh_query_round_many"][1][2] is C.c_uint32
    assert native.query_round_many(None, []) == []
