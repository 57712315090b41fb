"""Interpreter register spilling on the host (compile.cpp's allow_spill allocation, dev_isa.h
D_SPILL / D_FILL), through the test-only emulator that compiles with spilling
(tests/native/spill_emu.cpp: the product tape compiler and exec.h's step()), against the Python
oracle.

* fan tapes (tests/spill_cases.py) that need more than 15 registers compile with spill slots and
  evaluate to the oracle's values; fans that fit compile without a spill op;
* a word-level checker of the emitted code: every fill reads a slot an earlier spill wrote, slot
  numbers stay below the reported count, no spill op in a window's last slot;
* 210 random DAG tapes over every op class, most of which spill;
* the LASER-shaped queries compile to the words recorded before the allocator learned to spill
  (tests/golden/interp_words.json, scripts/interp_golden.py).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from mythril_amd.tape import NODE_DTYPE
from oracle import smt_eval as E
from tests import spill_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


OPS, WINDOW, spill_ops = sc.OPS, sc.WINDOW, sc.spill_ops


def check_spill_words(words, n_slots: int):
    """The word-level rules of a spilled tape; returns (spills, fills)."""
    written = set()
    n_spill = n_fill = 0
    for s, name, slot, w0 in spill_ops(words):
        assert slot < n_slots, (s, name, slot, n_slots)
        assert s % WINDOW != WINDOW - 1, "spill op in a window's last slot (%d)" % s
        if name == "D_SPILL":
            assert (w0 & 0xFF) < 15, "a spill reads a register, never X"
            written.add(slot)
            n_spill += 1
        else:
            assert slot in written, "D_FILL of slot %d at %d before any D_SPILL wrote it" % (slot, s)
            assert (w0 & 0xFF) == 15 and ((w0 >> 16) & 0xFF) <= 15
            n_fill += 1
    return n_spill, n_fill


@pytest.fixture(scope="module")
def semu():
    """The emulator that compiles with spilling, as the library does (tests/native/spill_emu.cpp);
    the suite's `emu` compiles without, as every caller without the spill hooks."""
    return sc.SpillEmulator()


def _oracle(ts, rows):
    return [int(E.evaluate(ts.tapes[0].nodes, ts.pool.values, r)) for r in rows]


@pytest.mark.parametrize("chain", [1, 10])
@pytest.mark.parametrize("k", [13, 16, 24, 40])
def test_fan_spills_and_matches_oracle(semu, k, chain):
    ts = sc.fan(k, chain)
    n_slots = int(semu.spills(ts)[0])
    assert n_slots > 0
    # each value beyond the twelve that fit waits in a slot of its own until its term of the sum
    assert n_slots == k - 12
    rows = sc.edge_rows(2, 96, 1000 * k + chain)
    got, n_regs = semu.eval(ts, 0, sc.soa(rows, 2))
    assert n_regs == 15
    assert got == _oracle(ts, rows)
    n_spill, n_fill = check_spill_words(semu.words(ts), n_slots)
    assert n_spill >= n_slots and n_fill >= n_spill


@pytest.mark.parametrize("k", [13, 24])
def test_fan_value_root(semu, k):
    """The 256-bit root t itself (values mode on the device), not only the Bool over it."""
    ts = sc.fan(k, 2, value=True)
    assert semu.spills(ts)[0] > 0
    rows = sc.edge_rows(2, 32, k)
    got, _ = semu.eval(ts, 0, sc.soa(rows, 2))
    assert got == _oracle(ts, rows)


@pytest.mark.parametrize("k,n_regs", [(10, 13), (11, 14), (12, 15)])
def test_fan_that_fits_has_no_spill_code(semu, k, n_regs):
    for chain in (1, 2, 10):
        ts = sc.fan(k, chain)
        assert semu.spills(ts)[0] == 0
        assert spill_ops(semu.words(ts)) == []
        rows = sc.edge_rows(2, 8, k)
        got, got_regs = semu.eval(ts, 0, sc.soa(rows, 2))
        assert got_regs == n_regs
        assert got == _oracle(ts, rows)


def test_slots_are_reused(semu):
    """Slots are numbered by first use and reused after their value's last use: a tape that
    spills many values one after the other needs fewer slots than it has spills."""
    reused = 0
    for seed in (3, 14, 41):
        ts = sc.fuzz_tape(seed)
        n_slots = int(semu.spills(ts)[0])
        n_spill, _ = check_spill_words(semu.words(ts), n_slots)
        assert n_slots > 0 and n_spill >= n_slots
        reused += n_spill > n_slots
        first_use = []
        for _, name, slot, _ in spill_ops(semu.words(ts)):
            if name == "D_SPILL" and slot not in first_use:
                first_use.append(slot)
        assert first_use == sorted(first_use), "slots are numbered by first use"
    assert reused


FUZZ = 210
_fuzz_spilled = {}


@pytest.mark.parametrize("seed", range(FUZZ))
def test_fuzz_matches_oracle(semu, seed):
    ts = sc.fuzz_tape(seed)
    assert 40 <= len(ts.tapes[0].nodes) <= 400
    n_slots = int(semu.spills(ts)[0])
    rows = sc.edge_rows(ts.n_vars, 12, seed)
    got, n_regs = semu.eval(ts, 0, sc.soa(rows, ts.n_vars))
    assert [bool(g) for g in got] == [bool(w) for w in _oracle(ts, rows)]
    words = semu.words(ts)
    n_spill, n_fill = check_spill_words(words, n_slots)
    if n_slots:
        assert n_regs == 15 and n_spill and n_fill
    else:
        assert n_spill == n_fill == 0
    _fuzz_spilled[seed] = (n_slots > 0, len(words) // 2 > WINDOW, ts.n_vars > 4)


def test_fuzz_share_that_spills(semu):
    """At least a third of the fuzz tapes spill (the generator's operand window is drawn for
    it), some of them over more than four columns and across a D_WINDOW."""
    for seed in range(FUZZ):  # (when this test runs alone)
        if seed not in _fuzz_spilled:
            ts = sc.fuzz_tape(seed)
            _fuzz_spilled[seed] = (semu.spills(ts)[0] > 0,
                                   len(semu.words(ts)) // 2 > WINDOW, ts.n_vars > 4)
    spilled = [v for v in _fuzz_spilled.values() if v[0]]
    assert 3 * len(spilled) >= FUZZ, (len(spilled), FUZZ)
    assert sum(1 for v in spilled if v[1]) >= 20, "spilling tapes longer than a window"
    assert sum(1 for v in spilled if v[2]) >= 20, "spilling tapes over more than four columns"
    assert any(not v[0] for v in _fuzz_spilled.values()), "fuzz tapes that fit"


def test_mixed_gpu_set_spills(semu):
    """The sets tests/test_gpu_spill.py runs on the device spill as that file assumes."""
    for n_cols, fit in sc.MIXED_FIT.items():
        got = semu.spills(sc.mixed_set(n_cols))
        assert len(got) == 19
        assert [t for t in range(19) if got[t] == 0] == fit, (n_cols, got)
        plain = semu.spills(sc.mixed_set(n_cols, plain=True))
        assert len(plain) == 20 and plain[8] == 0
        assert np.count_nonzero(plain) == 19 - len(fit)


def test_too_many_slots_is_register_pressure(semu):
    """Beyond MH_SPILL_SLOTS_MAX slots the refusal keeps the words Sieve.compile matches."""
    from tests.emu import EmuError

    assert semu.spills(sc.fan(12 + 256, 1))[0] == 256
    with pytest.raises(EmuError) as e:
        semu.words(sc.fan(12 + 257, 1))
    assert e.value.code == -2 and "register pressure" in str(e.value)


def test_existing_queries_compile_to_the_same_words(emu, semu):
    """tests/golden/interp_words.json was written by scripts/interp_golden.py before the
    allocator could spill: every tape that compiled then compiles to the same words now, with
    the spilling attempt allowed (as the library compiles) and without."""
    import importlib.util

    spec = importlib.util.spec_from_file_location(
        "interp_golden", os.path.join(ROOT, "scripts", "interp_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(mod.GOLDEN) as f:
        want = json.load(f)
    assert len(want) >= 19
    for which in (emu, semu):
        got = mod.records(which)
        assert set(got) == set(want)
        for name, rec in want.items():
            for size_rec, now in zip(rec["whole"], got[name]["whole"]):
                if size_rec is not None:  # (a size refused then may compile with spills now)
                    assert now == size_rec, name
            if rec["buckets"] is not None:
                assert got[name]["buckets"] == rec["buckets"], name


def test_callers_without_spill_hooks_are_still_refused(emu):
    """compile_tape spills only when asked: the suite's emulator, whose machine has no spill
    hooks, still gets the refusal."""
    from tests.emu import EmuError

    with pytest.raises(EmuError) as e:
        emu.words(sc.fan(13, 1))
    assert "register pressure" in str(e.value)


def test_spilling_compile_under_asan_ubsan(semu, tmp_path):
    """The fan and fuzz tapes through a stand-alone AddressSanitizer / UBSan build of the tape
    compiler and the host emulator (tests/native/spill_replay.cpp): slot counts and every output
    word equal this (unsanitized) build's."""
    import struct

    from tests.test_host_sanitized import CSRC, NATIVE, replay, sanitized_build

    import shutil
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    sets = [sc.fan(k, chain) for k in (12, 13, 24, 40) for chain in (1, 10)]
    sets += [sc.fan(24, 2, value=True)] + [sc.fuzz_tape(seed) for seed in range(0, FUZZ, 3)]
    corpus = str(tmp_path / "spill.bin")
    n_spilled = 0
    with open(corpus, "wb") as f:
        f.write(struct.pack("<I", len(sets)))
        for i, ts in enumerate(sets):
            nodes, _, consts = ts.flatten()
            nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
            consts = np.ascontiguousarray(consts, dtype=np.uint32)
            rows = sc.edge_rows(ts.n_vars, 16, i)
            soa = sc.soa(rows, ts.n_vars)
            slots = int(semu.spills(ts)[0])
            n_spilled += slots > 0
            vals, _ = semu.eval(ts, 0, soa)
            out = np.zeros((8, len(rows)), dtype=np.uint32)
            for j, v in enumerate(vals):
                for k in range(8):
                    out[k, j] = (v >> (32 * k)) & 0xFFFFFFFF
            f.write(struct.pack("<IIII", ts.n_vars, len(ts.pool.values), len(rows), len(nodes)))
            f.write(nodes.tobytes() + consts.tobytes() + soa.tobytes())
            f.write(struct.pack("<I", slots) + out.tobytes())
    exe = str(tmp_path / "spill_replay")
    sanitized_build([os.path.join(NATIVE, "spill_emu.cpp"), os.path.join(NATIVE, "spill_replay.cpp"),
                     os.path.join(CSRC, "compile.cpp")], exe)
    stats = replay(exe, corpus)
    assert int(stats["sets"]) == len(sets) and int(stats["spilled"]) == n_spilled > 40
