"""The windowed merge (merge_cell_files) on the CPU, through the harness tests/hostsim_merge_files: the sources, the round planner and
the round loop of csrc/host/merge_files_common.hpp - the code the device path runs - over pools in host memory, with the bodies of
csrc/core/gdb_merge.hpp (the cut, the boundary order check, the carry's address arithmetic) where the device runs them in kernels.
The expected bytes are merge_inputs.sorted_merge over the crafted shapes of tests/merge_files_inputs.py; the refusals' words are
checked too.  Host code only - no device."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import merge_files_inputs as mfi
import merge_inputs as mi


@pytest.fixture(scope="module")
def built():
    from genomicsdb_amd import build as b
    return b.build_hostsim_merge_files()


@pytest.fixture(scope="module")
def sim(built):
    L = ctypes.CDLL(built[0])
    L.hmf_merge.restype = ctypes.c_int64
    L.hmf_merge.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p, ctypes.c_uint64,
                            ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_uint64]
    L.hmf_cut_below.restype = ctypes.c_uint64
    L.hmf_cut_below.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64]
    L.hmf_boundary_in_order.argtypes = [ctypes.c_int64] * 4
    L.hmf_carry_offset.restype = ctypes.c_uint64
    L.hmf_carry_offset.argtypes = [ctypes.c_uint64] * 3
    return L


def _merge(sim, sources, output, window):
    """sources: bytes, or str paths -> (cell count or -1, stats, message)"""
    k = len(sources)
    keep = [s.encode() if isinstance(s, str) else s for s in sources]
    paths = (ctypes.c_char_p * k)(*[v if isinstance(s, str) else None for v, s in zip(keep, sources)])
    data = (ctypes.c_void_p * k)(*[None if isinstance(s, str) else ctypes.cast(ctypes.c_char_p(v), ctypes.c_void_p) for v, s in zip(keep, sources)])
    sizes = (ctypes.c_uint64 * k)(*[0 if isinstance(s, str) else len(v) for v, s in zip(keep, sources)])
    st = (ctypes.c_double * 5)()
    msg = ctypes.create_string_buffer(1024)
    n = sim.hmf_merge(k, paths, data, sizes, str(output).encode(), window, st, msg, 1024)
    return n, dict(rounds=int(st[0]), carried=int(st[1]), grown=int(st[2]), window=int(st[3]), cells_in=int(st[4])), msg.value.decode()


def _holds(st, expectations):
    for name, what in expectations.items():
        v = st[name]
        assert (v > 1 if name == "rounds" else v > 0) if what == "pos" else (v == 1 if what == "one" else v == 0), (name, what, st)


@pytest.mark.parametrize("shape", mfi.shapes(), ids=lambda s: s[0])
def test_crafted_shapes_against_the_sorted_merge(sim, tmp_path, shape):
    name, sources, windows, expectations = shape
    want = mi.sorted_merge(sources)
    out = tmp_path / "merged.bin"
    as_file = tmp_path / "source0.bin"
    as_file.write_bytes(sources[0])
    for window in windows:
        for srcs in (sources, [str(as_file)] + sources[1:]):
            n, st, msg = _merge(sim, srcs, out, window)
            assert n == len(mi.split_cells(want)) == st["cells_in"], (window, msg)
            assert out.read_bytes() == want, window
            assert not os.path.exists(str(out) + ".merge.tmp")
            _holds(st, expectations)
            out.unlink()


def test_a_one_byte_window_is_correct_through_growth_alone(sim, tmp_path):
    rng = mi.rng(40)
    parts = [mi.crafted_stream(rng, 120, (s,), 40) for s in range(3)]
    n, st, msg = _merge(sim, parts, tmp_path / "o", 1)
    assert n == 360 and (tmp_path / "o").read_bytes() == mi.sorted_merge(parts), msg
    assert st["grown"] > 0 and st["window"] > 1


@pytest.mark.parametrize("case", mfi.refusals(), ids=lambda c: c[0])
def test_refusals_keep_the_words_and_count_from_the_start_of_the_source(sim, tmp_path, case):
    name, sources, window, pattern = case
    out = tmp_path / "merged.bin"
    for as_path in (False, True):
        srcs = list(sources)
        if as_path:
            (tmp_path / "last.bin").write_bytes(sources[-1])
            srcs[-1] = str(tmp_path / "last.bin")
        n, st, msg = _merge(sim, srcs, out, window)
        assert n == -1 and re.search(pattern, msg), msg
        assert not out.exists() and not os.path.exists(str(out) + ".merge.tmp")


def test_a_missing_file_and_no_source_are_refused(sim, tmp_path):
    n, _, msg = _merge(sim, [str(tmp_path / "not there")], tmp_path / "o", 4096)
    assert n == -1 and "stream 0: cannot read" in msg
    n, _, msg = _merge(sim, [], tmp_path / "o", 4096)
    assert n == -1 and "at least one stream" in msg


def test_the_cut_is_the_number_of_keys_strictly_below(sim):
    rng = random.Random(41)
    keys = sorted((rng.randrange(12), rng.randrange(4)) for _ in range(500))
    packed = (ctypes.c_int64 * (2 * len(keys)))(*[x for k in keys for x in k])
    for col in range(-1, 14):
        for row in range(-1, 5):
            assert sim.hmf_cut_below(packed, len(keys), col, row) == sum(1 for k in keys if k < (col, row)), (col, row)
    assert sim.hmf_cut_below(packed, 0, 5, 5) == 0
    big = (ctypes.c_int64 * 4)(-2**63, 2**63 - 1, 2**63 - 1, -2**63)
    assert sim.hmf_cut_below(big, 2, 2**63 - 1, -2**63) == 1 and sim.hmf_cut_below(big, 2, 2**63 - 1, 2**63 - 1) == 2


def test_the_boundary_check_and_the_carry_arithmetic(sim):
    assert sim.hmf_boundary_in_order(5, 5, 5, 5) == 1          # equal keys may follow each other
    assert sim.hmf_boundary_in_order(5, 5, 5, 6) == 1 and sim.hmf_boundary_in_order(5, 5, 6, 0) == 1
    assert sim.hmf_boundary_in_order(5, 5, 5, 4) == 0 and sim.hmf_boundary_in_order(5, 5, 4, 9) == 0
    assert sim.hmf_boundary_in_order(-2**63, 0, 2**63 - 1, 0) == 1 and sim.hmf_boundary_in_order(2**63 - 1, 0, -2**63, 0) == 0
    assert sim.hmf_carry_offset(1000, 1000, 0) == 0 and sim.hmf_carry_offset(1064, 1000, 16) == 80
    assert sim.hmf_carry_offset(2**40 + 5, 2**40, 2**41) == 2**41 + 5


def test_the_sanitized_program_agrees_with_the_stable_sort(built, tmp_path):
    r = subprocess.run([built[1], str(tmp_path)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    assert b"hostsim_merge_files: ok" in r.stdout
