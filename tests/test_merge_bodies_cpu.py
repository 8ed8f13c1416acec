"""The bodies of the cell-stream merge (csrc/core/gdb_merge.hpp) on the CPU, through the harness tests/hostsim_merge, which drives
them tile by tile as the rank kernel of csrc/kernels/gdb_merge.hip does.  The expected order is Python's stable sort of the two key
lists by (column, row), A's keys listed first - so equal keys keep their order inside a stream and A comes first on a tie.  Also the
key extraction from headers at every alignment and the host's walk over the size chain.  Host code only - no device."""
import ctypes
import random
import struct

import pytest

import merge_inputs as mi


@pytest.fixture(scope="module")
def sim():
    from genomicsdb_amd import build as b
    L = ctypes.CDLL(b.build_hostsim_merge()[0])
    L.hm_split.restype = ctypes.c_uint64
    L.hm_split.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
    L.hm_merge.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    L.hm_keys.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    L.hm_walk.restype = ctypes.c_int64
    L.hm_walk.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64]
    return L


def _pack(keys):
    return (ctypes.c_int64 * max(2 * len(keys), 1))(*[x for k in keys for x in k])


def _merge(sim, A, B):
    """-> for every output position the index of its cell in A + B"""
    src = (ctypes.c_uint64 * max(len(A) + len(B), 1))()
    sim.hm_merge(_pack(A), len(A), _pack(B), len(B), src)
    return list(src)[:len(A) + len(B)]


def _expected(A, B):
    keys = A + B
    return sorted(range(len(keys)), key=lambda i: keys[i])


def _sorted_keys(rng, n, cols, rows):
    return sorted((rng.randrange(cols), rng.choice(rows)) for _ in range(n))


def test_tile_size_is_what_the_kernel_uses(sim):
    assert sim.hm_tile() == 1024


def test_lengths_around_the_tile_on_either_side(sim):
    T = sim.hm_tile()
    rng = random.Random(11)
    for na in (0, 1, T - 1, T, T + 1):
        for nb in (0, 1, T - 1, T, T + 1):
            A, B = _sorted_keys(rng, na, 40, (0, 1, 2)), _sorted_keys(rng, nb, 40, (3, 4))       # disjoint rows, as after the checks
            assert _merge(sim, A, B) == _expected(A, B), (na, nb)
            A, B = _sorted_keys(rng, na, 6, (0, 1)), _sorted_keys(rng, nb, 6, (0, 1))             # ties across the sides: A first
            assert _merge(sim, A, B) == _expected(A, B), (na, nb, "ties")


def test_one_side_wholly_before_the_other_and_alternation(sim):
    T = sim.hm_tile()
    rng = random.Random(12)
    lo = _sorted_keys(rng, 2 * T + 3, 100, (0, 1))
    hi = [(c + 1000, r) for c, r in _sorted_keys(rng, T + 7, 100, (2, 3))]
    assert _merge(sim, lo, hi) == _expected(lo, hi) == list(range(len(lo) + len(hi)))
    assert _merge(sim, hi, lo) == _expected(hi, lo)
    even = [(i, 0) for i in range(0, 2 * T + 2, 2)]
    odd = [(i, 1) for i in range(1, 2 * T + 1, 2)]
    assert _merge(sim, even, odd) == _expected(even, odd)
    assert _merge(sim, odd, even) == _expected(odd, even)


def test_long_runs_of_equal_keys_keep_their_order(sim):
    T = sim.hm_tile()
    rng = random.Random(13)
    runs = [(7, 3)] * (3 * T) + [(9, 3)] * (T + 5)
    other = _sorted_keys(rng, T + 1, 14, (4, 5, 6))
    for A, B in ((runs, other), (other, runs), (runs, runs)):
        assert _merge(sim, A, B) == _expected(A, B)


def test_every_diagonal_split(sim):
    rng = random.Random(14)
    A, B = _sorted_keys(rng, 300, 30, (0, 1, 2)), _sorted_keys(rng, 200, 30, (0, 1, 2))
    want = _expected(A, B)
    a, b = _pack(A), _pack(B)
    for d in range(len(want) + 1):
        assert sim.hm_split(d, a, len(A), b, len(B)) == sum(1 for i in want[:d] if i < len(A)), d


def test_keys_from_unaligned_headers_and_the_chain_walk(sim):
    rng = random.Random(15)
    cells = []
    for i in range(64):
        row = rng.randrange(-2**63, 2**63)
        col = rng.randrange(-2**63, 2**63)
        cells.append((row, col, mi.cell(row, col, rng.randbytes(i % 23))))        # sizes 24 .. 46: every alignment of the next header
    data = b"".join(c for _, _, c in cells)
    off = (ctypes.c_uint64 * len(cells))()
    msg = ctypes.create_string_buffer(512)
    assert sim.hm_walk(data, len(data), 0, off, len(cells), msg, 512) == len(cells)
    at = 0
    for i, (_, _, c) in enumerate(cells):
        assert off[i] == at
        at += len(c)
    keys = (ctypes.c_int64 * (2 * len(cells)))()
    size = (ctypes.c_uint64 * len(cells))()
    sim.hm_keys(data, off, len(cells), keys, size)
    for i, (row, col, c) in enumerate(cells):
        assert (keys[2 * i], keys[2 * i + 1], size[i]) == (col, row, len(c))


@pytest.mark.parametrize("cut,offset", [(1, 0), (23, 0), (25, 0), (-1, None)])
def test_a_truncated_chain_names_stream_and_byte_offset(sim, cut, offset):
    data = mi.cell(0, 5, b"") + mi.cell(1, 5, b"x" * 10) + mi.cell(2, 6, b"y" * 3)
    part = data[:cut]
    last = len(mi.cell(0, 5, b"")) + len(mi.cell(1, 5, b"x" * 10))
    msg = ctypes.create_string_buffer(512)
    assert sim.hm_walk(part, len(part), 4, None, 0, msg, 512) == -1
    text = msg.value.decode()
    want = (0 if cut in (1, 23) else 24) if offset is not None else last
    assert "stream 4" in text and "byte offset %d" % want in text and "runs past the end" in text
    bad = struct.pack("<qqQ", 0, 0, 7)
    assert sim.hm_walk(bad, len(bad), 1, None, 0, msg, 512) == -1 and "cell_size 7" in msg.value.decode()
