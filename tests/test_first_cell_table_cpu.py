"""The first-cell table of the site pass (stage_first_cell, genomicsdb_amd/csrc/core/gdb_stages.hpp): site_first_ref with the table against
site_first_ref with its binary search over the fragment's cells, through tests/hostsim_numtext/, on hand-made and seeded random cell lists
sorted by (column, row).  Both ways of finding a begin's record are run: the position table of the pipeline and the search over the record
starts that wide windows keep."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import helpers

DIR = os.path.join(helpers.ROOT, "tests", "hostsim_numtext")

_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        L = ctypes.CDLL(os.path.join(DIR, "libhostsim_numtext.so"))
        L.hostsim_numtext_first_ref.restype = None
        L.hostsim_numtext_first_ref.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _lib = L
    return _lib


def first_refs(begin, valid, refs, rstart, qb, qe, use_table, use_position_table=1):
    """[(REF text or None)] per record, and the table itself"""
    begin = np.array(begin, dtype=np.int64)
    assert (np.diff(begin) >= 0).all()
    valid = np.array(valid, dtype=np.uint8)
    off = np.cumsum([0] + [len(r) for r in refs]).astype(np.uint32)
    data = b"".join(refs) + b"\0"
    rs = np.array(rstart, dtype=np.int64)
    P = len(rs)
    table = np.full(P + 1, -5, dtype=np.int64)
    at = np.zeros(P + 1, dtype=np.int64)
    ln = np.zeros(P + 1, dtype=np.int32)
    pad = np.zeros(1, dtype=np.int64)
    lib().hostsim_numtext_first_ref((begin if len(begin) else pad).ctypes.data, len(begin), (valid if len(valid) else pad).ctypes.data, off.ctypes.data, data,
                                    (rs if P else pad).ctypes.data, P, qb, qe, use_table, use_position_table, table.ctypes.data, at.ctypes.data, ln.ctypes.data)
    out = [None if at[k] < 0 else data[at[k]:at[k] + ln[k]] for k in range(P)]
    assert all(ln[k] == 0 for k in range(P) if at[k] < 0)
    return out, list(table[:P])


def model(begin, valid, refs, rstart):
    out = []
    for s in rstart:
        cs = [c for c in range(len(begin)) if begin[c] == s]
        out.append(refs[cs[0]] if cs and valid[cs[0]] else None)
    return out


def both_ways(begin, valid, refs, rstart, qb, qe):
    want = model(begin, valid, refs, rstart)
    searched, _ = first_refs(begin, valid, refs, rstart, qb, qe, 0)
    assert searched == want
    for position_table in (1, 0):
        got, table = first_refs(begin, valid, refs, rstart, qb, qe, 1, position_table)
        assert got == want
        for k, s in enumerate(rstart):
            cs = [c for c in range(len(begin)) if begin[c] == s]
            assert table[k] == (cs[0] if cs else -1)
    return want


def test_several_cells_share_a_begin():
    want = both_ways([100, 100, 100, 105, 105], [1, 1, 1, 1, 1], [b"A", b"CC", b"GGG", b"T", b"TA"], [100, 105], 100, 120)
    assert want == [b"A", b"T"]


def test_no_cell_begins_at_a_records_start():
    want = both_ways([90, 100, 110], [1, 1, 1], [b"A", b"C", b"G"], [100, 101, 104, 110], 100, 120)
    assert want == [b"C", None, None, b"G"]


def test_first_cell_has_no_valid_ref():
    want = both_ways([100, 100, 103], [0, 1, 0], [b"A", b"C", b"G"], [100, 103], 100, 110)
    assert want == [None, None]


def test_records_before_the_first_cell_and_behind_the_last():
    want = both_ways([105, 106], [1, 1], [b"A", b"C"], [100, 105, 106, 109], 100, 110)
    assert want == [None, b"A", b"C", None]
    # cells before the window and behind it, and a record at the window's first and last column
    want = both_ways([80, 99, 100, 120, 121, 130], [1] * 6, [b"A", b"C", b"G", b"T", b"AA", b"CC"], [100, 110, 120], 100, 120)
    assert want == [b"G", None, b"T"]


def test_no_cells_and_no_records():
    assert both_ways([], [], [], [100, 101], 100, 110) == [None, None]
    assert both_ways([100], [1], [b"A"], [], 100, 110) == []


@pytest.mark.parametrize("seed", range(20))
def test_random_sorted_cell_lists(seed):
    rng = random.Random(1000 + seed)
    qb = rng.randrange(0, 50) + (2**33 if seed % 5 == 0 else 1000)
    qe = qb + rng.randrange(1, 200)
    begin, pos = [], qb - 30
    for _ in range(rng.randrange(0, 300)):
        if rng.random() < 0.6:
            pos += rng.randrange(0, 4)
        begin.append(pos)
    valid = [rng.random() < 0.7 for _ in begin]
    refs = [bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(1, 5))) for _ in begin]
    rstart = sorted(rng.sample(range(qb, qe + 1), rng.randrange(0, qe - qb + 2)))
    both_ways(begin, valid, refs, rstart, qb, qe)
