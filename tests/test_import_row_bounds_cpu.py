"""Row bounds of an incremental import ("lb_callset_row_idx" / "ub_callset_row_idx") in the host importer.  The yardstick is the
WHOLE import of the mapping (held to the reference's goldens by tests/test_importer_cpu.py), taken apart by row in Python: for
every split row k the two bounded imports are exactly its two halves, and their Python sort is the whole import again - also for a
column partition with intervals replayed at its begin, for a multi-sample file split across batches (the divisor of sum-like INFO
values stays the file's sample count) and for a vid with 2-dimensional fields.  Host code only - no device."""
import os

import pytest

import helpers
import merge_inputs as mi

MAPPINGS = [("t0_1_2.json", "vid.json"), ("t6_7_8.json", "vid.json"), ("t0_overlapping.json", "vid.json"), ("t0_1_2_combined.json", "vid.json"),
            ("t0_1_2_all_asa.json", "vid_all_asa.json")]
ROWS = {"t0_overlapping.json": 1}      # rows of the mapping (the others have 3)
MAX = 2**63 - 2


@pytest.fixture(scope="module")
def gdb():
    from genomicsdb_amd import build as b
    b.build_native()
    import genomicsdb_amd
    return genomicsdb_amd


def _paths(callsets, vid):
    return os.path.join(helpers.GOLDEN, "inputs", vid), os.path.join(helpers.GOLDEN, "inputs", "callsets", callsets)


_whole = {}


def _whole_import(gdb, callsets, vid, column_begin):
    key = (callsets, vid, column_begin)
    if key not in _whole:
        v, c = _paths(callsets, vid)
        _whole[key] = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=column_begin)
    return _whole[key]


@pytest.mark.parametrize("column_begin", [0, 12200])
@pytest.mark.parametrize("callsets,vid", MAPPINGS, ids=[m[0] for m in MAPPINGS])
def test_bounded_imports_are_the_halves_of_the_whole_import(gdb, callsets, vid, column_begin):
    v, c = _paths(callsets, vid)
    whole, n_whole = _whole_import(gdb, callsets, vid, column_begin)
    if column_begin == 0:
        assert whole == helpers.cells_for(callsets, vid)
    n_rows = ROWS.get(callsets, 3)
    assert n_whole > 0 and {r for r, _, _ in mi.split_cells(whole)} == set(range(n_rows))
    for k in range(n_rows + 1):
        lo, n_lo = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=column_begin, lb_callset_row_idx=0, ub_callset_row_idx=k - 1) if k else (b"", 0)
        hi, n_hi = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=column_begin, lb_callset_row_idx=k)
        assert lo == mi.rows_between(whole, 0, k - 1), "rows < %d" % k
        assert hi == mi.rows_between(whole, k, MAX), "rows >= %d" % k
        assert n_lo + n_hi == n_whole
        assert mi.sorted_merge([lo, hi]) == whole and mi.sorted_merge([hi, lo]) == whole


def test_a_single_row_of_a_multi_sample_file_keeps_the_files_divisor(gdb):
    """every row of t0_1_2_combined on its own: the cells of that sample in the whole import (INFO DP divided among the 3 samples of the header)"""
    v, c = _paths("t0_1_2_combined.json", "vid.json")
    whole, _ = _whole_import(gdb, "t0_1_2_combined.json", "vid.json", 0)
    parts = []
    for row in range(3):
        st = {}
        part, _ = gdb.import_cells(v, c, file_root=helpers.GOLDEN, lb_callset_row_idx=row, ub_callset_row_idx=row, stats=st)
        assert part == mi.rows_between(whole, row, row) and len(part) > 0
        assert st["num_files"] == 1
        parts.append(part)
    assert mi.sorted_merge(parts) == whole


@pytest.mark.parametrize("lb,ub,rows", [(2, 0, (0, 2)), (-5, 1, (0, 1)), (-7, -3, (0, 0)), (1, 10**12, (1, 2)), (0, MAX, (0, 2)), (1, -4, (0, 1)), (5, 9, None)])
def test_bounds_are_clamped_as_the_reference_clamps_them(gdb, lb, ub, rows):
    """negative -> 0, swapped when reversed, the upper bound capped at the mapping's largest row (genomicsdb_config_base.cc:167-180)"""
    v, c = _paths("t0_1_2.json", "vid.json")
    whole, _ = _whole_import(gdb, "t0_1_2.json", "vid.json", 0)
    got, n = gdb.import_cells(v, c, file_root=helpers.GOLDEN, lb_callset_row_idx=lb, ub_callset_row_idx=ub)
    if rows is None:        # (5, min(9, 2)): no row lies inside
        assert got == b"" and n == 0
    else:
        assert got == mi.rows_between(whole, rows[0], rows[1]) and n > 0


def test_num_files_counts_only_opened_files(gdb, tmp_path):
    """a file without a callset in bounds is not opened: a mapping whose out-of-bounds files do not exist imports, and is not counted"""
    import json
    src = json.load(open(_paths("t0_1_2.json", "vid.json")[1]))
    for name, cs in src["callsets"].items():
        if cs["row_idx"] != 1:
            cs["filename"] = "inputs/vcfs/no_such_file_%d.vcf.gz" % cs["row_idx"]
    m = tmp_path / "callsets.json"
    m.write_text(json.dumps(src))
    v = _paths("t0_1_2.json", "vid.json")[0]
    whole, _ = _whole_import(gdb, "t0_1_2.json", "vid.json", 0)
    st = {}
    got, _ = gdb.import_cells(v, str(m), file_root=helpers.GOLDEN, lb_callset_row_idx=1, ub_callset_row_idx=1, stats=st)
    assert got == mi.rows_between(whole, 1, 1) and st["num_files"] == 1
    with pytest.raises(gdb.GenomicsDBException, match="cannot open"):
        gdb.import_cells(v, str(m), file_root=helpers.GOLDEN, lb_callset_row_idx=1, ub_callset_row_idx=2)
    st = {}
    gdb.import_cells(*_paths("t0_1_2.json", "vid.json"), file_root=helpers.GOLDEN, stats=st)
    assert st["num_files"] == 3
    st = {}
    gdb.import_cells(*_paths("t0_1_2.json", "vid.json"), file_root=helpers.GOLDEN, lb_callset_row_idx=0, ub_callset_row_idx=1, stats=st)
    assert st["num_files"] == 2


def test_loader_json_row_bounds_reach_vcf2tiledb(gdb, tmp_path):
    """the loader JSON's bounds choose the batch the tool writes (host import: no device needed to overwrite)"""
    import json
    import subprocess
    tool = os.path.join(os.path.dirname(gdb.__file__), "vcf2tiledb")
    whole, _ = _whole_import(gdb, "t0_1_2.json", "vid.json", 0)
    for lb, ub, rows in ((0, 1, (0, 1)), (2, 2, (2, 2)), (2, 1, (1, 2)), (-3, 0, (0, 0))):
        loader = {"produce_tiledb_array": True, "column_partitions": [{"begin": 0, "workspace": str(tmp_path), "array": "arr"}],
                  "callset_mapping_file": os.path.join("inputs", "callsets", "t0_1_2.json"), "vid_mapping_file": os.path.join("inputs", "vid.json"),
                  "treat_deletions_as_intervals": True, "lb_callset_row_idx": lb, "ub_callset_row_idx": ub}
        lj = tmp_path / "loader.json"
        lj.write_text(json.dumps(loader))
        r = subprocess.run([tool, str(lj)], cwd=helpers.GOLDEN, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        assert (tmp_path / "arr" / "cells.bin").read_bytes() == mi.rows_between(whole, rows[0], rows[1])
        assert ",files,%d," % (rows[1] - rows[0] + 1) in r.stderr.decode()
