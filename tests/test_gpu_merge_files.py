"""The windowed merge on the device: merge_cell_files (csrc/kernels/gdb_merge.hip, csrc/host/merge_files_common.hpp) merges files
and memory to a file round by round through a bounded window of device memory.  The expected bytes never come from the code under
test alone: for imported cells the yardstick is the WHOLE import of the mapping by the host importer (held to the reference's goldens
by tests/test_importer_cpu.py), for crafted opaque sources merge_inputs.sorted_merge (tests/merge_files_inputs.py holds the shapes,
which the CPU harness of the planner is held against too).  Every case asserts from the statistics that the windowed path ran."""
import json
import os
import re
import subprocess
import sys

import pytest

import helpers
import merge_files_inputs as mfi
import merge_inputs as mi

pytestmark = pytest.mark.gpu

INPUTS = os.path.join(helpers.GOLDEN, "inputs")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
MAPPINGS = [("t0_1_2.json", 3), ("t6_7_8.json", 3), ("t0_overlapping.json", 1), ("t0_1_2_combined.json", 3)]      # the mappings of test_gpu_merge_cells.py
MAX = 2**63 - 2


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


def _merged(gdb, sources, directory, window, paths=()):
    """the merged bytes and the statistics; the sources whose index is in `paths` are given as files"""
    out = os.path.join(str(directory), "merged.bin")
    srcs = []
    for i, s in enumerate(sources):
        if i in paths:
            p = os.path.join(str(directory), "source%d.bin" % i)
            with open(p, "wb") as f:
                f.write(s)
            srcs.append(p)
        else:
            srcs.append(s)
    st = {}
    n = gdb.merge_cell_files(srcs, out, window_bytes=window, stats=st)
    with open(out, "rb") as f:
        got = f.read()
    os.remove(out)
    assert not os.path.exists(out + ".merge.tmp")
    # the windowed path ran: its rounds, its window and its staging are in the statistics
    assert st["rounds"] >= 1 and st["window_bytes"] > 0 and st["pinned_bytes"] > 0 and st["device_bytes_peak"] > 0 and st["tile"] == mfi.TILE
    assert st["cells_out"] == n == st["cells_in"] and st["bytes_out"] == len(got) == sum(len(s) for s in sources) and st["num_streams"] == len(sources)
    return got, st


def _holds(st, expectations):
    names = dict(rounds="rounds", carried="carried_cells", grown="grown")
    for name, what in expectations.items():
        v = st[names[name]]
        assert (v > 1 if name == "rounds" else v > 0) if what == "pos" else (v == 1 if what == "one" else v == 0), (name, what, st)


# ---- 1. fixture mappings at every split row, in both source orders -----------------------------------------------------------------
@pytest.mark.parametrize("column_begin", [0, 12200])
@pytest.mark.parametrize("callsets,n_rows", MAPPINGS, ids=[m[0] for m in MAPPINGS])
def test_fixture_mappings_at_every_split_row(gdb, tmp_path, callsets, n_rows, column_begin):
    v, c = os.path.join(INPUTS, "vid.json"), os.path.join(INPUTS, "callsets", callsets)
    whole, n_whole = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=column_begin)
    assert n_whole > 0
    if column_begin == 0:
        assert whole == helpers.cells_for(callsets, "vid.json")
    for k in range(n_rows + 1):
        lo = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=column_begin, ub_callset_row_idx=k - 1)[0] if k else b""
        hi = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=column_begin, lb_callset_row_idx=k)[0]
        assert lo == mi.rows_between(whole, 0, k - 1) and hi == mi.rows_between(whole, k, MAX), k
        for window in (1, 512, 1 << 20):
            for srcs, paths in (([lo, hi], ()), ([hi, lo], (0,))):
                got, st = _merged(gdb, srcs, tmp_path, window, paths)
                assert got == whole, (k, window)
                if window == 1:
                    assert st["grown"] > 0, (k, st)      # a one-byte window: correct through growth alone


# ---- 2. synthetic input: three row ranges at a window of 64 KiB -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth(gdb, tmp_path_factory):
    import synth_gvcf_text
    d = str(tmp_path_factory.mktemp("synth_merge_files"))
    v, c = synth_gvcf_text.write_inputs(d, n_files=6, n_lines=2000, multi=3)
    whole, n = gdb.import_cells(v, c, file_root=d)
    parts = [gdb.import_cells(v, c, file_root=d, lb_callset_row_idx=lo, ub_callset_row_idx=hi)[0] for lo, hi in ((0, 2), (3, 5), (6, MAX))]
    for (lo, hi), p in zip(((0, 2), (3, 5), (6, MAX)), parts):
        assert p == mi.rows_between(whole, lo, hi) and len(p) > 0
    return whole, n, parts


@pytest.mark.parametrize("order,paths", [((0, 1, 2), ()), ((2, 1, 0), ()), ((1, 2, 0), ()), ((0, 1, 2), (1,))], ids=["in order", "reversed", "rotated", "one as a file"])
def test_synthetic_three_sources(gdb, synth, tmp_path, order, paths):
    whole, n, parts = synth
    assert n > 4 * mfi.TILE
    got, st = _merged(gdb, [parts[i] for i in order], tmp_path, 65536, paths)
    assert got == whole
    assert st["rounds"] > 1 and st["carried_cells"] > 0 and st["cells_out"] == n


# ---- 3. to 9. crafted sources ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mfi.shapes(), ids=lambda s: s[0])
def test_crafted_shapes_against_the_sorted_merge(gdb, tmp_path, shape):
    name, sources, windows, expectations = shape
    want = mi.sorted_merge(sources)
    for window in windows:
        for paths in ((), (0,)):
            got, st = _merged(gdb, sources, tmp_path, window, paths)
            assert got == want, (window, paths)
            _holds(st, expectations)
    if name.startswith("equal-key runs"):
        kept = [c for r, _, c in mi.split_cells(want) if r == 0]
        assert b"".join(kept) == (sources[0] if name == "equal-key runs" else sources[1])      # the runs' order is kept


def test_a_waiting_source_is_carried_never_dropped(gdb, tmp_path):
    name, sources, windows, _ = [s for s in mfi.shapes() if s[0] == "hi listed before lo"][0]
    got, st = _merged(gdb, sources, tmp_path, windows[0])
    assert got == sources[1] + sources[0]
    # hi's first chunk waits while lo is merged: it is carried in every round but the last
    assert st["carried_cells"] >= st["rounds"] - 1 > 0


# ---- 10. refusals, each at a chunk boundary --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mfi.refusals(), ids=lambda c: c[0])
def test_refusals_keep_the_words_and_leave_no_file(gdb, tmp_path, case):
    name, sources, window, pattern = case
    out = str(tmp_path / "merged.bin")
    last = str(tmp_path / "last.bin")
    with open(last, "wb") as f:
        f.write(sources[-1])
    for srcs in (list(sources), list(sources[:-1]) + [last]):
        with pytest.raises(gdb.GenomicsDBException, match=pattern):
            gdb.merge_cell_files(srcs, out, window_bytes=window)
        assert not os.path.exists(out) and not os.path.exists(out + ".merge.tmp")


# ---- 11. bounded memory: the same generator at N and 4 N cells ---------------------------------------------------------------------------
def test_device_and_pinned_memory_do_not_depend_on_the_length_of_the_sources(gdb, tmp_path):
    stats = []
    for n in (500, 2000):
        sources = [b"".join(mfi.cells64(n, row=0, step=2)), b"".join(mfi.cells64(n, row=1, col0=1, step=2))]
        got, st = _merged(gdb, sources, tmp_path, 8192, (0,))
        assert got == mi.sorted_merge(sources) and st["grown"] == 0 and st["window_bytes"] == 8192
        stats.append(st)
    assert stats[0]["device_bytes_peak"] == stats[1]["device_bytes_peak"] and stats[0]["pinned_bytes"] == stats[1]["pinned_bytes"]
    assert stats[1]["rounds"] > stats[0]["rounds"] > 1
    # the documented multiples of the window: 8.7 for the device (plus bitmaps, scan scratch and control words), 4.7 for the pinned staging
    assert stats[0]["device_bytes_peak"] < 9 * 8192 + (1 << 16) and stats[0]["pinned_bytes"] < 5 * 8192 + (1 << 12)


def test_the_default_window_is_derived_from_the_device(gdb, tmp_path):
    sources = [b"".join(mfi.cells64(300, row=0, step=2)), b"".join(mfi.cells64(300, row=1, col0=1, step=2))]
    got, st = _merged(gdb, sources, tmp_path, 0, (1,))
    assert got == mi.sorted_merge(sources)
    # every source's share of the derived window is capped by its length: both fit, one round
    assert st["rounds"] == 1 and st["window_bytes"] == sum(len(s) for s in sources) and st["grown"] == 0


# ---- 12. vcf2tiledb --merge-window-bytes -------------------------------------------------------------------------------------------------
def _loader(ws, vid, callsets, **more):
    loader = {"row_based_partitioning": False, "produce_tiledb_array": True, "column_partitions": [{"begin": 0, "workspace": str(ws), "array": "arr"}],
              "callset_mapping_file": callsets, "vid_mapping_file": vid, "treat_deletions_as_intervals": True}
    loader.update(more)
    lj = ws / "loader.json"
    lj.write_text(json.dumps(loader))
    return str(lj)


def test_vcf2tiledb_merges_window_by_window(gdb, tmp_path):
    # (the array of the fixture mappings is 860 bytes, one round at a window of 4 096: a synthetic import of 3 600 cells instead, 4
    # single-sample files and one of 2 samples, the last 2 rows the batch)
    import synth_gvcf_text
    d = str(tmp_path / "inputs")
    v, c = synth_gvcf_text.write_inputs(d, n_files=4, n_lines=600, multi=2)
    whole, n_whole = gdb.import_cells(v, c, file_root=d)
    assert n_whole == 3600 and len(whole) > 20 * 4096
    tool = os.path.join(os.path.dirname(gdb.__file__), "vcf2tiledb")

    def run(ws, flags, **more):
        r = subprocess.run([tool] + flags + [_loader(ws, v, c, **more)], cwd=d, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        return r.stderr.decode()
    results = {}
    for flavour, flags in (("in_core", []), ("windowed", ["--merge-window-bytes", "4096"])):
        ws = tmp_path / flavour
        ws.mkdir()
        run(ws, [], lb_callset_row_idx=0, ub_callset_row_idx=3)
        assert (ws / "arr" / "cells.bin").read_bytes() == mi.rows_between(whole, 0, 3)
        err = run(ws, flags, lb_callset_row_idx=4, ub_callset_row_idx=5, delete_and_create_tiledb_array=False)
        results[flavour] = (ws / "arr" / "cells.bin").read_bytes()
        assert sorted(os.listdir(ws / "arr")) == ["cells.bin"]
        windowed = [l for l in err.splitlines() if ",merge_tiledb_array_windowed," in l]
        in_core = [l for l in err.splitlines() if ",merge_tiledb_array," in l]
        if flavour == "in_core":
            assert len(in_core) == 1 and not windowed
            continue
        assert len(windowed) == 1 and not in_core
        fields = windowed[0].split(",")
        value = {fields[i]: fields[i + 1] for i in range(4, len(fields) - 1, 2)}
        assert int(value["rounds"]) > 1 and int(value["streams"]) == 2 and 0 < int(value["window_bytes"]) <= 4096
        assert int(value["cells_out"]) == len(mi.split_cells(results["windowed"]))
    assert results["windowed"] == results["in_core"] == whole
