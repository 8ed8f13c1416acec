"""The bodies of the input histogram (csrc/core/gdb_histogram.hpp; vcf_histogram) on the CPU, through the stand-alone program
tests/hostsim_histogram (built with the address and undefined-behaviour sanitizers, run as a subprocess), against the plain-Python
model tests/tools/histogram_model.py, which never calls the code under test.  Counts are integers: every comparison is exact.
  check 1  bodies == model on every fixture callset mapping that lists only VCF files (t0_1_2_combined, the multi-sample file, is
           among them: a weight above 1), over the whole vid in wide bins and over [0, 20000] in bins of 116 columns;
  check 2  row bounds that leave out a file, row bounds inside the multi-sample file, column bounds; the BCF2 body on an encoded mapping;
  check 3  the bin arithmetic at its edges; a column above max_histogram_range names file and line;
  check 4  the generator of the device tests really holds the run lengths it is there for;
  check 5  the print, the C symbols, the tool's refusals.
Host code only - no device."""
import json
import os
import subprocess

import numpy as np
import pytest

import helpers
import histogram_inputs as hi                       # (puts tests/tools on the path, which bcf_inputs needs)
from histogram_inputs import histogram_model as model
import bcf_inputs  # noqa: E402

WIDE = (hi.LAST_COLUMN, 310198, 0, model.LAST)      # max_histogram_range, num_bins, column bounds
FINE = (20000, 173, 0, 20000)


@pytest.fixture(scope="module")
def gdb():
    from genomicsdb_amd import build as b
    b.build_native()
    import genomicsdb_amd
    return genomicsdb_amd


@pytest.fixture(scope="module")
def prog():
    from genomicsdb_amd import build as b
    return b.build_hostsim_histogram()


def run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.decode()


def sim(prog, vid, callsets, root, max_range, num_bins, cb=0, ce=model.LAST, lb=0, ub=model.LAST):
    return run(prog, "hist", vid, callsets, root or "-", max_range, num_bins, cb, ce, lb, ub)


def want(vid, callsets, root, max_range, num_bins, cb=0, ce=model.LAST, lb=0, ub=model.LAST):
    info = {}
    counts = model.histogram(vid, callsets, root, max_range, num_bins, cb, ce, lb, ub, info)
    return "stats files %d records %d counted %d\n" % (info["files"], info["records"], info["counted"]) + model.text(counts, max_range), counts, info


def test_the_fixture_list_holds_the_multi_sample_file():
    names = hi.fixture_mappings()
    assert "t0_1_2_combined.json" in names and "t0_1_2.json" in names and "t6_7_8.json" in names and len(names) >= 8
    assert not any("csv" in n or "buffer" in n for n in names)
    assert model.weights(hi.fixture("t0_1_2_combined.json")[1]) == [("inputs/vcfs/t0_1_2_combined.vcf.gz", 3)]


@pytest.mark.parametrize("shape", [WIDE, FINE], ids=["wide", "fine"])
@pytest.mark.parametrize("name", hi.fixture_mappings())
def test_bodies_equal_the_model(prog, name, shape):
    vid, callsets, root = hi.fixture(name)
    text, counts, info = want(vid, callsets, root, *shape)
    assert info["records"] > 0
    if shape is WIDE:
        assert info["counted"] == info["records"] and sum(counts) > 0
    assert sim(prog, vid, callsets, root, *shape) == text


def test_row_bounds_leave_out_a_file_and_column_bounds_cut(prog):
    vid, callsets, root = hi.fixture("t0_1_2.json")
    all_text, all_counts, all_info = want(vid, callsets, root, *FINE)
    text, counts, info = want(vid, callsets, root, *FINE, lb=1, ub=2)
    assert info["files"] == 2 and all_info["files"] == 3 and sum(counts) < sum(all_counts)
    assert sim(prog, vid, callsets, root, *FINE, lb=1, ub=2) == text
    text, counts, info = want(vid, callsets, root, 20000, 173, 12142, 17384)
    assert 0 < info["counted"] < info["records"]
    assert sim(prog, vid, callsets, root, 20000, 173, 12142, 17384) == text
    # reversed bounds are swapped, as the loader does
    assert sim(prog, vid, callsets, root, *FINE, lb=2, ub=1) == want(vid, callsets, root, *FINE, lb=1, ub=2)[0]


@pytest.mark.parametrize("lb,ub,weight", [(1, 1, 1), (0, 1, 2), (0, 2, 3)])
def test_the_weight_is_the_number_of_callsets_inside_the_row_bounds(prog, lb, ub, weight):
    vid, callsets, root = hi.fixture("t0_1_2_combined.json")
    text, counts, info = want(vid, callsets, root, *FINE, lb=lb, ub=ub)
    assert sum(counts) == weight * info["counted"] and info["counted"] > 0
    assert sim(prog, vid, callsets, root, *FINE, lb=lb, ub=ub) == text


def test_the_bcf_body_equals_the_model_on_the_text(prog, tmp_path):
    vid, callsets, root = hi.fixture("t0_1_2.json")
    new_cs, streams, _ = bcf_inputs.encode_mapping(vid, callsets, root, str(tmp_path))
    assert all(s[:5] == b"BCF\x02\x02" for s in streams.values())
    assert sim(prog, vid, new_cs, str(tmp_path), *FINE) == want(vid, callsets, root, *FINE)[0]


def bin_of(prog, max_range, num_bins, col, cb=0, ce=model.LAST):
    return run(prog, "bin", max_range, num_bins, cb, ce, col).splitlines()


def test_bin_arithmetic_at_the_edges(prog):
    assert bin_of(prog, 999, 1, 0) == ["size 1000", "bin 0 lo 0 hi 999"]
    assert bin_of(prog, 999, 1, 999) == ["size 1000", "bin 0 lo 0 hi 999"]
    assert bin_of(prog, 999, 1, 1000) == ["size 1000", "range"]
    # more bins than columns: bins of one column, the bins behind the range stay empty
    assert bin_of(prog, 9, 100, 9) == ["size 1", "bin 9 lo 9 hi 9"]
    assert bin_of(prog, 9, 100, 10) == ["size 1", "range"]
    # size_of_bin = (1000 + 1 + 9) // 10 = 101: the first and last value of bin 3, and its neighbours
    assert bin_of(prog, 1000, 10, 302) == ["size 101", "bin 2 lo 202 hi 302"]
    assert bin_of(prog, 1000, 10, 303) == ["size 101", "bin 3 lo 303 hi 403"]
    assert bin_of(prog, 1000, 10, 403) == ["size 101", "bin 3 lo 303 hi 403"]
    assert bin_of(prog, 1000, 10, 404) == ["size 101", "bin 4 lo 404 hi 504"]
    # max_histogram_range itself is counted and lands in the last bin; one above is the error
    assert bin_of(prog, 1000, 10, 1000) == ["size 101", "bin 9 lo 909 hi 1009"]
    assert bin_of(prog, 1000, 10, 1001) == ["size 101", "range"]
    # outside the column bounds: not counted, and no error even above the range
    assert bin_of(prog, 1000, 10, 99, 100, 200) == ["size 101", "out"]
    assert bin_of(prog, 1000, 10, 5000, 100, 200) == ["size 101", "out"]
    for max_range, num_bins in ((999, 1), (9, 100), (1000, 10), (hi.GEN_RANGE, hi.GEN_NUM_BINS)):
        assert bin_of(prog, max_range, num_bins, 0)[0] == "size %d" % model.size_of_bin(max_range, num_bins)
    assert model.size_of_bin(hi.GEN_RANGE, hi.GEN_NUM_BINS) == hi.GEN_BIN
    assert run(prog, "bin", 10, 0, 0, 10, 1).startswith("error: ") and "histogram: num_bins is 0" in run(prog, "bin", 10, 0, 0, 10, 1)


def test_a_column_at_the_range_counts_and_one_above_names_file_and_line(prog, tmp_path):
    vid, callsets, root, path, line = hi.write_one_line(str(tmp_path / "at"), "1", 1001)        # column 1000
    text, counts, info = want(vid, callsets, root, 1000, 10)
    assert counts[9] == 1 and info["counted"] == 3
    assert sim(prog, vid, callsets, root, 1000, 10) == text
    vid, callsets, root, path, line = hi.write_one_line(str(tmp_path / "above"), "1", 1002)     # column 1001
    with pytest.raises(model.HistogramRange) as e:
        model.histogram(vid, callsets, root, 1000, 10)
    assert (e.value.path, e.value.line) == (path, line) and line == 7
    out = sim(prog, vid, callsets, root, 1000, 10)
    assert out == "error: VCF2BinaryException : a column outside the range of the histogram [0,1000] (%s line 7)\n" % path or \
        out == "error: a column outside the range of the histogram [0,1000] (%s line 7)\n" % path, out
    # with column bounds that leave the record out there is no error
    assert sim(prog, vid, callsets, root, 1000, 10, 0, 1000) == want(vid, callsets, root, 1000, 10, 0, 1000)[0]
    # the splitter's errors in the splitter's words
    vid, callsets, root, path, line = hi.write_one_line(str(tmp_path / "contig"), "chrUn", 5)
    out = sim(prog, vid, callsets, root, 1000, 10)
    assert out.startswith("error: ") and "contig chrUn is not in the vid mapping (%s line 7)" % path in out, out


def test_the_generator_holds_the_run_lengths_it_is_there_for():
    offsets = model.contig_offsets(hi.VID)
    seq = model.bin_sequence(hi.gen_text(), offsets, hi.GEN_RANGE, hi.GEN_NUM_BINS)
    runs = model.runs(seq)
    assert [n for _, n, _ in runs] == [n for _, _, n in hi.GEN_RUNS] and None not in seq
    lengths = {n for _, n, _ in runs}
    assert {1, 63, 64, 65, 300} <= lengths
    assert 650 <= len(seq) <= 750 and len(seq) % 64 != 0 and len(seq) % 256 != 0                      # a last partial wavefront
    assert any(first < 256 * k <= first + n - 1 for first, n, _ in runs for k in (1, 2))              # a run crosses a 256-thread block
    assert any(first % 64 != 0 and (first + n) % 64 != 0 and n > 128 for first, n, _ in runs)         # whole wavefronts inside one run
    assert len({b for _, _, b in runs}) == len(runs)                                                  # no bin comes back: runs are bins
    assert len({ln.split("\t")[0] for ln in hi.gen_lines()}) == 2


def test_the_print_is_the_models_print(gdb):
    assert gdb.histogram_text(np.zeros(7, dtype=np.uint64), 100) == "Histogram: [\n]\n" == model.text([0] * 7, 100)
    counts = [0, 3, 0, 2 ** 40, 1, 0, 0, 0, 0, 7]
    assert gdb.histogram_text(np.array(counts, dtype=np.uint64), 1000) == model.text(counts, 1000)
    assert model.text(counts, 1000) == "Histogram: [\n101,201,3\n303,403,1099511627776\n404,504,1\n909,1009,7\n]\n"
    vid, callsets, root = hi.fixture("t0_1_2.json")
    counts = model.histogram(vid, callsets, root, *FINE)
    assert gdb.histogram_text(np.array(counts, dtype=np.uint64), FINE[0]) == model.text(counts, FINE[0])
    with pytest.raises(ValueError):
        gdb.histogram_text(np.zeros(0, dtype=np.uint64), 100)


def test_c_symbols_are_present(gdb):
    from genomicsdb_amd import _lib
    L = _lib.lib()
    for name in ("gdbamd_input_histogram", "gdbamd_histogram_text"):
        assert name in _lib.SYMBOLS and getattr(L, name)
    header = open(os.path.join(helpers.ROOT, "include", "genomicsdb_amd.h")).read()
    assert "int gdbamd_input_histogram(" in header and "int64_t gdbamd_histogram_text(" in header and "} gdbamd_histogram_stats;" in header
    assert callable(gdb.input_histogram) and callable(gdb.histogram_text)


def _loader(callsets, **more):
    doc = {"row_based_partitioning": False, "column_partitions": [{"begin": 0, "workspace": "/tmp/unused", "array": "unused"}],
           "callset_mapping_file": callsets, "vid_mapping_file": hi.VID}
    doc.update(more)
    return doc


def test_the_tool_refuses_a_json_without_its_keys_and_a_machine_without_a_device(gdb, tmp_path):
    tool = os.path.join(os.path.dirname(gdb.__file__), "vcf_histogram")
    assert os.path.exists(tool)
    hidden = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")      # the child sees no device, wherever the test runs
    vid, callsets, root = hi.fixture("t0_1_2.json")
    for missing in ("num_bins", "max_histogram_range"):
        doc = _loader(callsets, max_histogram_range=20000, num_bins=173)
        del doc[missing]
        lj = tmp_path / ("no_%s.json" % missing)
        lj.write_text(json.dumps(doc))
        r = subprocess.run([tool, str(lj)], cwd=root, capture_output=True, timeout=120, env=hidden)
        assert r.returncode != 0 and '"%s"' % missing in r.stderr.decode() and r.stdout == b"", (missing, r.stderr.decode())
    lj = tmp_path / "whole.json"
    lj.write_text(json.dumps(_loader(callsets, max_histogram_range=20000, num_bins=173)))
    r = subprocess.run([tool, str(lj)], cwd=root, capture_output=True, timeout=120, env=hidden)
    assert r.returncode != 0 and "no HIP device" in r.stderr.decode() and r.stdout == b"", r.stderr.decode()
    r = subprocess.run([tool], capture_output=True, timeout=120, env=hidden)
    assert r.returncode != 0 and "Needs 1 arg" in r.stderr.decode()
