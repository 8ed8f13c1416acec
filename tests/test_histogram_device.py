"""The input histogram on the device (csrc/kernels/gdb_histogram.hip; input_histogram(...), vcf_histogram) against the plain-Python
model tests/tools/histogram_model.py.  Counts are integers: every comparison is exact.  Every case also asserts from the statistics
that the kernel ran: at least one batch, the records counted are the model's, and no more atomics than records counted (one per
run of equal bins inside a wavefront).  Inputs: the fixture callset mappings that list only VCF files, and the generator of
tests/histogram_inputs.py, whose bins come in runs of 1, 63, 64, 65 and 300 records, with a run across a 256-thread block and a last
partial wavefront - as plain text, gzip and BGZF, as BCF2 files and as BCF2 streams in memory."""
import json
import os
import subprocess

import numpy as np
import pytest

import helpers
import histogram_inputs as hi                       # (puts tests/tools on the path, which bcf_inputs needs)
from histogram_inputs import histogram_model as model
import bcf_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

WIDE = dict(max_histogram_range=hi.LAST_COLUMN, num_bins=310198)
FINE = dict(max_histogram_range=20000, num_bins=173, column_begin=0, column_end=20000)
GEN = dict(max_histogram_range=hi.GEN_RANGE, num_bins=hi.GEN_NUM_BINS)


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    return hi.write_generated(str(tmp_path_factory.mktemp("hist_gen")))


@pytest.fixture(scope="module")
def gen_want():
    """the model on the generator's text, computed once: (counts, info) with both callsets and with the first only"""
    d = {}

    def of(generated, **rows):
        key = tuple(sorted(rows.items()))
        if key not in d:
            info = {}
            vid, callsets, root = generated["plain"]
            d[key] = (model.histogram(vid, callsets, root, hi.GEN_RANGE, hi.GEN_NUM_BINS, info=info, **rows), info)
        return d[key]
    return of


def want_of(vid, callsets, root, max_histogram_range, num_bins, column_begin=0, column_end=model.LAST, lb=0, ub=model.LAST):
    info = {}
    return model.histogram(vid, callsets, root, max_histogram_range, num_bins, column_begin, column_end, lb, ub, info), info


def check(got, st, counts, info, min_batches=1):
    assert got.dtype == np.uint64 and got.tolist() == counts
    assert st["num_batches"] >= min_batches and st["num_files"] == info["files"]
    assert st["num_records"] == info["records"] and st["num_counted"] == info["counted"] and st["total_weight"] == sum(counts)
    assert (1 if info["counted"] else 0) <= st["num_atomics"] <= info["counted"]


@pytest.mark.parametrize("shape", [WIDE, FINE], ids=["wide", "fine"])
@pytest.mark.parametrize("name", hi.fixture_mappings())
def test_fixture_mappings_equal_the_model(gdb, name, shape):
    vid, callsets, root = hi.fixture(name)
    counts, info = want_of(vid, callsets, root, **shape)
    st = {}
    got = gdb.input_histogram(vid, callsets, file_root=root, stats=st, **shape)
    check(got, st, counts, info)
    assert gdb.histogram_text(got, shape["max_histogram_range"]) == model.text(counts, shape["max_histogram_range"])


@pytest.mark.parametrize("enc,inflate", [("plain", "auto"), ("gzip", "auto"), ("bgzf", "host"), ("bgzf", "device")])
def test_generated_runs_in_three_encodings(gdb, generated, gen_want, enc, inflate):
    counts, info = gen_want(generated)
    assert sum(counts) == 2 * info["counted"] == 2 * sum(n for _, _, n in hi.GEN_RUNS)
    vid, callsets, root = generated[enc]
    st = {}
    got = gdb.input_histogram(vid, callsets, file_root=root, inflate=inflate, stats=st, **GEN)
    check(got, st, counts, info)
    # one batch: a run of n records that begins at record i takes one atomic per wavefront it touches
    if st["num_batches"] == 1:
        assert st["num_atomics"] == sum((first + n - 1) // 64 - first // 64 + 1 for first, n, _ in model.runs(model.bin_sequence(hi.gen_text(), model.contig_offsets(vid), hi.GEN_RANGE, hi.GEN_NUM_BINS)))
    assert (st["ms_inflate"] > 0) == (inflate == "device")


@pytest.mark.parametrize("enc", ["plain", "gzip"])
def test_a_small_text_budget_cuts_runs_at_batch_boundaries(gdb, generated, gen_want, enc):
    counts, info = gen_want(generated)
    vid, callsets, root = generated[enc]
    st = {}
    got = gdb.input_histogram(vid, callsets, file_root=root, text_budget_bytes=6000, stats=st, **GEN)
    check(got, st, counts, info, min_batches=5)


def test_row_bounds_choose_the_weight_of_the_generated_file(gdb, generated, gen_want):
    counts, info = gen_want(generated, lb=1, ub=1)
    both, _ = gen_want(generated)
    assert [2 * c for c in counts] == both
    vid, callsets, root = generated["plain"]
    st = {}
    check(gdb.input_histogram(vid, callsets, file_root=root, lb_callset_row_idx=1, ub_callset_row_idx=1, stats=st, **GEN), st, counts, info)


@pytest.fixture(scope="module")
def bcf(generated, tmp_path_factory):
    """the generator's mapping and t0,t1,t2 as BCF2 -> {name: (vid, new callsets, root of the .bcf files, streams, original mapping)}"""
    d = tmp_path_factory.mktemp("hist_bcf")
    out = {}
    for name, (vid, callsets, root) in (("gen", generated["plain"]), ("t0_1_2", hi.fixture("t0_1_2.json"))):
        new_cs, streams, _ = bcf_inputs.encode_mapping(vid, callsets, root, str(d / name))
        out[name] = (vid, new_cs, str(d / name), streams, (vid, callsets, root))
    return out


@pytest.mark.parametrize("form", ["file", "stream"])
@pytest.mark.parametrize("name,shape,budget", [("gen", GEN, 0), ("gen", GEN, 6000), ("t0_1_2", FINE, 0)], ids=["gen", "gen_small_budget", "t0_1_2"])
def test_bcf2_files_and_streams(gdb, bcf, name, shape, budget, form):
    vid, new_cs, root, streams, original = bcf[name]
    counts, info = want_of(*original, **shape)
    st = {}
    if form == "stream":
        got = gdb.input_histogram(vid, new_cs, file_root="/nonexistent", streams=streams, text_budget_bytes=budget, stats=st, **shape)
    else:
        got = gdb.input_histogram(vid, new_cs, file_root=root, text_budget_bytes=budget, stats=st, **shape)
    check(got, st, counts, info, min_batches=5 if budget else 1)


@pytest.mark.parametrize("lb,ub,weight", [(1, 1, 1), (0, 1, 2), (0, 2, 3)])
def test_the_multi_sample_fixture_weighs_by_its_callsets_inside_the_row_bounds(gdb, lb, ub, weight):
    vid, callsets, root = hi.fixture("t0_1_2_combined.json")
    counts, info = want_of(vid, callsets, root, lb=lb, ub=ub, **FINE)
    assert sum(counts) == weight * info["counted"] > 0
    st = {}
    check(gdb.input_histogram(vid, callsets, file_root=root, lb_callset_row_idx=lb, ub_callset_row_idx=ub, stats=st, **FINE), st, counts, info)


def test_row_bounds_leave_out_a_file(gdb):
    vid, callsets, root = hi.fixture("t0_1_2.json")
    counts, info = want_of(vid, callsets, root, lb=1, ub=2, **FINE)
    assert info["files"] == 2
    st = {}
    check(gdb.input_histogram(vid, callsets, file_root=root, lb_callset_row_idx=1, ub_callset_row_idx=2, stats=st, **FINE), st, counts, info)


def test_column_bounds_cut_a_contig(gdb, generated):
    vid, callsets, root = generated["plain"]
    for cb, ce in ((4100, hi.CONTIG2 + 49), (0, 4149), (hi.CONTIG2 + 50, model.LAST)):
        counts, info = want_of(vid, callsets, root, hi.GEN_RANGE, hi.GEN_NUM_BINS, cb, ce)
        assert 0 < info["counted"] < info["records"]
        st = {}
        check(gdb.input_histogram(vid, callsets, file_root=root, column_begin=cb, column_end=ce, stats=st, **GEN), st, counts, info)
    # the same bounds over a range that the records outside them exceed: they are not counted, so they are no error
    counts, info = want_of(vid, callsets, root, 9999, 10, 0, 4149)
    st = {}
    check(gdb.input_histogram(vid, callsets, file_root=root, max_histogram_range=9999, num_bins=10, column_end=4149, stats=st), st, counts, info)


def test_a_column_above_the_range_names_path_and_line(gdb, generated, tmp_path):
    vid, callsets, root, path, line = hi.write_one_line(str(tmp_path / "above"), "1", 1002)     # column 1001
    with pytest.raises(gdb.GenomicsDBException) as x:
        gdb.input_histogram(vid, callsets, 1000, 10, file_root=root)
    assert "a column outside the range of the histogram [0,1000] (%s line %d)" % (path, line) in str(x.value) and line == 7
    vid, callsets, root, path, line = hi.write_one_line(str(tmp_path / "at"), "1", 1001)        # column 1000: counted, in the last bin
    got = gdb.input_histogram(vid, callsets, 1000, 10, file_root=root)
    assert got.tolist() == want_of(vid, callsets, root, 1000, 10)[0] and got[9] == 1
    # in the generated file the first column above 4199 is that of the 394th record line (193 in front of the run of 300, then its
    # 201st): physical line 398, in the second block of threads and, at the small budget, not in the first batch
    vid, callsets, root = generated["plain"]
    with pytest.raises(model.HistogramRange) as e:
        model.histogram(vid, callsets, root, 4199, 42)
    assert e.value.line == 398
    for budget in (0, 6000):
        with pytest.raises(gdb.GenomicsDBException) as x:
            gdb.input_histogram(vid, callsets, 4199, 42, file_root=root, text_budget_bytes=budget)
        assert "(%s line 398)" % os.path.join(root, "hist_gen.vcf") in str(x.value)
    # the splitter's errors in the splitter's words
    vid, callsets, root, path, line = hi.write_one_line(str(tmp_path / "contig"), "chrUn", 5)
    with pytest.raises(gdb.GenomicsDBException) as x:
        gdb.input_histogram(vid, callsets, 1000, 10, file_root=root)
    assert "contig chrUn is not in the vid mapping (%s line 7)" % path in str(x.value)


def test_refusals(gdb, generated):
    vid, callsets, root = generated["plain"]
    with pytest.raises(gdb.GenomicsDBException, match="num_bins is 0"):
        gdb.input_histogram(vid, callsets, 1000, 0, file_root=root)
    with pytest.raises(gdb.GenomicsDBException, match="max_histogram_range -1 is negative"):
        gdb.input_histogram(vid, callsets, -1, 10, file_root=root)
    # counters that no device holds: through the C call, which refuses before it touches the caller's array (input_histogram would
    # first make an array of that size)
    from genomicsdb_amd import _lib
    L = _lib.lib()
    one =np.zeros(1, dtype=np.uint64)
    rc = L.gdbamd_input_histogram(os.fsencode(vid), os.fsencode(callsets), os.fsencode(root), 2 ** 62, 2 ** 45, 0, model.LAST, 0, model.LAST, 0, 0, 0, 0, None, None, None,
                                  one.ctypes.data, None)
    assert rc == -1 and "%d bins of 8 bytes do not fit in the " % 2 ** 45 in str(_lib.last_error()) and one[0] == 0
    with pytest.raises(gdb.GenomicsDBException, match="stream no_such_file is not a .filename. of the callset mapping"):
        gdb.input_histogram(vid, callsets, 1000, 10, file_root=root, streams={"no_such_file": b""})
    csv_vid = os.path.join(hi.INPUTS, "vid_csv_hand.json")
    csv_cs = os.path.join(hi.INPUTS, "callsets", "csv_hand.json")
    with pytest.raises(gdb.GenomicsDBException, match="csv_hand.csv is a CSV cell file"):
        gdb.input_histogram(csv_vid, csv_cs, 1000, 10, file_root=helpers.GOLDEN)


def _equi_text(counts, bin_size, parts):
    import ctypes
    from genomicsdb_amd import _lib
    L = _lib.lib()
    L.gdbamd_equi_partition_text.restype = ctypes.c_int64
    L.gdbamd_equi_partition_text.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64]
    a = np.array(counts, dtype=np.uint64)
    n = L.gdbamd_equi_partition_text(a.ctypes.data, a.size, 0, bin_size, parts, None, 0)
    assert n > 0
    buf = ctypes.create_string_buffer(n + 1)
    L.gdbamd_equi_partition_text(a.ctypes.data, a.size, 0, bin_size, parts, buf, n)
    return buf.raw[:n].decode()


def test_the_tool_prints_the_models_print_and_the_equi_partitions(gdb, tmp_path):
    tool = os.path.join(os.path.dirname(gdb.__file__), "vcf_histogram")
    vid, callsets, root = hi.fixture("t0_1_2.json")
    doc = {"row_based_partitioning": False, "column_partitions": [{"begin": 0, "workspace": str(tmp_path / "ws"), "array": "unused"}],
           "callset_mapping_file": os.path.join("inputs", "callsets", "t0_1_2.json"), "vid_mapping_file": os.path.join("inputs", "vid.json"),
           "max_histogram_range": 20000, "num_bins": 173}
    lj = tmp_path / "hist.json"
    lj.write_text(json.dumps(doc))
    counts, info = want_of(vid, callsets, root, 20000, 173)
    r = subprocess.run([tool, str(lj)], cwd=root, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == model.text(counts, 20000)
    timer = [ln for ln in r.stderr.decode().splitlines() if ",input_histogram," in ln]
    assert len(timer) == 1 and ",files,3," in timer[0] and ",records,%d," % info["records"] in timer[0] and ",histogram_ms," in timer[0]
    r = subprocess.run([tool, "--equi-partitions", "2", "--inflate-on-host", str(lj)], cwd=root, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == model.text(counts, 20000) + _equi_text(counts, model.size_of_bin(20000, 173), 2)
    # partition 1 of two: only the records that begin at or behind 17000
    doc["column_partitions"] = [{"begin": 0, "workspace": str(tmp_path / "ws"), "array": "a0"}, {"begin": 17000, "workspace": str(tmp_path / "ws"), "array": "a1"}]
    lj.write_text(json.dumps(doc))
    r = subprocess.run([tool, "-r", "1", str(lj)], cwd=root, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == model.text(want_of(vid, callsets, root, 20000, 173, 17000)[0], 20000)
