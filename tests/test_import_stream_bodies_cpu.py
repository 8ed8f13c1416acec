"""The bodies of the streaming importer (csrc/core/gdb_import_stream.hpp) on the CPU: the harness tests/hostsim_import_stream runs the
order check, the classification and the compaction order in plain loops inside the caller's loop, as a library and as a stand-alone
program built with the address and undefined-behaviour sanitizers, and is compared batch by batch with the model
tests/tools/stream_import_model.py on the cases of tests/test_import_stream_device.py; the cells of all batches are those of the host
importer.  Also without a GPU: "stream_name" in a callset mapping, the chromosome intervals of a column partition, the JNI symbols."""
import ctypes
import json
import os
import subprocess

import pytest

import helpers
import stream_import_inputs as sii
from stream_import_inputs import model

INPUTS = sii.INPUTS
VID = os.path.join(INPUTS, "vid.json")


@pytest.fixture(scope="module")
def gdb():
    from genomicsdb_amd import build as b
    b.build_native()
    import genomicsdb_amd
    return genomicsdb_amd


@pytest.fixture(scope="module")
def hostsim():
    from genomicsdb_amd import build as b
    lib_path, program = b.build_hostsim_import_stream()
    lib = ctypes.CDLL(lib_path)
    lib.hostsim_import_stream_run.restype = ctypes.c_uint64
    lib.hostsim_import_stream_run.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64]

    def run(case_text, tmp_path):
        n = lib.hostsim_import_stream_run(case_text.encode(), None, 0)
        buf = ctypes.create_string_buffer(n)
        lib.hostsim_import_stream_run(case_text.encode(), buf, n)
        p = tmp_path / "case.txt"
        p.write_text(case_text)
        r = subprocess.run([program, str(p)], capture_output=True, timeout=60)      # address + undefined-behaviour sanitizers: any report fails the run
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == buf.raw
        return buf.raw.decode()
    return run


def _check(hostsim, tmp_path, S, host, capacity, column_begin=0, column_end=sii.MAX_COLUMN):
    writes = S.writes(capacity)
    expected = model.run(S.model_input(writes), column_begin, column_end)
    got = hostsim(sii.hostsim_case_text(S, writes, column_begin, column_end), tmp_path)
    assert got == sii.hostsim_report(expected)
    # the concatenation of the batches is the host importer's column-major order
    want = [(col, row, size) for row, col, size, _ in sii.parse_cells(host(column_begin, column_end))]
    assert [c for b in expected for c in b["cells"]] == want
    bound = model.pending_bound(S.model_input(writes), column_begin, column_end)
    assert max(b["pending_cells"] for b in expected) <= bound[0] and max(b["pending_bytes"] for b in expected) <= bound[1]
    return expected


@pytest.mark.parametrize("treat", [True, False])
@pytest.mark.parametrize("capacity", [1, 20480])
def test_buffer_streams_of_t0_t1_t2(gdb, hostsim, tmp_path, capacity, treat):
    S, host, _, _ = sii.fixture_case(gdb, tmp_path, "t0_1_2_buffer.json", files=sii.buffer_files(), treat=treat)
    expected = _check(hostsim, tmp_path, S, host, capacity)
    if capacity == 1:      # the three streams end at column 17384: those cells wait for the streams to end
        last = [c for c in expected[-1]["cells"] if c[0] == 17384]
        assert len(last) == 3 and expected[-1]["W"] == model.POS_INF and all(c[0] < 17384 for b in expected[:-1] for c in b["cells"])


@pytest.mark.parametrize("callsets,begin", [("t6_7_8.json", 0), ("t0_1_2.json", 12200), ("t0_overlapping.json", 12202), ("t0_1_2_combined.json", 0)])
def test_fixture_mappings_one_record_per_write(gdb, hostsim, tmp_path, callsets, begin):
    S, host, _, _ = sii.fixture_case(gdb, tmp_path, callsets)
    expected = _check(hostsim, tmp_path, S, host, 1, column_begin=begin)
    if begin == 12200:      # (at 12202 every candidate of t0_overlapping is superseded by a record AT the partition begin: no cell is replayed)
        assert sum(b["spanning"] for b in expected) > 0


def test_synthetic_dense_against_sparse(gdb, hostsim, tmp_path):
    sources, rows_of = sii.synthetic_sources()
    host = sii.host_reference(gdb, VID, sources, rows_of, str(tmp_path), False)
    S = sii.Streams(VID, sources, rows_of, host())
    expected = _check(hostsim, tmp_path, S, host, 256)
    writes = S.writes(256)
    # two records at one POS on either side of a write boundary; the dense stream is refilled many times while the sparse one waits
    assert any(S.columns[0][w[-1]] == S.columns[0][v[0]] for w, v in zip(writes[0], writes[0][1:]))
    assert sum(1 for b in expected if b["exhausted"] == [0]) > 10 * len(writes[1])
    _check(hostsim, tmp_path, S, host, [1 << 20, 1])
    _check(hostsim, tmp_path, S, host, 256, column_begin=S.columns[0][150], column_end=S.columns[0][250])


def test_a_stream_that_goes_back_is_named(gdb, hostsim, tmp_path):
    S, host, _, _ = sii.fixture_case(gdb, tmp_path, "t0_1_2_buffer.json", files=sii.buffer_files())
    S.columns[1][1] = S.columns[1][0] - 1
    for capacity in (1, 20480):      # across two writes, and inside one
        writes = S.writes(capacity)
        with pytest.raises(model.StreamOrderError) as e:
            model.run(S.model_input(writes))
        assert (e.value.stream, e.value.record) == (1, 2)
        assert hostsim(sii.hostsim_case_text(S, writes, 0, sii.MAX_COLUMN), tmp_path).endswith("ERROR order 1 2\n")


def test_stream_name_in_a_callset_mapping(gdb, tmp_path):
    """a callset names its source by "filename" or by "stream_name"; both is the reference's error"""
    c = tmp_path / "both.json"
    c.write_text(json.dumps({"callsets": {"HG00141": {"row_idx": 0, "idx_in_file": 0, "filename": "a.vcf", "stream_name": "a_stream"}}}))
    with pytest.raises(gdb.GenomicsDBException, match='Cannot have both "filename" and "stream_name" as the data source for sample/CallSet HG00141'):
        gdb.import_cells(VID, str(c))
    # a stream_name is a source like a filename: the host importer looks for a file of that name
    with pytest.raises(gdb.GenomicsDBException, match="HG00141_stream"):
        gdb.import_cells(VID, os.path.join(INPUTS, "callsets", "t0_1_2_buffer.json"), file_root=str(tmp_path))


def test_chromosome_intervals_of_a_column_partition(gdb):
    contigs = json.load(open(VID))["contigs"]
    names = sorted(contigs, key=lambda k: contigs[k]["tiledb_column_offset"])
    whole = json.loads(gdb.chromosome_intervals(sii.loader_json(VID)))
    assert whole == {"contigs": [{n: [1, contigs[n]["length"]]} for n in names]}
    text = gdb.chromosome_intervals(sii.loader_json(VID, column_begin=12200))
    assert text.startswith('{"contigs":[{"1":[12201,249250621]},{"2":[1,243199373]},') and " " not in text
    inside = json.loads(gdb.chromosome_intervals(sii.loader_json(VID, column_begin=100, column_end=249250621 + 4999)))      # ends inside contig 2, the vid's second
    assert inside == {"contigs": [{"1": [101, 249250621]}, {"2": [1, 5000]}]}
    one = json.loads(gdb.chromosome_intervals(sii.loader_json(VID, column_begin=0, column_end=99999)))                       # ends inside contig 1
    assert one == {"contigs": [{"1": [1, 100000]}]}


def test_jni_importer_symbols_are_exported(gdb):
    lib = os.path.join(os.path.dirname(gdb.__file__), "libtiledbgenomicsdb.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, check=True).stdout.decode()
    for name in ("jniGenomicsDBImporter", "jniInitializeGenomicsDBImporterObject", "jniAddBufferStream", "jniSetupGenomicsDBLoader", "jniWriteDataToBufferStream",
                 "jniImportBatch", "jniGetChromosomeIntervalsForColumnPartition", "jniCopyVidMap", "jniCopyCallsetMap"):
        assert " T Java_com_intel_genomicsdb_importer_GenomicsDBImporterJni_%s\n" % name in out + "\n", name


def test_importer_without_a_device_fails_loudly(gdb, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    imp = gdb.StreamImporter(sii.loader_json(VID))
    try:
        imp.add_buffer_stream("HG00141_stream", False, 1024, b"")
        with pytest.raises(gdb.GenomicsDBException, match="Duplicate buffer stream name HG00141_stream"):
            imp.add_buffer_stream("HG00141_stream", False, 1024, b"")
        with pytest.raises(gdb.GenomicsDBException, match="without calling setup_loader"):
            imp.import_batch()
        with pytest.raises(gdb.GenomicsDBException, match="no HIP device"):
            imp.setup(json.load(open(os.path.join(INPUTS, "callsets", "t0_1_2_buffer.json"))))
    finally:
        imp.close()
