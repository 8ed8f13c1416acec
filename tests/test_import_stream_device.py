"""The streaming importer on the device (csrc/kernels/gdb_import_stream.hip) through StreamImporter: buffer streams of VCF text and
of BCF2 records, written piece by piece.  Every case asserts the cells and the exhausted list of every batch against the model
tests/tools/stream_import_model.py, the concatenation of the batches against the HOST importer on the same records as files, and the
most cells and bytes a batch held against the model's figure and its bound; then the errors, and the same import through the driver
tool, the C ABI underneath StreamImporter and the JNI natives."""
import json
import os
import subprocess

import pytest

import helpers
import stream_import_inputs as sii
from stream_import_inputs import model

pytestmark = pytest.mark.gpu

INPUTS = sii.INPUTS
VID = os.path.join(INPUTS, "vid.json")
KINDS = pytest.mark.parametrize("bcf", [False, True], ids=["vcf_text", "bcf2"])


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


@KINDS
@pytest.mark.parametrize("treat", [True, False], ids=["deletions_as_intervals", "deletions_as_sites"])
@pytest.mark.parametrize("capacity", [1, 20480], ids=["one_record_per_write", "capacity_20480"])
def test_buffer_streams_of_t0_t1_t2(gdb, tmp_path, capacity, treat, bcf):
    """the reference's buffer-stream import (tests/run.py:523-582): the callsets come as a JSON string, none from a file"""
    S, host, v, c = sii.fixture_case(gdb, tmp_path, "t0_1_2_buffer.json", files=sii.buffer_files(), bcf=bcf, treat=treat)
    batches, st = sii.run_streams(lambda: gdb.StreamImporter(sii.loader_json(v, treat=treat)), S, capacity, callsets_json=open(c).read(), host=host)
    cells = b"".join(b for b, _ in batches)
    if capacity == 1:      # the three streams end at column 17384: those cells are held until the streams end
        assert [col for _, col, _, _ in sii.parse_cells(batches[-1][0])] == [17384] * 3 and len(batches) > 2
    if treat and not bcf:
        assert cells == helpers.cells_for("t0_1_2.json", "vid.json")
        q, _ = helpers.query_json("t0_1_2.json", "vid.json", {}, "load")
        s = gdb.GenomicsDBQueryStream(query_json=q, cells=cells, buffer_capacity=1 << 20)
        try:
            assert s.read() == helpers.golden_text("t0_1_2_loading")
        finally:
            s.close()


@KINDS
def test_import_cells_matches_a_stream_name_like_a_filename(gdb, tmp_path, bcf):
    """import_cells(streams=...), the whole-stream path: a callset that names its source by "stream_name" is fed from the stream of that name"""
    S, host, v, c = sii.fixture_case(gdb, tmp_path, "t0_1_2_buffer.json", files=sii.buffer_files(), bcf=bcf)
    whole = {n: S.headers[k] + b"".join(S.records[k]) for k, n in enumerate(S.names)}
    assert gdb.import_cells(v, c, device=0, streams=whole)[0] == host()


@KINDS
def test_overlapping_deletions_t6_t7_t8(gdb, tmp_path, bcf):
    S, host, v, c = sii.fixture_case(gdb, tmp_path, "t6_7_8.json", bcf=bcf)
    sii.run_streams(lambda: gdb.StreamImporter(sii.loader_json(v, c)), S, 1, host=host)


@KINDS
@pytest.mark.parametrize("callsets,begin", [("t0_1_2.json", 12200), ("t0_overlapping.json", 12202)])
def test_partition_begin_candidates_arrive_before_what_decides_them(gdb, tmp_path, callsets, begin, bcf):
    S, host, v, c = sii.fixture_case(gdb, tmp_path, callsets, bcf=bcf)
    _, st = sii.run_streams(lambda: gdb.StreamImporter(sii.loader_json(v, c, column_begin=begin)), S, 1, column_begin=begin, host=host)
    spanning_in_host_cells = sum(1 for _, col, _, _ in sii.parse_cells(host(begin, sii.MAX_COLUMN)) if col < begin)
    assert st["num_spanning_cells"] == spanning_in_host_cells
    if begin == 12200:      # (at 12202 every candidate of t0_overlapping is superseded by a record AT the partition begin: the host importer replays no cell either)
        assert st["num_spanning_cells"] > 0


@KINDS
def test_three_samples_in_one_stream(gdb, tmp_path, bcf):
    """t0_1_2_combined: three rows per record, INFO sums divided among the samples"""
    S, host, v, c = sii.fixture_case(gdb, tmp_path, "t0_1_2_combined.json", bcf=bcf)
    assert len(S.names) == 1 and all(len(rec) == 3 for rec in S.cells[0])
    sii.run_streams(lambda: gdb.StreamImporter(sii.loader_json(v, c)), S, 1, host=host)


@pytest.fixture(scope="module")
def synthetic(gdb, tmp_path_factory):
    out = {}
    sources, rows_of = sii.synthetic_sources()
    for bcf in (False, True):
        host = sii.host_reference(gdb, VID, sources, rows_of, str(tmp_path_factory.mktemp("synth_streams")), bcf)
        out[bcf] = (sii.Streams(VID, sources, rows_of, host(), bcf), host, sii.stream_callsets(rows_of))
    return out


@KINDS
def test_synthetic_dense_stream_against_sparse_stream(gdb, synthetic, bcf):
    """300 records against 12 over the same columns in 256-byte writes: the dense stream is refilled many times while the sparse one
    waits (the refill rule), and two records of one stream at one POS fall on either side of a write boundary (the strict <)"""
    S, host, callsets = synthetic[bcf]
    writes = S.writes(256)
    assert any(S.columns[0][w[-1]] == S.columns[0][u[0]] for w, u in zip(writes[0], writes[0][1:]))
    batches, st = sii.run_streams(lambda: gdb.StreamImporter(sii.loader_json(VID)), S, 256, callsets_json=callsets, host=host)
    assert sum(1 for _, ex in batches if ex == [(0, 0)]) > 10 * len(writes[1])
    assert st["num_records"] == sum(len(r) for r in S.records)
    # the dense stream whole against the sparse one record by record: the first batch keeps most of the dense stream's cells, so the
    # classification and the compaction run over more than one block, and later batches move cells from pool to pool
    batches, st = sii.run_streams(lambda: gdb.StreamImporter(sii.loader_json(VID)), S, [1 << 20, 1], callsets_json=callsets, host=host)
    assert st["max_pending_cells"] > 256 and len(sii.parse_cells(batches[0][0])) < 64 and len(batches) > 10
    # a partition cut out of the middle: candidates at its begin, cells behind its end dropped
    lo, hi = S.columns[0][150], S.columns[0][250]
    sii.run_streams(lambda: gdb.StreamImporter(sii.loader_json(VID, column_begin=lo, column_end=hi)), S, 256, column_begin=lo, column_end=hi, callsets_json=callsets, host=host)


@KINDS
def test_edge_cases(gdb, tmp_path, bcf):
    v = VID
    # a single stream; a write larger than the capacity (every record is: capacity 1)
    S, host, _, c = sii.fixture_case(gdb, tmp_path / "single", "t0_overlapping.json", bcf=bcf)
    assert len(S.names) == 1
    sii.run_streams(lambda: gdb.StreamImporter(sii.loader_json(v, c)), S, 1, host=host, end_with_empty_write=False)
    # a stream that no callset uses: index -1, never reported, and a write to it raises
    S, host, _, c = sii.fixture_case(gdb, tmp_path / "unused", "t0_1_2_buffer.json", files=sii.buffer_files(), bcf=bcf, extra_unused="nobody_stream")
    assert S.used == [True, True, True, False]
    sii.run_streams(lambda: gdb.StreamImporter(sii.loader_json(v, c)), S, 20480, host=host)
    imp = gdb.StreamImporter(sii.loader_json(v, c))
    try:
        for name, head in zip(S.names, S.headers):
            imp.add_buffer_stream(name, bcf, 64, head)
        assert imp.setup() == [0, 1, 2, -1]
        with pytest.raises(gdb.GenomicsDBException, match="stream nobody_stream is not used by a callset"):
            imp.write(3, S.records[3][0])
        # header-only streams: the first batch ends them all, nothing comes out
        cells, exhausted = imp.import_batch()
        assert cells == b"" and exhausted == [] and imp.done
        imp.finish()
    finally:
        imp.close()


def _open(gdb, S, loader, callsets_json="", setup=True):
    imp = gdb.StreamImporter(loader)
    for name, head in zip(S.names, S.headers):
        imp.add_buffer_stream(name, S.bcf, 64, head)
    if setup:
        imp.setup(callsets_json)
    return imp


@KINDS
def test_errors_name_the_stream_and_the_record(gdb, tmp_path, bcf):
    ws = tmp_path / "ws"
    S, host, v, c = sii.fixture_case(gdb, tmp_path / "ref", "t0_1_2_buffer.json", files=sii.buffer_files(), bcf=bcf)
    loader = sii.loader_json(v, c, workspace=str(ws), produce_tiledb_array=True)
    two = S.records[1][:2]
    assert len(two) == 2 and S.columns[1][0] < S.columns[1][1]

    def failing(do, message):
        imp = _open(gdb, S, loader)
        try:
            with pytest.raises(gdb.GenomicsDBException, match=message):
                do(imp)
            with pytest.raises(gdb.GenomicsDBException):      # a failed importer can only be closed
                imp.finish()
        finally:
            imp.close()
        assert not ws.exists() or not any(f.name.startswith("cells.bin") for f in ws.rglob("*"))

    # columns going back inside one write, and across two writes
    def back_in_one_write(imp):
        imp.write(0, S.records[0][0]); imp.write(1, two[1] + two[0]); imp.write(2, S.records[2][0])
        imp.import_batch()
    failing(back_in_one_write, "stream HG01958_stream: record 2 lies at a column in front of the record before it")

    def back_across_writes(imp):
        imp.write(0, S.records[0][0]); imp.write(1, two[1]); imp.write(2, S.records[2][0])
        _, exhausted = imp.import_batch()
        for s, _ in exhausted:
            imp.write(s, b"".join(S.records[s][1:2]))
        imp.write(1, two[0])      # (not reported: its last column lies behind W; the write is taken all the same)
        imp.import_batch()
    failing(back_across_writes, "stream HG01958_stream: record 2 lies at a column in front of the record before it")

    # a write cut inside a record
    cut = two[0] + two[1][:len(two[1]) // 2]
    failing(lambda imp: imp.write(1, cut), "stream HG01958_stream: the write ends inside .* that begins at byte offset %d of" % (len(S.headers[1]) + len(two[0])))

    # is_bcf contradicting the header, import_batch before setup
    imp = gdb.StreamImporter(loader)
    try:
        for name, head in zip(S.names, S.headers):
            imp.add_buffer_stream(name, not bcf, 64, head)
        with pytest.raises(gdb.GenomicsDBException, match="stream HG00141_stream was added as %s, but its initialisation bytes" % ("VCF text" if bcf else "BCF2")):
            imp.setup()
    finally:
        imp.close()
    imp = _open(gdb, S, loader, setup=False)
    try:
        with pytest.raises(gdb.GenomicsDBException, match="Cannot import a batch in the GenomicsDBImporter without calling setup_loader"):
            imp.import_batch()
        imp.setup()
        with pytest.raises(gdb.GenomicsDBException, match="Cannot add buffer stream once setup_loader"):
            imp.add_buffer_stream("late", bcf, 64, S.headers[0])
        with pytest.raises(gdb.GenomicsDBException, match="partition index 1"):
            imp.write(0, S.records[0][0], partition_idx=1)
    finally:
        imp.close()
    assert not ws.exists() or not any(f.name.startswith("cells.bin") for f in ws.rglob("*"))


def _loader_file(tmp_path, name, callsets, **kw):
    ws = tmp_path / name
    ws.mkdir()
    loader = {"row_based_partitioning": False, "produce_combined_vcf": True, "produce_tiledb_array": True, "column_partitions": [{"begin": 0, "workspace": str(ws), "array": "arr"}],
              "callset_mapping_file": os.path.join("inputs", "callsets", callsets), "vid_mapping_file": os.path.join("inputs", "vid.json"),
              "treat_deletions_as_intervals": True, "vcf_header_filename": os.path.join("inputs", "template_vcf_header.vcf"),
              "reference_genome": os.path.join("inputs", "chr1_10MB.fasta.gz"), "segment_size": 40}
    loader.update(kw)
    (ws / "loader.json").write_text(json.dumps(loader))
    return ws


def test_driver_tool_and_jni_natives_make_the_array_of_vcf2tiledb(gdb, tmp_path):
    pkg = os.path.dirname(gdb.__file__)
    mapping = os.path.join("inputs", "callsets", "t0_1_2_buffer_mapping.json")
    ws = _loader_file(tmp_path, "files", "t0_1_2.json")
    r = subprocess.run([os.path.join(pkg, "vcf2tiledb"), "--import-on-device", str(ws / "loader.json")], cwd=helpers.GOLDEN, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    want = (ws / "arr" / "cells.bin").read_bytes()
    assert want and r.stdout == helpers.golden_text("t0_1_2_loading")
    # the driver tool: 64-byte buffers, so every record goes alone; combined VCF and array
    ws = _loader_file(tmp_path, "tool", "t0_1_2_buffer.json")
    r = subprocess.run([os.path.join(pkg, "test_genomicsdb_importer"), "-l", str(ws / "loader.json"), "-b", "64", mapping], cwd=helpers.GOLDEN, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == helpers.golden_text("t0_1_2_loading") and (ws / "arr" / "cells.bin").read_bytes() == want
    # array only: the batches are spooled to cells.bin.import.tmp and renamed in finish()
    ws = _loader_file(tmp_path, "spool", "t0_1_2_buffer.json", produce_combined_vcf=False)
    r = subprocess.run([os.path.join(pkg, "test_genomicsdb_importer"), "-l", str(ws / "loader.json"), "-b", "64", mapping], cwd=helpers.GOLDEN, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert sorted(f.name for f in (ws / "arr").iterdir()) == ["cells.bin"] and (ws / "arr" / "cells.bin").read_bytes() == want
    # the JNI natives in GATK's order, through a JVM-less harness
    from genomicsdb_amd import build as b
    harness = b.build_jni_importer_harness()
    ws = _loader_file(tmp_path, "jni", "t0_1_2_buffer.json", produce_combined_vcf=False)
    r = subprocess.run([harness, os.path.join(pkg, "libtiledbgenomicsdb.so"),
                        str(ws / "loader.json"), mapping, "64"], cwd=helpers.GOLDEN, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode() + r.stdout.decode()
    assert (ws / "arr" / "cells.bin").read_bytes() == want
    assert '{"contigs":[{"1":[1,249250621]}' in r.stdout.decode()
