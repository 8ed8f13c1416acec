"""The BCF2 stream a GATK caller reads - is_bcf, use_missing_values_only_not_vector_end, no IDX keys, the flags
GenomicsDBFeatureReader always passes (reference GenomicsDBQueryStream.java:39-41) - against what the reference recorded of it: the
java_vcf goldens, htsjdk's text of that stream.  tests/tools/htsjdk_text.py is the printer (pinned on the CPU by
tests/test_htsjdk_text.py); the flag's branches of the BCF2 page kernel are also held to the exact rule of the reference's
collect_and_extend_fields on the synthetic shapes of tests/variant_shapes.py (every lane count and integer width)."""
import ctypes
import json
import os
import subprocess

import pytest

import helpers
import variant_shapes as vs
from golden_cases import FULL, JAVA_CASES, JAVA_CONTIG_INTERVALS, JAVA_MULTI_ARRAY_CASES, JAVA_UNCOVERED

import htsjdk_text
import vcf2bcf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    from genomicsdb_amd import _lib
    assert _lib.lib().gdb_mi355_device_count() > 0, "no HIP device"
    return genomicsdb_amd


def _assert_no_vector_end(data):
    """htsjdk has no vector_end value: none may be left in a FORMAT block of the stream it reads (the printer, which also reads
    htslib's form of padding, would cut a vector there and hide it)"""
    hdr, recs = htsjdk_text.parse_stream(data)
    for r in recs:
        r = htsjdk_text.decode_record(hdr, r)
        for fname, t, n, per in r.fmt:
            if t != htsjdk_text.BT_CHAR:
                assert not any(htsjdk_text._missing_vend(t)[1] in v for v in per), (r.pos + 1, fname)


def _java_stream(gdb, q, cells):
    s = gdb.GenomicsDBQueryStream(query_json=q, cells=cells, buffer_capacity=1 << 20, is_bcf=True, use_missing_values_only_not_vector_end=True,
                                  keep_idx_fields_in_bcf_header=False)
    data = s.read()
    s.close()
    return data


@pytest.mark.parametrize("case", JAVA_CASES, ids=[c[0] for c in JAVA_CASES])
def test_java_stream_prints_as_the_java_golden(gdb, case, monkeypatch):
    """header and records of the flagged stream through the printer = the golden FILE, byte for byte; in one page and in pages of 700
    bytes the stream is the same bytes"""
    name, callsets, vid, ov, golden, _ = case
    cells = helpers.cells_for(callsets, vid)
    q, _ = helpers.query_json(callsets, vid, ov, "query")
    one_page = _java_stream(gdb, q, cells)
    assert one_page[:5] == b"BCF\x02\x02" and b",IDX=" not in one_page
    assert htsjdk_text.stream_to_text(one_page) == helpers.golden_text(golden)
    _assert_no_vector_end(one_page)
    monkeypatch.setenv("GDBAMD_DEVICE_PAGE_BYTES", "700")
    assert _java_stream(gdb, q, cells) == one_page


MULTI = [c for c in JAVA_MULTI_ARRAY_CASES if c[0] not in JAVA_UNCOVERED]


@pytest.mark.parametrize("case", MULTI, ids=[c[0] for c in MULTI])
def test_java_streams_of_three_arrays_print_as_the_java_golden(gdb, case, monkeypatch):
    """the query over the three arrays of the reference's multi-contig import: every column partition imported on its own, one
    flagged stream each over the part of the query inside its array (GenomicsDBFeatureIterator.java:114-118 - a reference block that
    crosses a partition's end is cut there: END=12160, then 12161-12200), their records in order under one header = the golden file"""
    name, callsets, vid, partitions, (lo, hi) = case
    v = os.path.join(helpers.GOLDEN, "inputs", vid)
    c = os.path.join(helpers.GOLDEN, "inputs", "callsets", callsets)
    for page_bytes in (None, "700"):
        if page_bytes:
            monkeypatch.setenv("GDBAMD_DEVICE_PAGE_BYTES", page_bytes)
        lines, streams = None, []
        for begin, end in partitions:
            cells, _ = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=begin, column_end=end)
            q, _ = helpers.query_json(callsets, vid, {"query_column_ranges": [[[max(lo, begin), min(hi, end)]]]}, "query")
            data = _java_stream(gdb, q, cells)
            streams.append(data)
            _assert_no_vector_end(data)
            hdr, recs = htsjdk_text.parse_stream(data)
            if lines is None:
                lines = htsjdk_text.header_lines(hdr.text)
            lines += [htsjdk_text.record_line(hdr, r) for r in recs]
        if page_bytes is None:
            assert ("\n".join(lines) + "\n").encode() == helpers.golden_text(name)
            first = streams
        else:
            assert streams == first


def test_java_goldens_through_the_jni_natives_with_a_contig_interval(gdb, tmp_path):
    """the two goldens the reference asks for as a contig interval: jniGenomicsDBInit(chr, start, end) with the three flags as Java
    passes them (tests/jni_harness), the query JSON itself covering the whole array"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(helpers.ROOT, "tests", "jni_harness")])
    H = ctypes.CDLL(os.path.join(helpers.ROOT, "tests", "jni_harness", "libjniharness.so"))
    H.jni_harness_read_stream_flags.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p,
                                                ctypes.c_uint64]
    assert len(JAVA_CONTIG_INTERVALS) == 2
    for name, (contig, begin, end) in JAVA_CONTIG_INTERVALS.items():
        _, callsets, vid, ov, golden, _ = [c for c in JAVA_CASES if c[0] == name][0]
        q, _ = helpers.query_json(callsets, vid, dict(ov, query_column_ranges=FULL), "query")
        ws = tmp_path / name
        (ws / "array").mkdir(parents=True)
        (ws / "array" / "cells.bin").write_bytes(helpers.cells_for(callsets, vid))
        q["workspace"] = str(ws)
        q["array"] = "array"
        qf = ws / "query.json"
        qf.write_text(json.dumps(q))
        out, n = ctypes.c_void_p(), ctypes.c_uint64()
        err = ctypes.create_string_buffer(2048)
        rc = H.jni_harness_read_stream_flags(b"", str(qf).encode(), contig.encode(), begin, end, 1, 1, 0, 3000, 0, ctypes.byref(out), ctypes.byref(n), err, 2048)
        assert rc == 0, err.value
        data = ctypes.string_at(out.value, n.value)
        H.jni_harness_free(out)
        assert data[:5] == b"BCF\x02\x02" and b",IDX=" not in data
        assert htsjdk_text.stream_to_text(data) == helpers.golden_text(golden), name
        _assert_no_vector_end(data)


# ---- the flag's branches behind every lane count and width: the synthetic shapes ------------------------------------------------------
def _engine_header_text(eng):
    h = eng.header
    if h[:5] == b"BCF\x02\x02":
        h = h[9:]
    return h.rstrip(b"\x00").decode()


# the four shapes of tests/variant_shapes.py, and mid's cells under a callset mapping of three more samples: rows without a cell, absent
# from every record (in the four shapes every sample has a call at every record, so no GT is absent there)
SHAPE_NAMES = ["plain", "mid", "wide", "long", "mid_absent"]
ABSENT_ROWS = 3


def _build_shape(name, tmp):
    if name != "mid_absent":
        return vs.build(name, tmp)
    from genomicsdb_amd import synth
    N, begin, end, cells, _ = vs.inputs("mid", tmp)
    d = os.path.join(str(tmp), name)
    os.makedirs(d, exist_ok=True)
    q = helpers.synth_query(d, N + ABSENT_ROWS, begin, end)
    want, nrec, _ = helpers.oracle_run_synth(q, cells, synth.SEED, with_header=False)
    return vs.Shape(name, N + ABSENT_ROWS, begin, end, cells, q, want, nrec)


@pytest.fixture(scope="module")
def shape_streams(gdb, tmp_path_factory):
    """name -> (shape, header text, Header, decoded records of the default BCF2 body, decoded records of the flagged body); the
    engines run once per shape, when a test first asks.  On the way: the flagged body in one page and in pages of 256 KiB is the
    same bytes, and both engines give the shape's record count"""
    tmp, made = tmp_path_factory.mktemp("java_shapes"), {}

    def get(name):
        if name in made:
            return made[name]
        shape = _build_shape(name, tmp)
        ref = vs.reference_bases(shape.begin, shape.end)
        bodies = {}
        for flag in (False, True):
            e = gdb.CombineEngine(shape.query, is_bcf=True, use_missing_values_only_not_vector_end=flag)
            e.stage_cells(shape.cells)
            e.set_reference(shape.begin, ref)
            body, st = e.run_interval(shape.begin, shape.end, arena_bytes=1 << 30)
            assert st.num_records == shape.nrec and st.pages == 1, (name, flag, st.num_records, st.pages)
            if flag:
                paged, sp = e.run_interval(shape.begin, shape.end, arena_bytes=1 << 18)
                assert sp.num_records == shape.nrec and sp.pages >= 2, (name, sp.num_records, sp.pages)
                assert paged == body, name
                header_text = _engine_header_text(e)
            bodies[flag] = body
            e.close()
        hdr = htsjdk_text.Header(header_text)
        default = [htsjdk_text.decode_record(hdr, r) for r in htsjdk_text.split_records(bodies[False])]
        flagged = [htsjdk_text.decode_record(hdr, r) for r in htsjdk_text.split_records(bodies[True])]
        assert len(default) == len(flagged) == shape.nrec, name
        made[name] = (shape, header_text, hdr, default, flagged)
        return made[name]
    return get


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_flagged_bcf_follows_the_reference_rule_on_the_synthetic_shapes(shape_streams, name):
    """130 / 150 samples (a partial last 64-sample chunk), int8 and int16 FORMAT vectors, entries past 512 bytes: every record of the
    flagged body is exactly what the rule of the reference's collect_and_extend_fields makes of the default body's record - the
    shared block byte for byte, the FORMAT fields as raw integers and float bit patterns"""
    shape, _, _, default, flagged = shape_streams(name)
    for d, f in zip(default, flagged):
        assert htsjdk_text.flag_rule_mismatch(d, f) is None
    # the rule is not vacuous: vector_end padding behind values, more than one integer width, and (mid_absent) samples with nothing at all
    padded = absent = 0
    widths = set()
    for d in default:
        for fname, t, n, per in d.fmt:
            widths.add(t)
            vend = htsjdk_text._missing_vend(t)[1] if t != htsjdk_text.BT_CHAR else None
            for v in per:
                if fname == "GT":
                    absent += v[0] == vend
                elif vend is not None and v[0] != vend and v[-1] == vend:
                    padded += 1
    assert padded >= 1, name
    assert {htsjdk_text.BT_INT8, htsjdk_text.BT_INT16} <= widths, (name, widths)
    if name == "mid_absent":
        assert absent == ABSENT_ROWS * shape.nrec, absent
    for f in flagged:
        for fname, t, n, per in f.fmt:
            if t != htsjdk_text.BT_CHAR:
                vend = htsjdk_text._missing_vend(t)[1]
                assert not any(vend in v for v in per), (name, f.pos, fname)


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_flagged_bcf_of_the_synthetic_shapes_prints_like_the_oracle_text(shape_streams, name):
    """the flagged body through the printer the Java goldens pin = that printer over the oracle's text of the shape, encoded as BCF2
    with vector_end padding by tests/tools/vcf2bcf.py (under the engine's header): the synthetic widths tied to the same printer.
    The oracle's text holds a float in six significant digits (RAW_MQ=1.03574e+06 for 1035735.375), so the stream's floats go through
    that text (the oracle's format_float, read back as a float) before they are printed: the comparison is made at the precision the
    text has.  The floats' own bits are held to the default stream's by the rule test, and the default stream to the text elsewhere."""
    import struct
    shape, header_text, hdr, _, flagged = shape_streams(name)
    seen = {}

    def through_text(bits):
        if bits not in seen:
            text = helpers.format_float(struct.unpack("<f", struct.pack("<I", bits))[0])
            seen[bits] = struct.unpack("<I", struct.pack("<f", float(text)))[0]
        return seen[bits]
    want_stream, _ = vcf2bcf.encode(header_text.rstrip("\n").encode() + b"\n" + shape.want)
    assert [htsjdk_text.record_line(hdr, f, float_bits=through_text) for f in flagged] == htsjdk_text.record_lines(want_stream)
