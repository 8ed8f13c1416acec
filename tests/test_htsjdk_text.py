"""tests/tools/htsjdk_text.py (the printer the GPU tests read the htsjdk-flag BCF2 stream with) pinned on reference data alone, no
device: the reference recorded the same query twice, as htslib's text (the C++ goldens) and as htsjdk's text of the BCF2 stream (the
java_vcf goldens).  The C++ text, encoded as BCF2 by tests/tools/vcf2bcf.py (vector_end padding) and printed by the printer, must be
the Java golden."""
import json
import os
import struct

import pytest

import helpers
from golden_cases import JAVA_CASES, JAVA_MULTI_ARRAY_CASES, JAVA_UNCOVERED, JAVA_CONTIG_INTERVALS

import htsjdk_text
import vcf2bcf

WITH_TWIN = [c for c in JAVA_CASES if c[5] is not None]


def _split(text):
    lines = text.decode().split("\n")
    assert lines[-1] == ""
    lines = lines[:-1]
    return [l for l in lines if l.startswith("#")], [l for l in lines if not l.startswith("#")]


def test_every_java_golden_of_the_fixture_tree_is_a_case():
    """14 java_vcf goldens: each one a row of JAVA_CASES / JAVA_MULTI_ARRAY_CASES; only the two multi-array goldens may be set aside"""
    files = sorted(f for f in os.listdir(os.path.join(helpers.GOLDEN, "outputs")) if "java" in f)
    covered = sorted({c[4] for c in JAVA_CASES} | {c[0] for c in JAVA_MULTI_ARRAY_CASES})
    assert files == covered and len(files) == 14
    assert set(JAVA_UNCOVERED) <= {c[0] for c in JAVA_MULTI_ARRAY_CASES}
    assert sorted(c[0] for c in JAVA_CASES if c[5] is None) == ["java_t6_7_8_vcf_at_8029501"]
    assert set(JAVA_CONTIG_INTERVALS) <= {c[0] for c in JAVA_CASES}


@pytest.mark.parametrize("case", WITH_TWIN, ids=[c[0] for c in WITH_TWIN])
def test_records_of_the_cpp_twin_print_as_the_java_golden(case):
    name, callsets, vid, ov, golden, twin = case
    vid_json = json.load(open(os.path.join(helpers.GOLDEN, "inputs", vid)))
    data, report = vcf2bcf.encode(helpers.golden_text(twin), vid=vid_json)
    _, want = _split(helpers.golden_text(golden))
    assert htsjdk_text.record_lines(data) == want
    if want and "\tGT" in want[0]:
        assert report["vector_end"] > 0          # the vector_end form of padding went through the printer


@pytest.mark.parametrize("case", WITH_TWIN, ids=[c[0] for c in WITH_TWIN])
def test_header_rule_on_the_cpp_twin(case):
    name, callsets, vid, ov, golden, twin = case
    head, _ = _split(helpers.golden_text(twin))
    want, _ = _split(helpers.golden_text(golden))
    assert htsjdk_text.header_lines("\n".join(head)) == want
    # the same through a BCF2 header with IDX keys
    data, _ = vcf2bcf.encode(helpers.golden_text(twin))
    assert b",IDX=" in data
    assert htsjdk_text.stream_to_text(data).decode().split("\n")[:len(want)] == want


@pytest.mark.parametrize("case", JAVA_CASES, ids=[c[0] for c in JAVA_CASES])
def test_oracle_text_of_every_row_prints_as_the_java_golden(case):
    """the rows' own parameters, checked without a device: the CPU oracle's text of the query, encoded and printed, is the golden
    file, header included (this covers the row without a C++ twin)"""
    name, callsets, vid, ov, golden, _ = case
    q, _ = helpers.query_json(callsets, vid, ov, "query")
    text, _, _ = helpers.oracle_run(q, helpers.cells_for(callsets, vid))
    data, _ = vcf2bcf.encode(text)
    assert htsjdk_text.stream_to_text(data) == helpers.golden_text(golden)


@pytest.mark.parametrize("case", JAVA_MULTI_ARRAY_CASES, ids=[c[0] for c in JAVA_MULTI_ARRAY_CASES])
def test_oracle_text_of_three_arrays_prints_as_the_java_golden(case):
    """the two goldens of a query over three arrays: each column partition imported on its own (host importer) and asked for the
    part of the query inside it; the records of the three back to back under one header are the golden file"""
    import genomicsdb_amd
    name, callsets, vid, partitions, (lo, hi) = case
    v = os.path.join(helpers.GOLDEN, "inputs", vid)
    c = os.path.join(helpers.GOLDEN, "inputs", "callsets", callsets)
    lines = None
    for begin, end in partitions:
        cells, _ = genomicsdb_amd.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=begin, column_end=end)
        q, _ = helpers.query_json(callsets, vid, {"query_column_ranges": [[[max(lo, begin), min(hi, end)]]]}, "query")
        text, _, _ = helpers.oracle_run(q, cells)
        hdr, recs = htsjdk_text.parse_stream(vcf2bcf.encode(text)[0])
        if lines is None:
            lines = htsjdk_text.header_lines(hdr.text)
        lines += [htsjdk_text.record_line(hdr, r) for r in recs]
    assert ("\n".join(lines) + "\n").encode() == helpers.golden_text(name)


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


@pytest.mark.parametrize("value,text", [(_f32(1.067), "1.07"), (_f32(-1.067), "-1.067e+00"), (_f32(0.005), "5.000e-03"), (_f32(0.056), "0.056"),
                                        (2.5, "2.50"), (8.0, "8.00"), (_f32(31.72), "31.72"), (_f32(-0.432), "-4.320e-01"), (0.0, "0.00"),
                                        (2.125, "2.13")])
def test_format_vcf_double_known_answers(value, text):
    """the goldens' own numbers, and one exact tie (2.125: Java's Formatter rounds half up)"""
    assert htsjdk_text.format_vcf_double(value) == text


def test_format_vcf_double_edges():
    assert htsjdk_text.format_vcf_double(1e-21) == "0.00" and htsjdk_text.format_vcf_double(-1e-21) == "0.00"
    assert htsjdk_text.format_vcf_double(0.0099996) == "1.000e-02"          # the mantissa rounds up to 10: renormalised
    assert htsjdk_text.format_vcf_double(0.0625) == "0.063" and htsjdk_text.format_vcf_double(0.01) == "0.010"
    assert htsjdk_text.format_vcf_double(1.0) == "1.00" and htsjdk_text.format_vcf_double(-3.0) == "-3.000e+00"


M8, V8 = -128, -127


@pytest.mark.parametrize("vector,text", [([0, M8, M8], "."), ([0, 0], "./."), ([2, 5, 2], "0/1/0"), ([3, 4], "0|1"), ([M8, M8, M8], "."),
                                         ([2, 4, V8], "0/1"), ([0, 1], "./."), ([1, 0, 0], ".|.|."), ([V8, V8], ".")])
def test_gt_known_answers(vector, text):
    """int8 GT vectors: no-call then missing (an absent sample under the flag), phase taken from the FIRST allele"""
    assert htsjdk_text.gt_text(htsjdk_text.BT_INT8, vector) == text


def test_sample_vector_rules():
    t8, t16, tf, tc = htsjdk_text.BT_INT8, htsjdk_text.BT_INT16, htsjdk_text.BT_FLOAT, htsjdk_text.BT_CHAR
    assert htsjdk_text.vector_text(t8, [1, 2, V8, 3]) == "1,2"                # cut at the first vector_end
    assert htsjdk_text.vector_text(t8, [1, M8, 3, M8, M8]) == "1,.,3"         # trailing missing = padding, inner missing = '.'
    assert htsjdk_text.vector_text(t16, [-32768, -32768]) == "." and htsjdk_text.vector_text(t16, [-128, -127]) == "-128,-127"
    assert htsjdk_text.vector_text(t8, []) == "."
    assert htsjdk_text.vector_text(tf, [0x7F800001, 0x7F800001]) == "." and htsjdk_text.vector_text(tf, [0x40200000, 0x7F800002]) == "2.50"
    assert htsjdk_text.vector_text(tc, [0, 0, 0]) == "." and htsjdk_text.vector_text(tc, [7, 0, 0]) == "."
    assert htsjdk_text.vector_text(tc, list(b"0|1\0\0")) == "0|1" and htsjdk_text.vector_text(tc, list(b"a.b")) == "a.b"


def test_expected_flagged_on_a_hand_made_record():
    """the rule the GPU tests hold the flagged stream to (reference variant_field_handler.cc:846-866), on values written by hand"""
    t8, tf, tc = htsjdk_text.BT_INT8, htsjdk_text.BT_FLOAT, htsjdk_text.BT_CHAR
    FM, FV = 0x7F800001, 0x7F800002
    d = htsjdk_text.Record()
    d.shared, d.pos, d.n_sample = b"shared", 4, 3
    d.fmt = [("GT", t8, 3, [[2, 4, 6], [2, V8, V8], [V8, V8, V8]]),
             ("PL", t8, 3, [[1, 2, 3], [7, V8, V8], [M8, V8, V8]]),
             ("XF", tf, 2, [[0x3F800000, FV], [FM, FV], [FM, FM]]),
             ("PID", tc, 3, [list(b"5_A"), [7, 0, 0], [7, 1, 0]])]
    want = [("GT", t8, 3, [[2, 4, 6], [2, M8, M8], [0, M8, M8]]),
            ("PL", t8, 3, [[1, 2, 3], [7, M8, M8], [M8, M8, M8]]),
            ("XF", tf, 2, [[0x3F800000, FM], [FM, FM], [FM, FM]]),
            ("PID", tc, 3, [list(b"5_A"), [0, 0, 0], [7, 1, 0]])]
    assert htsjdk_text.expected_flagged(d) == want
    f = htsjdk_text.Record()
    f.shared, f.pos, f.n_sample, f.fmt = b"shared", 4, 3, want
    assert htsjdk_text.flag_rule_mismatch(d, f) is None
    # what a subtly wrong kernel would write: vector_end left in, the no-call in the wrong slot, one element short, another width
    for q, s, bad in ((1, 1, [7, M8, V8]), (0, 2, [M8, 0, M8]), (0, 2, [0, M8, V8]), (2, 1, [FM, FV]), (3, 1, [7, 0, 0])):
        f.fmt = [(n_, t_, c_, [list(v) for v in per]) for n_, t_, c_, per in want]
        f.fmt[q][3][s] = bad
        assert htsjdk_text.flag_rule_mismatch(d, f) is not None, (q, s)
    f.fmt = [("GT", htsjdk_text.BT_INT16, 3, want[0][3])] + want[1:]
    assert "types" in htsjdk_text.flag_rule_mismatch(d, f)
    f.fmt, f.shared = want, b"Shared"
    assert "shared" in htsjdk_text.flag_rule_mismatch(d, f)


def test_missing_padding_prints_like_vector_end_padding():
    """the two forms of one record: FORMAT vectors padded with vector_end (htslib) and with missing, an absent GT as no-call +
    missing (the htsjdk flag) print the same line"""
    text = (b"##fileformat=VCFv4.2\n##contig=<ID=1,length=1000>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"g\">\n"
            b"##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"p\">\n##FORMAT=<ID=PID,Number=1,Type=String,Description=\"s\">\n"
            b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\tc\n"
            b"1\t5\t.\tA\tC,G\t.\t.\t.\tGT:PL:PID\t0/1/2:1,2,3,4,5,6:5_A\t.:7,8,9:.\t.:.:.\n")
    data, _ = vcf2bcf.encode(text)
    hdr, recs = htsjdk_text.parse_stream(data)
    want = "1\t5\t.\tA\tC,G\t.\t.\t.\tGT:PID:PL\t0/1/2:5_A:1,2,3,4,5,6\t.:.:7,8,9\t."
    assert htsjdk_text.record_line(hdr, recs[0]) == want
    rec = bytearray(recs[0])
    n = 0
    for i in range(8 + struct.unpack_from("<I", rec, 0)[0], len(rec)):       # the individual block holds int8 and char only
        if rec[i] == 0x81:
            rec[i] = 0x80
            n += 1
    assert n == 2 + 2 + 3 + 5       # GT of b and c, PL of b and c
    assert htsjdk_text.record_line(hdr, bytes(rec)) == want
