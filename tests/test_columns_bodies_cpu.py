"""The bodies of the column decoder (genomicsdb_amd/csrc/core/gdb_columns.hpp) on the CPU, through tests/hostsim_columns/, against the plain-Python
model tests/tools/columns_model.py.  Inputs are "bu" streams made without a device by tests/tools/vcf2bcf.py: every text golden of the
query-mode cases of tests/golden_cases.py, and a hand-written VCF that holds what a BCF2 decoder gets wrong first (each condition is asserted
from the model's reading of the records before anything is compared).  The model builds every column twice - from the BCF2 records and from the
VCF text - and the two have to agree before the bodies are looked at.  The same bodies run once more in a stand-alone program built with the
address and undefined-behaviour sanitizers."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import helpers
import bcf2text
import columns_model as cm
import vcf2bcf
from golden_cases import CASES

DIR = os.path.join(helpers.ROOT, "tests", "hostsim_columns")
DTYPE_CODE = {"int8": 1, "int16": 2, "int32": 3, "float32": 5}
NP_OF_CODE = {1: np.int8, 2: np.int16, 3: np.int32, 4: np.int64, 5: np.uint32, 6: np.uint8}      # float columns are compared as bits

_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        L = ctypes.CDLL(os.path.join(DIR, "libhostsim_columns.so"))
        L.hostsim_columns_decode.restype = ctypes.c_void_p
        L.hostsim_columns_decode.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_char_p)] + [ctypes.POINTER(ctypes.c_int32)] * 4 + [ctypes.c_char_p, ctypes.c_uint64]
        L.hostsim_columns_count.argtypes = [ctypes.c_void_p]
        L.hostsim_columns_get.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_void_p)]
        L.hostsim_columns_free.argtypes = [ctypes.c_void_p]
        _lib = L
    return _lib


def field_specs(header_text, fields):
    """[(name, dictionary key, dtype code, width, flags)] as the harness takes them (flags: 1 INFO, 2 float, 4 GT)"""
    hdr, hf = bcf2text.Header(header_text), cm.header_fields(header_text)
    key_of = {name: i for i, name in hdr.ids.items()}
    out = []
    for name, spec in fields.items():
        kind, ident, dtype, width, is_gt, is_float = cm._resolve(name, spec, hf)
        out.append((name, key_of[ident], DTYPE_CODE[dtype], width, (1 if kind == "INFO" else 0) | (2 if is_float else 0) | (4 if is_gt else 0)))
    return out


def bodies(stream, fields, contig_offset_by_name):
    """the columns the kernel bodies make of a "bu" stream; raises RuntimeError with the fault's text"""
    hdr, records = bcf2text.parse_stream(stream)
    page = b"".join(records)
    offs = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
    n_contig = max(hdr.contigs) + 1
    coff = (ctypes.c_int64 * n_contig)(*[contig_offset_by_name.get(hdr.contigs.get(i), 0) for i in range(n_contig)])
    specs = field_specs(hdr.text, fields)
    nf = len(specs)
    names = (ctypes.c_char_p * max(1, nf))(*[s[0].encode() for s in specs])
    cols = [(ctypes.c_int32 * max(1, nf))(*[s[k] for s in specs]) for k in (1, 2, 3, 4)]
    err = ctypes.create_string_buffer(1024)
    L = lib()
    h = L.hostsim_columns_decode(page, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(records), len(hdr.samples), coff, n_contig, nf, names, *cols, err, 1024)
    if not h:
        raise RuntimeError(err.value.decode())
    out = {}
    try:
        for i in range(L.hostsim_columns_count(h)):
            name = ctypes.create_string_buffer(128)
            dtype, ndim, shape, data = ctypes.c_int(), ctypes.c_int(), (ctypes.c_int64 * 3)(), ctypes.c_void_p()
            L.hostsim_columns_get(h, i, name, 128, ctypes.byref(dtype), ctypes.byref(ndim), shape, ctypes.byref(data))
            shp = tuple(shape[:ndim.value])
            n = int(np.prod(shp))
            np_t = np.dtype(NP_OF_CODE[dtype.value])
            raw = ctypes.string_at(data.value, n * np_t.itemsize)
            out[name.value.decode()] = np.frombuffer(raw, dtype=np_t).reshape(shp).copy()
    finally:
        L.hostsim_columns_free(h)
    return out


def same(got, want):
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].dtype, got[name].shape, want[name].dtype, want[name].shape)
        assert np.array_equal(got[name], want[name]), name


def vid_offsets(vid):
    v = json.load(open(os.path.join(helpers.GOLDEN, "inputs", vid)))
    return {name: c["tiledb_column_offset"] for name, c in v["contigs"].items()}


# ---- the goldens ---------------------------------------------------------------------------------------------------------------------
QUERY_CASES = [c for c in CASES if c[5] == "query"]


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_golden_text_through_the_bodies(case):
    name, callsets, vid, ov, golden, mode = case
    text = helpers.golden_text(golden)
    stream, _ = vcf2bcf.encode(text)
    offsets = vid_offsets(vid)
    hdr, records = bcf2text.parse_stream(stream)
    fields = cm.numeric_fields(hdr.text)
    assert "INFO/DP" in fields and "BaseQRankSum" in fields and (ov.get("sites_only_query") or "GT" in fields)
    from_bcf = cm.columns_from_bcf(stream, fields, offsets)
    from_text = cm.columns_from_text(text, fields, offsets)
    assert len(records) > 0 and from_bcf["pos"].shape == (len(records),)
    assert set(from_text) >= set(cm.SITE) and cm.agree(from_bcf, from_text) == []
    same(bodies(stream, fields, offsets), from_bcf)


def test_haploid_and_triploid_genotypes_share_one_width():
    case = [c for c in QUERY_CASES if c[0] == "t0_haploid_triploid_1_2_3_triploid_deletion_vcf_produce_GT"][0]
    stream, _ = vcf2bcf.encode(helpers.golden_text(case[4]))
    want = cm.columns_from_bcf(stream, {"GT": "int8"}, vid_offsets(case[2]))
    gt = want["GT"]
    assert gt.shape[2] == 3 and (gt[:, :, 2] == cm.VEND["int8"]).any() and (gt[:, :, 2] >= 0).any()
    same(bodies(stream, {"GT": "int8"}, vid_offsets(case[2])), want)


# ---- the hand-written input ------------------------------------------------------------------------------------------------------------
PLX16 = ",".join(str(i * 3) for i in range(16))
HAND = "\n".join([
    "##fileformat=VCFv4.2",
    '##FILTER=<ID=q10,Description="q">',
    "##contig=<ID=1,length=1000000>",
    "##contig=<ID=2,length=1000000>",
    '##INFO=<ID=END,Number=1,Type=Integer,Description="e">',
    '##INFO=<ID=AF,Number=A,Type=Float,Description="f">',
    '##INFO=<ID=DP,Number=1,Type=Integer,Description="d">',
    '##INFO=<ID=DB,Number=0,Type=Flag,Description="b">',
    '##INFO=<ID=NM,Number=1,Type=String,Description="n">',
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="g">',
    '##FORMAT=<ID=XI,Number=.,Type=Integer,Description="x">',
    '##FORMAT=<ID=ST,Number=1,Type=String,Description="s">',
    '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="d">',
    '##FORMAT=<ID=PLX,Number=.,Type=Integer,Description="p">',
    '##FORMAT=<ID=XF,Number=.,Type=Float,Description="f">',
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts0\ts1\ts2",
    "1\t100\t.\tA\tC,G\t50.5\t.\tAF=0.25,0.5;DP=30;DB;NM=abc\tGT:XI:ST:DP:PLX\t0/1:5,-120:foo:10:%s\t1:127:ba:.:.\t0|1|2:.,3:q:12:1,2" % PLX16,
    "1\t200\trs1\tAT\t.\t.\tPASS\tEND=250;DP=7\tGT:XI:ST:DP\t./.:127,128:x:300\t0/0:-121:yy\t.:.:.:.",
    "2\t300\t.\tG\tT\t3\tq10\tAF=.\tGT:XI:DP:XF\t1|0:70000,-32761:5:1.5,.\t0/1:1:6:.\t1/1:2:7:2.25",
    "2\t400\t.\tC\tA\t.\t.\t.\tGT:ST\t0/1:a\t0/1:b\t0/1:c",
]) + "\n"
HAND_OFFSETS = {"1": 0, "2": 1000000000}
HAND_FIELDS = {"GT": "int8", "XI": "int32", "DP": "int16", "PLX": "int16", "XF": "float32", "AF": "float32", "INFO/DP": "int8"}


def hand_stream():
    return vcf2bcf.encode(HAND.encode())[0]


def hand_input_holds_what_it_is_meant_to():
    """the conditions the hand-written input is there for, asserted from the model's reading of the records"""
    hdr, records = bcf2text.parse_stream(hand_stream())
    key = {name: i for i, name in hdr.ids.items()}
    recs = [cm.parse_record(r) for r in records]
    # one field in int8, int16 and int32
    assert [r["fmt"][key["XI"]][0] for r in recs[:3]] == [bcf2text.BT_INT8, bcf2text.BT_INT16, bcf2text.BT_INT32]
    # -120 stays int8, -121 does not; 127 next to 128
    assert -120 in recs[0]["fmt"][key["XI"]][1][0] and recs[1]["fmt"][key["XI"]][1][1][0] == -121 and recs[1]["fmt"][key["XI"]][1][0] == [127, 128]
    # a vector of more than 14 elements: the descriptor's count overflows into a typed integer
    assert len(recs[0]["fmt"][key["PLX"]][1][0]) == 16
    assert bytes([0x11, key["PLX"], 0xF1, 0x11, 16]) in records[0]
    # a char block between two requested numeric ones
    order = HAND.split("\n")[16].split("\t")[8].split(":")
    assert order.index("XI") < order.index("ST") < order.index("DP") and recs[0]["fmt"][key["ST"]][0] == bcf2text.BT_CHAR
    # a field absent from some records; a sample with trailing fields dropped
    assert key["XI"] not in recs[3]["fmt"] and key["PLX"] not in recs[1]["fmt"]
    assert HAND.split("\n")[17].split("\t")[10].count(":") == 2 < HAND.split("\n")[17].split("\t")[8].count(":")
    # haploid, diploid and triploid GT in one record; ./. ; phased
    assert [len([v for v in g if v != bcf2text.INT8_VEND]) for g in recs[0]["fmt"][key["GT"]][1]] == [2, 1, 3]
    assert recs[1]["fmt"][key["GT"]][1][0] == [0, 0] and recs[2]["fmt"][key["GT"]][1][0] == [4, 3]
    # an INFO float, an INFO Flag and an INFO string to step over, a record with one allele
    assert recs[0]["info"][key["AF"]][0] == bcf2text.BT_FLOAT and recs[0]["info"][key["DB"]][1] == [] and recs[0]["info"][key["NM"]][0] == bcf2text.BT_CHAR
    assert len(recs[1]["alleles"]) == 1


def test_hand_written_input_through_the_bodies():
    hand_input_holds_what_it_is_meant_to()
    stream = hand_stream()
    from_bcf = cm.columns_from_bcf(stream, HAND_FIELDS, HAND_OFFSETS)
    from_text = cm.columns_from_text(HAND, HAND_FIELDS, HAND_OFFSETS)
    assert cm.agree(from_bcf, from_text) == [] and {"GT", "GT_phase", "XI", "DP", "PLX", "INFO/DP"} <= set(from_text)
    # by hand
    assert from_bcf["GT"].shape == (4, 3, 3) and from_bcf["GT"][0].tolist() == [[0, 1, -127], [1, -127, -127], [0, 1, 2]]
    assert from_bcf["GT_phase"][0].tolist() == [[0, 0, 0], [0, 0, 0], [0, 1, 1]] and from_bcf["GT"][1, 0].tolist() == [-1, -1, -127]
    assert from_bcf["XI"][3].tolist() == [[-2**31, -2**31 + 1]] * 3 and from_bcf["XI"][0, 2].tolist() == [-2**31, 3]
    assert from_bcf["DP"][1].tolist() == [[300], [-32768], [-32768]] and from_bcf["PLX"].shape == (4, 3, 16)
    assert from_bcf["AF"].shape == (4, 2) and from_bcf["AF"][2].tolist() == [0x7F800001, 0x7F800002] and from_bcf["INFO/DP"][:, 0].tolist() == [30, 7, -128, -128]
    assert from_bcf["end"].tolist() == [100, 250, 300, 400] and from_bcf["column"].tolist() == [99, 199, 1000000299, 1000000399]
    assert bytes(from_bcf["alleles"]) == b"A,C,GATG,TC,A" and from_bcf["alleles_off"].tolist() == [0, 5, 7, 10, 13]
    assert from_bcf["qual"].tolist()[1] == 0x7F800001
    same(bodies(stream, HAND_FIELDS, HAND_OFFSETS), from_bcf)
    # a given width that every record fits
    wide = dict(HAND_FIELDS, GT=("int16", 4), XI=("int32", 2))
    same(bodies(stream, wide, HAND_OFFSETS), cm.columns_from_bcf(stream, wide, HAND_OFFSETS))
    # no field at all: the site columns
    same(bodies(stream, {}, HAND_OFFSETS), cm.columns_from_bcf(stream, {}, HAND_OFFSETS))


def test_a_width_below_a_vector_names_field_and_pos():
    stream = hand_stream()
    with pytest.raises(cm.ColumnsError) as e:
        cm.columns_from_bcf(stream, {"PLX": ("int16", 4)}, HAND_OFFSETS)
    assert (e.value.kind, e.value.field, e.value.pos) == ("width", "PLX", 100)
    with pytest.raises(RuntimeError, match=r"field PLX .*width 4.*pos 100\)"):
        bodies(stream, {"PLX": ("int16", 4)}, HAND_OFFSETS)
    # the smallest offending record speaks: XI is too long at pos 100, 200 and 300
    with pytest.raises(RuntimeError, match=r"field XI .*pos 100\)"):
        bodies(stream, {"DP": "int16", "XI": ("int32", 1)}, HAND_OFFSETS)


def test_an_integer_outside_the_dtype_names_field_and_pos():
    stream = hand_stream()
    with pytest.raises(cm.ColumnsError) as e:
        cm.columns_from_bcf(stream, {"DP": "int8"}, HAND_OFFSETS)
    assert (e.value.kind, e.value.field, e.value.pos) == ("range", "DP", 200)
    with pytest.raises(RuntimeError, match=r"field DP .*int8.*pos 200\)"):
        bodies(stream, {"GT": "int8", "DP": "int8"}, HAND_OFFSETS)
    # -121 is one of int8's reserved values, 128 is above it: both at pos 200, nothing at pos 100 (-120 and 127 fit)
    with pytest.raises(RuntimeError, match=r"field XI .*int8.*pos 200\)"):
        bodies(stream, {"XI": "int8"}, HAND_OFFSETS)
    with pytest.raises(RuntimeError, match=r"field XI .*int16.*pos 300\)"):
        bodies(stream, {"XI": "int16"}, HAND_OFFSETS)


def _one_record(xi_per_sample):
    """the hand-written header with one record whose XI values are given per sample"""
    head = HAND.split("\n")[:16]
    return ("\n".join(head + ["1\t100\t.\tA\tC\t.\t.\t.\tGT:XI\t" + "\t".join("0/1:" + x for x in xi_per_sample)]) + "\n").encode()


@pytest.mark.parametrize("xi,block,narrow,wide", [
    (["300,-127", "1", "2"], bcf2text.BT_INT16, "int8", "int16"),        # int8's end-of-vector as a number
    (["300,-128", "1", "2"], bcf2text.BT_INT16, "int8", "int16"),        # int8's missing as a number
    (["-127,5", "1", "2"], bcf2text.BT_INT16, "int8", "int16"),          # ... in front: not a sample without a value either
    (["1", "2", "-128"], bcf2text.BT_INT16, "int8", "int16"),
    (["70000,-32767", "1", "2"], bcf2text.BT_INT32, "int16", "int32"),   # int16's end-of-vector as a number
    (["1", "-32768,70000", "2"], bcf2text.BT_INT32, "int16", "int32"),   # int16's missing as a number
])
def test_a_real_value_that_equals_a_sentinel_of_the_dtype_asked_for(xi, block, narrow, wide):
    """whether an element is missing or end-of-vector is the SOURCE type's to say: -127 in an int16 block is a number, and no int8"""
    stream = vcf2bcf.encode(_one_record(xi))[0]
    hdr, records = bcf2text.parse_stream(stream)
    key = {name: i for i, name in hdr.ids.items()}
    t, per = cm.parse_record(records[0])["fmt"][key["XI"]]
    assert t == block and any(v in (-127, -128, -32767, -32768) for vals in per for v in vals)
    want = cm.columns_from_bcf(stream, {"XI": wide}, HAND_OFFSETS)
    same(bodies(stream, {"XI": wide}, HAND_OFFSETS), want)
    assert [[v for v in row if v != cm.VEND[wide]] for row in want["XI"][0].tolist()] == [[int(v) for v in x.split(",")] for x in xi]
    with pytest.raises(cm.ColumnsError) as e:
        cm.columns_from_bcf(stream, {"XI": narrow}, HAND_OFFSETS)
    assert (e.value.kind, e.value.field, e.value.pos) == ("range", "XI", 100)
    with pytest.raises(RuntimeError, match=r"field XI .*%s.*pos 100\)" % narrow):
        bodies(stream, {"XI": narrow}, HAND_OFFSETS)


def test_a_reserved_code_of_the_source_type_is_no_number():
    """-126 .. -121 of an int8 block are reserved codes that no writer produces: not numbers, whatever dtype is asked for"""
    stream = vcf2bcf.encode(_one_record(["5,-120", "1", "2"]))[0]
    assert stream.count(bytes([0x05, 0x88])) == 1
    stream = stream.replace(bytes([0x05, 0x88]), bytes([0x05, 0x86]))       # -120 -> -122
    with pytest.raises(cm.ColumnsError) as e:
        cm.columns_from_bcf(stream, {"XI": "int32"}, HAND_OFFSETS)
    assert (e.value.kind, e.value.field, e.value.pos) == ("range", "XI", 100)
    with pytest.raises(RuntimeError, match=r"field XI .*pos 100\)"):
        bodies(stream, {"XI": "int32"}, HAND_OFFSETS)


def test_the_limit_of_requests_is_one_number():
    import re
    from genomicsdb_amd import _lib as binding
    pub = re.search(r"#define GDBAMD_MAX_COLUMN_REQUESTS (\d+)", open(os.path.join(helpers.ROOT, "include", "genomicsdb_amd.h")).read())
    assert int(pub.group(1)) == binding.MAX_COLUMN_REQUESTS == len(binding.ColumnsStats().width)


def test_a_record_cut_short_is_refused():
    hdr, records = bcf2text.parse_stream(hand_stream())
    cut = hand_stream()[:-3]
    page = cut[len(cut) - sum(len(r) for r in records) + 3:]
    assert len(page) == sum(len(r) for r in records) - 3
    L = lib()
    offs = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
    offs[-1] -= 3
    err = ctypes.create_string_buffer(1024)
    coff = (ctypes.c_int64 * 2)(0, 10**9)
    empty = (ctypes.c_int32 * 1)()
    h = L.hostsim_columns_decode(page, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(records), 3, coff, 2, 0, (ctypes.c_char_p * 1)(), empty, empty, empty, empty, err, 1024)
    assert not h and "no whole BCF2 record" in err.value.decode() and "pos 400" in err.value.decode()


# ---- the same bodies under the sanitizers ------------------------------------------------------------------------------------------------
def _fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & (2**64 - 1)
    return "%016x" % h


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    subprocess.check_call(["make", "-s", "-C", DIR])
    stream = hand_stream()
    path = tmp_path / "hand.bcf"
    path.write_bytes(stream)
    hdr, _ = bcf2text.parse_stream(stream)
    args = ["%s:%d:%d:%d:%d" % s for s in field_specs(hdr.text, HAND_FIELDS)]
    r = subprocess.run([os.path.join(DIR, "hostsim_columns_main"), str(path), "3", "2"] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = cm.columns_from_bcf(stream, HAND_FIELDS, HAND_OFFSETS)
    got = {ln.split()[0]: ln.split()[3] for ln in r.stdout.splitlines()}
    assert sorted(got) == sorted(want)
    for name, a in want.items():
        assert got[name] == _fnv(a), name
    # the faults, too
    bad = ["%s:%d:%d:%d:%d" % s for s in field_specs(hdr.text, {"DP": "int8"})]
    r = subprocess.run([os.path.join(DIR, "hostsim_columns_main"), str(path), "3", "2"] + bad, capture_output=True, text=True)
    assert r.returncode == 3 and "field DP" in r.stdout and "pos 200" in r.stdout, r.stdout + r.stderr
