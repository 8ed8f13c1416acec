"""The BCF2 path of the device importer on the CPU, through the harness tests/hostsim_import_bcf (header parse, record walk,
index, measure, write, partition-begin rule, sort and gather as plain loops around the bodies of csrc/core/gdb_import_bcf.hpp and
the host share csrc/host/import_bcf.hpp).  The expected cells never come from the code under test: they are the host TEXT
importer's (csrc/host/vcf_importer.cc, pinned by the goldens), in two independent ways:
  check 1  cells(BCF2 of X) == import_cells(X) for the original text X, encoded by tests/tools/vcf2bcf.py;
  check 2  cells(S) == import_cells(text of S) for the text the older, independent decoder tests/tools/bcf2text.py prints of S.
Host code only - no device."""
import ctypes
import json
import os
import re
import struct
import subprocess
import sys

import pytest

import helpers
from golden_cases import CASES

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bcf_inputs  # noqa: E402

INPUTS = os.path.join(helpers.GOLDEN, "inputs")
COLUMN_END = 2**63 - 2


def _is_2d(vid):
    fields = json.load(open(os.path.join(INPUTS, vid)))["fields"]
    fields = fields.values() if isinstance(fields, dict) else fields
    return any(isinstance(f.get("length"), list) or isinstance(f.get("type"), list) for f in fields)


PAIRS = sorted({(c[1], c[2]) for c in CASES if not _is_2d(c[2])})
HAND = ("import_hand.json", "vid_import_hand.json")
HAND_BCF = ("import_hand_bcf.json", "vid_import_hand_bcf.json")


@pytest.fixture(scope="module")
def gdb():
    from genomicsdb_amd import build as b
    b.build_native()
    import genomicsdb_amd
    return genomicsdb_amd


@pytest.fixture(scope="module")
def built():
    from genomicsdb_amd import build as b
    return b.build_hostsim_import_bcf()


@pytest.fixture(scope="module")
def sim(built):
    L = ctypes.CDLL(built[0])
    c = ctypes
    L.hsb_last_error.restype = c.c_char_p
    L.hsb_import.argtypes = [c.c_char_p, c.c_char_p, c.c_char_p, c.c_int, c.c_int64, c.c_int64, c.c_uint64, c.POINTER(c.c_void_p), c.POINTER(c.c_uint64), c.POINTER(c.c_int64)]
    L.hsb_free.argtypes = [c.c_void_p]
    return L


def _paths(callsets, vid):
    return os.path.join(INPUTS, vid), os.path.join(INPUTS, "callsets", callsets)


def sim_import(L, vid, callsets, root, treat=True, begin=0, end=COLUMN_END, budget=0):
    """-> (bytes, {files, records, cells, spanning, batches}); raises RuntimeError with the harness's message"""
    p, n = ctypes.c_void_p(), ctypes.c_uint64()
    st = (ctypes.c_int64 * 5)()
    rc = L.hsb_import(os.fsencode(vid), os.fsencode(callsets), os.fsencode(root), 1 if treat else 0, begin, end, budget, ctypes.byref(p), ctypes.byref(n), st)
    if rc != 0:
        raise RuntimeError(L.hsb_last_error().decode())
    try:
        return ctypes.string_at(p.value, n.value), dict(zip(("files", "records", "cells", "spanning", "batches"), st))
    finally:
        L.hsb_free(p)


def _both_checks(gdb, sim, v, c, root, tmp, treats=(True, False), decodable=True, **enc):
    """checks 1 and 2 for the mapping c over text files under root; -> (cells with deletions as intervals, encoder report)"""
    bc, streams, report = bcf_inputs.encode_mapping(v, c, root, str(tmp / "bcf"), **enc)
    tc = bcf_inputs.decode_mapping(bc, streams, str(tmp / "text")) if decodable else None
    first = None
    for treat in treats:
        want, ncells = gdb.import_cells(v, c, file_root=root, treat_deletions_as_intervals=treat)
        got, st = sim_import(sim, v, bc, str(tmp / "bcf"), treat)
        assert ncells > 0 and st["cells"] == ncells
        assert got == want, "check 1"
        if decodable:
            assert got == gdb.import_cells(v, tc, file_root=str(tmp / "text"), treat_deletions_as_intervals=treat)[0], "check 2"
        first = got if first is None else first
    return first, report


@pytest.mark.parametrize("callsets,vid", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_fixtures_as_bcf2(gdb, sim, tmp_path, callsets, vid):
    v, c = _paths(callsets, vid)
    got, _ = _both_checks(gdb, sim, v, c, helpers.GOLDEN, tmp_path)
    assert got == helpers.cells_for(callsets, vid)


def test_bgzf_bcf_files_are_read_too(gdb, sim, tmp_path):
    v, c = _paths("t0_1_2.json", "vid.json")
    bc, streams, _ = bcf_inputs.encode_mapping(v, c, helpers.GOLDEN, str(tmp_path / "bcf"), bgzf=True)
    assert open(tmp_path / "bcf" / "f0.bcf", "rb").read(4) == b"\x1f\x8b\x08\x04"
    assert sim_import(sim, v, bc, str(tmp_path / "bcf"), budget=256)[0] == helpers.cells_for("t0_1_2.json", "vid.json")


def test_hand_made_input_covers_every_vector_kind(gdb, sim, tmp_path):
    """import_hand.vcf has no int32 vector; import_hand_bcf.vcf is that file plus two records, one of which has"""
    v, c = _paths(*HAND)
    _, rep = _both_checks(gdb, sim, v, c, helpers.GOLDEN, tmp_path / "hand")
    assert rep["int32"] == 0
    v, c = _paths(*HAND_BCF)
    got, rep = _both_checks(gdb, sim, v, c, helpers.GOLDEN, tmp_path / "hand_bcf")
    for kind in ("int8", "int16", "int32", "float", "char", "flag", "missing_inside_longer_vector", "vector_end"):
        assert rep[kind] >= 1, kind
    # known answers: MLEAC=70000,1 among 2 samples (int32 vector, element-wise sum); PL 0,300,70000; GT '1' next to '0/1' (vector_end cut)
    assert struct.pack("<iii", 2, 35000, 1) in got and struct.pack("<iii", 2, 35000, 0) in got
    assert struct.pack("<iiii", 3, 0, 300, 70000) in got
    assert struct.pack("<iiii", 1, 2, 3, 400) in got and struct.pack("<i", 3) + b"xyz" in got


@pytest.mark.parametrize("budget", [256, 0])
def test_partition_cuts(gdb, sim, tmp_path, budget):
    v, c = _paths("t0_1_2.json", "vid.json")
    bc, _, _ = bcf_inputs.encode_mapping(v, c, helpers.GOLDEN, str(tmp_path / "a"))
    for begin, end in ((0, 12199), (12200, COLUMN_END)):
        want, ncells = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=begin, column_end=end)
        got, st = sim_import(sim, v, bc, str(tmp_path / "a"), True, begin, end, budget)
        assert got == want and st["cells"] == ncells
        if begin:
            assert st["spanning"] > 0
        if budget:
            assert st["batches"] > st["files"]
    v, c = _paths("t0_overlapping.json", "vid.json")
    bc, _, _ = bcf_inputs.encode_mapping(v, c, helpers.GOLDEN, str(tmp_path / "b"))
    want, _ = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=12202)
    assert sim_import(sim, v, bc, str(tmp_path / "b"), True, 12202, COLUMN_END, budget)[0] == want


def test_synthetic(gdb, sim, tmp_path):
    import synth_gvcf_text
    d = str(tmp_path / "synth")
    v, c = synth_gvcf_text.write_inputs(d, n_files=6, n_lines=2000, multi=3)
    _, rep = _both_checks(gdb, sim, v, c, d, tmp_path, treats=(True,))
    assert rep["float"] > 0 and rep["int16"] > 0 and rep["vector_end"] > 0


@pytest.mark.parametrize("enc", [{"idx": "none"}, {"idx": "shuffle", "seed": 3}, {"idx": "shuffle", "seed": 4}, {"idx": "none", "pass_line": False},
                                 {"idx": "keep", "pass_line": False}], ids=["no_idx", "shuffled_idx_3", "shuffled_idx_4", "no_idx_no_pass_line", "idx_no_pass_line"])
def test_dictionary_order(gdb, sim, tmp_path, enc):
    """ids by order of first appearance, by shuffled IDX= keys, and PASS = 0 without a PASS line (bcf2text refuses a header
    without a PASS line, so check 2 is left to the other headers)"""
    for pair in (HAND_BCF, ("t0_1_2.json", "vid.json")):
        v, c = _paths(*pair)
        _both_checks(gdb, sim, v, c, helpers.GOLDEN, tmp_path / pair[0], decodable=enc.get("pass_line", True), **enc)
    if enc["idx"] == "shuffle":
        hdr = open(tmp_path / HAND_BCF[0] / "bcf" / "f0.bcf", "rb").read()
        idx = [int(x) for x in re.findall(rb"##(?:FILTER|INFO|FORMAT)=<[^\n]*,IDX=(\d+)>", hdr)]
        assert idx != sorted(idx)


def _one_file(tmp_path, lines, vid_fields):
    d = tmp_path / "in"
    d.mkdir()
    (d / "a.vcf").write_text("\n".join(["##fileformat=VCFv4.2"] + lines) + "\n")
    vid = {"fields": vid_fields, "contigs": {"1": {"length": 1000000, "tiledb_column_offset": 0}}}
    (d / "vid.json").write_text(json.dumps(vid))
    (d / "callsets.json").write_text(json.dumps({"callsets": {"S": {"row_idx": 0, "idx_in_file": 0, "filename": "a.vcf"}}}))
    return str(d / "vid.json"), str(d / "callsets.json"), str(d)


FIELDS = {"PASS": {"type": "int"}, "END": {"vcf_field_class": ["INFO"], "type": "int"}, "MQ": {"vcf_field_class": ["INFO"], "type": "float"},
          "DP": {"vcf_field_class": ["INFO", "FORMAT"], "type": "int"}, "GT": {"vcf_field_class": ["FORMAT"], "type": "int", "length": "PP"}}
CHROM = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"


def test_integers_for_a_float_attribute_import(gdb, sim, tmp_path):
    v, c, root = _one_file(tmp_path, ['##INFO=<ID=MQ,Number=1,Type=Integer,Description="x">', CHROM, "1\t10\t.\tA\tC\t.\t.\tMQ=60;DP=3\tGT:DP\t0/1:300",
                                      "1\t20\t.\tA\tC\t.\t.\tMQ=-7\tGT\t1|1"], FIELDS)
    got, rep = _both_checks(gdb, sim, v, c, root, tmp_path)
    assert struct.pack("<f", 60.0) in got and struct.pack("<f", -7.0) in got and rep["float"] == 0


def test_floats_for_an_integer_attribute_are_refused_by_name(gdb, sim, tmp_path):
    v, c, root = _one_file(tmp_path, ['##INFO=<ID=DP,Number=1,Type=Float,Description="x">', CHROM, "1\t10\t.\tA\tC\t.\t.\tMQ=60\tGT\t0/1", "1\t20\t.\tA\tC\t.\t.\tDP=3.5\tGT\t1|1"],
                          FIELDS)
    bc, _, _ = bcf_inputs.encode_mapping(v, c, root, str(tmp_path / "bcf"))
    with pytest.raises(RuntimeError, match=r"field DP: the record holds float values, the vid mapping declares int .*f0\.bcf record 2"):
        sim_import(sim, v, bc, str(tmp_path / "bcf"))


def test_unknown_contig_and_filter_speak_like_the_text_importer(gdb, sim, tmp_path):
    fields = dict(FIELDS)
    v, c, root = _one_file(tmp_path, [CHROM, "1\t10\t.\tA\tC\t.\tPASS\tMQ=60\tGT\t0/1", "1\t20\t.\tA\tC\t.\tNoSuchFilter\tMQ=1\tGT\t1|1", "7\t5\t.\tA\tC\t.\t.\tMQ=1\tGT\t1|1"], fields)
    bc, _, _ = bcf_inputs.encode_mapping(v, c, root, str(tmp_path / "bcf"))
    with pytest.raises(RuntimeError, match=r"FILTER NoSuchFilter is not in the vid mapping .*f0\.bcf record 2"):
        sim_import(sim, v, bc, str(tmp_path / "bcf"))
    with pytest.raises(gdb.GenomicsDBException, match="FILTER NoSuchFilter is not in the vid mapping"):
        gdb.import_cells(v, c, file_root=root)


def test_two_dimensional_vid_is_refused_for_bcf2_too(gdb, sim, tmp_path):
    v, c = _paths("t0_1_2_all_asa.json", "vid_all_asa.json")
    bc, _, _ = bcf_inputs.encode_mapping(v, c, helpers.GOLDEN, str(tmp_path / "bcf"))
    with pytest.raises(RuntimeError, match=r"field \w+: .*not imported by the device importer"):
        sim_import(sim, v, bc, str(tmp_path / "bcf"))


def test_host_importer_names_the_bcf2_file(gdb, tmp_path):
    v, c = _paths("t0_1_2.json", "vid.json")
    for bgzf in (False, True):
        d = tmp_path / ("z" if bgzf else "u")
        bc, _, _ = bcf_inputs.encode_mapping(v, c, helpers.GOLDEN, str(d), bgzf=bgzf)
        with pytest.raises(gdb.GenomicsDBException, match=r"f0\.bcf is BCF2: BCF2 input needs the device importer"):
            gdb.import_cells(v, bc, file_root=str(d))
    with pytest.raises(ValueError, match="streams"):
        gdb.import_cells(v, c, file_root=helpers.GOLDEN, streams={"x": b""})


def test_broken_chain_names_file_record_and_offset(sim, tmp_path):
    v, c = _paths(*HAND_BCF)
    bc, streams, _ = bcf_inputs.encode_mapping(v, c, helpers.GOLDEN, str(tmp_path / "bcf"))
    data = streams["f0.bcf"]
    (tmp_path / "bcf" / "f0.bcf").write_bytes(data[:-5])
    with pytest.raises(RuntimeError, match=r"truncated BCF2 record: .*f0\.bcf record 6 at byte offset \d+"):
        sim_import(sim, v, bc, str(tmp_path / "bcf"))


def test_the_three_refusals_of_the_gpu_suite(sim, tmp_path):
    v, c = _paths(*HAND_BCF)
    bc, streams, _ = bcf_inputs.encode_mapping(v, c, helpers.GOLDEN, str(tmp_path / "bcf"))
    words = {"truncated": "truncated BCF2 record", "type_code": "type code", "dictionary_id": "dictionary or contig id"}
    for kind, (data, record) in bcf_inputs.hostile_streams(streams["f0.bcf"]).items():
        (tmp_path / "bcf" / "f0.bcf").write_bytes(data)
        with pytest.raises(RuntimeError, match=r"%s.*f0\.bcf record %d" % (words[kind], record)):
            sim_import(sim, v, bc, str(tmp_path / "bcf"), budget=256)


def test_malformed_input_under_the_sanitizers(built, tmp_path):
    """the stand-alone program (never loaded into Python): the valid hand-made stream and 2 000 seeded mutations of it; every case is
    refused with an error or yields cells, and a sanitizer report would end the program with a non-zero status"""
    v, c = _paths(*HAND_BCF)
    bc, streams, _ = bcf_inputs.encode_mapping(v, c, helpers.GOLDEN, str(tmp_path / "bcf"))
    hostile = []
    for kind, (data, _) in bcf_inputs.hostile_streams(streams["f0.bcf"]).items():       # the three inputs the GPU tests use
        (tmp_path / (kind + ".bcf")).write_bytes(data)
        hostile.append(str(tmp_path / (kind + ".bcf")))
    r = subprocess.run([built[1], v, bc, str(tmp_path / "bcf" / "f0.bcf"), "2000", "1"] + hostile, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    words = r.stdout.decode().split()
    counts = dict(zip(words[0::2], (int(x) for x in words[1::2])))
    assert counts.pop("hostile_refused") == 6
    assert counts["cases"] == 2000 and sum(v for k, v in counts.items() if k != "cases") == 2000
    assert counts.get("bounds", 0) > 0 and counts.get("type_code", 0) > 0 and counts.get("broken_chain", 0) > 0 and counts.get("imported", 0) > 0
