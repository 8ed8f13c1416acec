"""BCF2 input of the device importer (csrc/kernels/gdb_import.hip over csrc/core/gdb_import_bcf.hpp): .bcf files - plain and
BGZF - and in-memory streams through import_cells(..., device=0[, streams=...]) and vcf2tiledb --import-on-device.  The expected
cells are the host TEXT importer's, in the two independent ways of tests/test_import_bcf_bodies_cpu.py: check 1 against the
original text, check 2 against the text tests/tools/bcf2text.py prints of the stream."""
import json
import os
import subprocess
import sys

import pytest

import helpers
from golden_cases import CASES

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bcf_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

INPUTS = os.path.join(helpers.GOLDEN, "inputs")


def _is_2d(vid):
    fields = json.load(open(os.path.join(INPUTS, vid)))["fields"]
    fields = fields.values() if isinstance(fields, dict) else fields
    return any(isinstance(f.get("length"), list) or isinstance(f.get("type"), list) for f in fields)


PAIRS = sorted({(c[1], c[2]) for c in CASES if not _is_2d(c[2])}) + [("import_hand.json", "vid_import_hand.json"), ("import_hand_bcf.json", "vid_import_hand_bcf.json")]


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


def _paths(callsets, vid):
    return os.path.join(INPUTS, vid), os.path.join(INPUTS, "callsets", callsets)


class Encoded:
    """a mapping of text files as plain BCF2 files, as BGZF .bcf files and as streams, with the expected cells (host text importer,
    computed once): want[treat] from the original text (check 1), want2[treat] from the decoder's text of the streams (check 2)"""

    def __init__(self, gdb, v, c, root, d):
        self.v = v
        self.plain_root, self.bgzf_root = os.path.join(d, "plain"), os.path.join(d, "bgzf")
        self.callsets, self.streams, self.report = bcf_inputs.encode_mapping(v, c, root, self.plain_root)
        bcf_inputs.encode_mapping(v, c, root, self.bgzf_root, bgzf=True)
        tc = bcf_inputs.decode_mapping(self.callsets, self.streams, os.path.join(d, "text"))
        self.want = {t: gdb.import_cells(v, c, file_root=root, treat_deletions_as_intervals=t) for t in (True, False)}
        self.want2 = {t: gdb.import_cells(v, tc, file_root=os.path.join(d, "text"), treat_deletions_as_intervals=t) for t in (True, False)}
        assert self.want == self.want2, "the text importer on the original text and on the decoder's text of the BCF2 streams"

    def run(self, gdb, form, budget=0, treat=True, **kw):
        st = {}
        if form == "streams":
            got = gdb.import_cells(self.v, self.callsets, file_root="/nonexistent", device=0, text_budget_bytes=budget, stats=st, streams=self.streams,
                                   treat_deletions_as_intervals=treat, **kw)
        else:
            got = gdb.import_cells(self.v, self.callsets, file_root=self.plain_root if form == "plain" else self.bgzf_root, device=0, text_budget_bytes=budget,
                                   stats=st, treat_deletions_as_intervals=treat, **kw)
        return got, st


_encoded = {}


@pytest.fixture(scope="module")
def encoded(gdb, tmp_path_factory):
    def get(callsets, vid):
        if (callsets, vid) not in _encoded:
            v, c = _paths(callsets, vid)
            _encoded[(callsets, vid)] = Encoded(gdb, v, c, helpers.GOLDEN, str(tmp_path_factory.mktemp("bcf")))
        return _encoded[(callsets, vid)]
    return get


@pytest.mark.parametrize("budget", [256, 4096, 0], ids=["budget256", "budget4096", "default_budget"])
@pytest.mark.parametrize("callsets,vid", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_bcf2_inputs_on_the_device(gdb, encoded, callsets, vid, budget):
    e = encoded(callsets, vid)
    for form in ("plain", "bgzf", "streams"):
        for treat in (True, False):
            got, st = e.run(gdb, form, budget, treat)
            assert got == e.want[treat] and got == e.want2[treat], (form, treat)
            record_bytes = sum(len(x) - (9 + int.from_bytes(x[5:9], "little")) for x in e.streams.values())
            assert st["num_cells"] == got[1] > 0 and st["num_deferred_values"] == 0 and st["text_bytes"] == record_bytes
            if budget == 256 and callsets == "t0_1_2.json":
                assert st["num_batches"] > st["num_files"]
            if form != "streams":
                assert st["num_host_inflated_files"] == st["num_files"]
    if callsets.startswith("import_hand_bcf"):
        for kind in ("int8", "int16", "int32", "float", "char", "flag", "missing_inside_longer_vector", "vector_end"):
            assert e.report[kind] >= 1, kind


@pytest.mark.parametrize("budget", [256, 0])
def test_partition_cuts_on_the_device(gdb, encoded, budget):
    v, c = _paths("t0_1_2.json", "vid.json")
    e = encoded("t0_1_2.json", "vid.json")
    for begin, end in ((0, 12199), (12200, 2**63 - 2)):
        want = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=begin, column_end=end)
        for form in ("plain", "streams"):
            got, st = e.run(gdb, form, budget, column_begin=begin, column_end=end)
            assert got == want
            assert st["num_spanning_cells"] > 0 or not begin
    v, c = _paths("t0_overlapping.json", "vid.json")
    e = encoded("t0_overlapping.json", "vid.json")
    assert e.run(gdb, "bgzf", budget, column_begin=12202)[0] == gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=12202)


@pytest.fixture(scope="module")
def synth(gdb, tmp_path_factory):
    import synth_gvcf_text
    d = str(tmp_path_factory.mktemp("synth_bcf"))
    v, c = synth_gvcf_text.write_inputs(os.path.join(d, "in"), n_files=6, n_lines=2000, multi=3)
    return Encoded(gdb, v, c, os.path.join(d, "in"), d)


@pytest.mark.parametrize("form", ["plain", "bgzf", "streams"])
def test_synthetic_on_the_device(gdb, synth, form):
    for budget in (4096, 65536, 0):
        got, st = synth.run(gdb, form, budget)
        assert got == synth.want[True] and st["num_deferred_values"] == 0 and st["num_records"] == 7 * 2000
    assert st["num_batches"] == st["num_files"] == 7
    cut = 2500000
    v, c = synth.v, os.path.join(os.path.dirname(synth.v), "callsets.json")
    want = gdb.import_cells(v, c, file_root=os.path.dirname(v), column_begin=cut)
    got, st = synth.run(gdb, form, 65536, column_begin=cut)
    assert got == want and st["num_spanning_cells"] > 0


def test_mixed_mapping(gdb, encoded, tmp_path):
    """one file as .vcf.gz, one as .bcf, one as a stream"""
    v, c = _paths("t0_1_2.json", "vid.json")
    e = encoded("t0_1_2.json", "vid.json")
    cs = json.load(open(c))
    entries = list(cs["callsets"].values()) if isinstance(cs["callsets"], dict) else cs["callsets"]
    files = []
    for x in entries:
        if x["filename"] not in files:
            files.append(x["filename"])
    assert len(files) == 3 and files[0].endswith(".vcf.gz")
    rename = {files[0]: os.path.join(helpers.GOLDEN, files[0]), files[1]: os.path.join(e.bgzf_root, "f1.bcf"), files[2]: "the_third_file"}
    for x in entries:
        x["filename"] = rename[x["filename"]]
    (tmp_path / "callsets.json").write_text(json.dumps(cs))
    st = {}
    got = gdb.import_cells(v, str(tmp_path / "callsets.json"), device=0, stats=st, streams={"the_third_file": e.streams["f2.bcf"]})
    assert got == e.want[True] and st["num_files"] == 3 and st["num_deferred_values"] == 0 and st["num_device_members"] > 0
    with pytest.raises(gdb.GenomicsDBException, match="stream no_such_file is not a .filename. of the callset mapping"):
        gdb.import_cells(v, str(tmp_path / "callsets.json"), device=0, streams={"the_third_file": e.streams["f2.bcf"], "no_such_file": b""})
    # VCF text through a stream, plain and gzip
    import gzip
    text = gzip.decompress(open(os.path.join(helpers.GOLDEN, files[2]), "rb").read())
    for data in (text, gzip.compress(text), open(os.path.join(helpers.GOLDEN, files[2]), "rb").read()):
        assert gdb.import_cells(v, str(tmp_path / "callsets.json"), device=0, streams={"the_third_file": data}) == e.want[True]


@pytest.mark.parametrize("keep_idx", [True, False], ids=["idx_kept", "idx_dropped"])
def test_bu_round_trip(gdb, tmp_path, keep_idx):
    """check 2 on a stream the new encoder never touched: the device's own "bu" output of the t0_1_2_vcf_at_0 combine, imported as
    a three-sample file"""
    name, callsets, vid, ov, golden, mode = [c for c in CASES if c[0] == "t0_1_2_vcf_at_0"][0]
    q, _ = helpers.query_json(callsets, vid, ov, mode)
    s = gdb.GenomicsDBQueryStream(query_json=q, cells=helpers.cells_for(callsets, vid), buffer_capacity=1 << 20, is_bcf=True, keep_idx_fields_in_bcf_header=keep_idx)
    stream = s.read()
    s.close()
    assert stream[:5] == b"BCF\x02\x02" and (b",IDX=" in stream) == keep_idx
    import bcf2text
    samples = bcf2text.parse_stream(stream)[0].samples
    assert len(samples) == 3
    cs = {"callsets": {nm: {"row_idx": k, "idx_in_file": k, "filename": "combined.bcf"} for k, nm in enumerate(samples)}}
    (tmp_path / "callsets.json").write_text(json.dumps(cs))
    tc = bcf_inputs.decode_mapping(str(tmp_path / "callsets.json"), {"combined.bcf": stream}, str(tmp_path / "text"))
    v = os.path.join(INPUTS, vid)
    want = gdb.import_cells(v, tc, file_root=str(tmp_path / "text"))
    assert want[1] > 0
    for budget in (256, 0):
        st = {}
        assert gdb.import_cells(v, str(tmp_path / "callsets.json"), device=0, text_budget_bytes=budget, stats=st, streams={"combined.bcf": stream}) == want
        assert st["num_deferred_values"] == 0


def test_refusals_name_file_and_record(gdb, encoded):
    """the three malformed inputs that tests/test_import_bcf_bodies_cpu.py shows to be refused cleanly on the CPU, under the sanitizers"""
    e = encoded("import_hand_bcf.json", "vid_import_hand_bcf.json")
    words = {"truncated": "truncated BCF2 record", "type_code": "type code", "dictionary_id": "dictionary or contig id"}
    for kind, (data, record) in bcf_inputs.hostile_streams(e.streams["f0.bcf"]).items():
        for budget in (256, 0):
            with pytest.raises(gdb.GenomicsDBException) as x:
                gdb.import_cells(e.v, e.callsets, device=0, text_budget_bytes=budget, streams={"f0.bcf": data})
            assert words[kind] in str(x.value) and "f0.bcf record %d" % record in str(x.value), kind


def test_inflate_device_refuses_bcf2(gdb, encoded):
    e = encoded("t0_1_2.json", "vid.json")
    for root in (e.bgzf_root, e.plain_root):
        with pytest.raises(gdb.GenomicsDBException, match=r"f0\.bcf is BCF2: BCF2 input is inflated on the host in this build"):
            gdb.import_cells(e.v, e.callsets, file_root=root, device=0, inflate="device")
    assert e.run(gdb, "bgzf", inflate="host")[0] == e.want[True]


def test_two_dimensional_vid_is_refused_for_bcf2_too(gdb, tmp_path):
    v, c = _paths("t0_1_2_all_asa.json", "vid_all_asa.json")
    bc, _, _ = bcf_inputs.encode_mapping(v, c, helpers.GOLDEN, str(tmp_path / "bcf"))
    with pytest.raises(gdb.GenomicsDBException, match=r"field \w+: .*not imported by the device importer"):
        gdb.import_cells(v, bc, file_root=str(tmp_path / "bcf"), device=0)


def test_vcf2tiledb_imports_bcf_files_on_the_device(gdb, encoded, tmp_path):
    name, callsets, vid, ov, golden, mode = [c for c in CASES if c[0] == "t0_1_2_loading"][0]
    e = encoded(callsets, vid)
    tool = os.path.join(os.path.dirname(gdb.__file__), "vcf2tiledb")
    outs = {}
    for flag, cs, args in (("host_text", os.path.join(INPUTS, "callsets", callsets), []), ("device_bcf", os.path.join(e.bgzf_root, "callsets.json"), ["--import-on-device"]),
                           ("host_bcf", os.path.join(e.bgzf_root, "callsets.json"), [])):
        ws = tmp_path / flag
        ws.mkdir()
        # a tree with the fixture's inputs/ and the three .bcf files next to it, so that relative file names resolve from the tool's directory
        for f in ("f0.bcf", "f1.bcf", "f2.bcf"):
            os.symlink(os.path.join(e.bgzf_root, f), ws / f)
        os.symlink(INPUTS, ws / "inputs")
        loader = {"row_based_partitioning": False, "produce_combined_vcf": True, "produce_tiledb_array": True,
                  "column_partitions": [{"begin": 0, "workspace": str(ws), "array": "arr"}],
                  "callset_mapping_file": cs, "vid_mapping_file": os.path.join("inputs", vid),
                  "treat_deletions_as_intervals": True, "vcf_header_filename": os.path.join("inputs", "template_vcf_header.vcf"),
                  "reference_genome": os.path.join("inputs", "chr1_10MB.fasta.gz"), "num_parallel_vcf_files": 1, "do_ping_pong_buffering": False,
                  "size_per_column_partition": 3000, "offload_vcf_output_processing": False, "discard_vcf_index": True, "segment_size": 40}
        lj = ws / "loader.json"
        lj.write_text(json.dumps(loader))
        r = subprocess.run([tool] + args + [str(lj)], cwd=str(ws), capture_output=True, timeout=120)
        if flag == "host_bcf":
            assert r.returncode != 0 and b"f0.bcf is BCF2: BCF2 input needs the device importer" in r.stderr
            continue
        assert r.returncode == 0, r.stderr.decode()
        outs[flag] = (r.stdout, (ws / "arr" / "cells.bin").read_bytes())
    assert outs["device_bcf"][1] == outs["host_text"][1] and len(outs["host_text"][1]) > 0
    assert outs["device_bcf"][0] == outs["host_text"][0] == helpers.golden_text(golden)
