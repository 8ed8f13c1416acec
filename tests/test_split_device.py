"""The device splitter (csrc/kernels/gdb_split.hip; split_files(...), vcf2tiledb --split-files) against the plain-Python model
tests/tools/split_model.py: every output inflates (Python gzip) to the model's bytes, is BGZF from its first byte to the EOF block
and has a .tbi that lists exactly its contigs - on the fixture sets, on a hand-made file, and on seeded synthetic gVCFs read as
plain text, gzip and BGZF at three text budgets.  Then the round trip through the device importer, and the command line."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import pytest

import helpers
import split_inputs as si
from split_inputs import split_model

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bgzf_write  # noqa: E402
import synth_gvcf_text  # noqa: E402
import tabix_reader  # noqa: E402

pytestmark = pytest.mark.gpu

SYNTH_BEGINS = [0, 1800000, 6801064]      # inside contig "1" and inside contig "2" (offset 5000000); a record of every file spans each cut


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return si.input_sets(tmp_path_factory.mktemp("split_sets"))


def check_output(path, want):
    buf = open(path, "rb").read()
    si.bgzf_members(buf)
    assert gzip.decompress(buf) == want, path
    idx = tabix_reader.Index(path + ".tbi")
    assert idx.kind == "tbi" and idx.names == si.contigs_in(want), path


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_device_split_equals_the_model(gdb, sets, tmp_path, name):
    vid, callsets, root, names, begins = sets[name]
    model, parts = si.model_of(vid, root, names, begins)
    si.assert_model_is_interesting(model, names, len(parts))
    st = {}
    out = gdb.split_files(vid, callsets, parts, results_directory=str(tmp_path), file_root=root, stats=st)
    assert sorted(out) == sorted(model)
    for key, path in out.items():
        assert path == os.path.join(str(tmp_path), "partition_%d_%s" % (key[1], os.path.basename(key[0])))
        check_output(path, model[key])
    assert sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(p) + ext for p in out.values() for ext in ("", ".tbi"))
    assert st["num_files"] == len(names) and st["text_bytes_out"] == sum(len(t) for t in model.values())
    assert st["num_lines_written"] == sum(sum(1 for ln in t.splitlines() if not ln.startswith(b"#")) for t in model.values())


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """-> {form: directory} of the same 2 + 1 synthetic files as plain text, gzip and BGZF (700-byte members: lines straddle them),
    the model of their split, the partitions"""
    base = tmp_path_factory.mktemp("split_synth")
    plain = str(base / "plain")
    vid, callsets = synth_gvcf_text.write_inputs(plain, n_files=2, n_lines=2000, multi=1)
    names = ["s0000.g.vcf", "s0001.g.vcf", "multi.vcf"]
    dirs = {"plain": plain}
    for form in ("gzip", "bgzf"):
        d = str(base / form)
        os.makedirs(d)
        for fn in names:
            data = open(os.path.join(plain, fn), "rb").read()
            if form == "gzip":
                with gzip.open(os.path.join(d, fn), "wb", compresslevel=1) as f:
                    f.write(data)
            else:
                bgzf_write.write_file(os.path.join(d, fn), data, member_size=700, level=1)
        shutil.copy(vid, d)
        shutil.copy(callsets, d)
        dirs[form] = d
    model, parts = si.model_of(vid, plain, names, SYNTH_BEGINS)
    offsets = split_model.contig_offsets(vid)
    for part in parts:
        for fn in names:
            assert split_model.round_trip_precondition(split_model.read_text(os.path.join(plain, fn)), offsets, part), (fn, part)
    return dirs, names, model, parts


@pytest.mark.parametrize("budget", [256, 65536, 0], ids=["budget256", "budget65536", "default_budget"])
@pytest.mark.parametrize("form", ["plain", "gzip", "bgzf"])
def test_synthetic_input_in_every_form_and_budget(gdb, synth, tmp_path, form, budget):
    dirs, names, model, parts = synth
    d = dirs[form]
    st = {}
    out = gdb.split_files(os.path.join(d, "vid.json"), os.path.join(d, "callsets.json"), parts, results_directory=str(tmp_path), file_root=d, text_budget_bytes=budget, stats=st)
    assert sorted(out) == sorted(model)
    for key, path in out.items():
        check_output(path, model[key])
    assert st["num_files"] == 3 and st["num_record_lines"] == 6000
    assert (st["ms_inflate"] > 0) == (form == "bgzf")
    if budget == 256:
        assert st["num_batches"] > st["num_files"]
    # index and classify run once per batch, whatever is produced: the same batches for 1 and for 3 partitions, fewer lines written
    one = {}
    os.makedirs(str(tmp_path / "one"))
    out1 = gdb.split_files(os.path.join(d, "vid.json"), os.path.join(d, "callsets.json"), parts, results_directory=str(tmp_path / "one"), file_root=d, produce=1,
                           text_budget_bytes=budget, stats=one)
    assert sorted(out1) == [(fn, 1) for fn in sorted(names)]
    for key, path in out1.items():
        check_output(path, model[key])
    assert one["num_batches"] == st["num_batches"] and one["num_record_lines"] == st["num_record_lines"]
    assert 0 < one["num_lines_written"] < st["num_lines_written"]


@pytest.mark.parametrize("p", [0, 1, 2])
def test_device_round_trip(gdb, synth, tmp_path, p):
    dirs, names, model, parts = synth
    d = dirs["bgzf"]
    vid, callsets = os.path.join(d, "vid.json"), os.path.join(d, "callsets.json")
    out = gdb.split_files(vid, callsets, parts, results_directory=str(tmp_path), file_root=d, produce=p)
    cs = json.load(open(callsets))
    for v in cs["callsets"].values():
        v["filename"] = out[(v["filename"], p)]
    cp = str(tmp_path / "callsets_split.json")
    json.dump(cs, open(cp, "w"))
    want = gdb.import_cells(vid, callsets, file_root=d, device=0, column_begin=parts[p][0], column_end=parts[p][1])
    got = gdb.import_cells(vid, cp, device=0, column_begin=parts[p][0], column_end=parts[p][1])
    assert want[1] > 0 and got[1] == want[1] and got[0] == want[0]


def _tool(gdb):
    return os.path.join(os.path.dirname(gdb.__file__), "vcf2tiledb")


def _loader(ws, callsets, begins):
    return {"row_based_partitioning": False, "produce_tiledb_array": True, "treat_deletions_as_intervals": True,
            "column_partitions": [{"begin": b, "workspace": str(ws), "array": "arr%d" % i} for i, b in enumerate(begins)],
            "callset_mapping_file": callsets, "vid_mapping_file": os.path.join("inputs", "vid.json")}


def test_command_line_splits_and_the_split_files_import_alike(gdb, sets, tmp_path):
    vid, callsets, root, names, begins = sets["a"]
    model, parts = si.model_of(vid, root, names, begins)
    res = tmp_path / "res"
    res.mkdir()
    lj = tmp_path / "loader.json"
    lj.write_text(json.dumps(_loader(tmp_path / "ws_orig", os.path.join("inputs", "callsets", "t0_1_2.json"), begins)))
    r = subprocess.run([_tool(gdb), "--split-files", "--split-all-partitions", "--split-callset-mapping-file", "--split-files-results-directory", str(res), str(lj)],
                       cwd=helpers.GOLDEN, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    timer = [ln for ln in r.stderr.decode().splitlines() if ",split_files," in ln]
    assert len(timer) == 1 and ",files,3," in timer[0] and ",batches," in timer[0]
    for fn in names:
        for p in range(3):
            check_output(str(res / ("partition_%d_%s" % (p, os.path.basename(fn)))), model[(fn, p)])
    # the written JSONs: per partition the callsets with row, index in the file and the split file; one loader JSON that lists them
    original = json.load(open(callsets))["callsets"]
    for p in range(3):
        cs = json.load(open(str(res / ("partition_%d_t0_1_2.json" % p))))
        assert sorted(cs) == ["callsets"] and sorted(cs["callsets"]) == sorted(original)
        for name, v in cs["callsets"].items():
            assert v == {"row_idx": original[name]["row_idx"], "idx_in_file": original[name]["idx_in_file"],
                         "filename": str(res / ("partition_%d_%s" % (p, os.path.basename(original[name]["filename"]))))}
    split_loader = res / "partition_0_loader.json"
    written = json.load(open(str(split_loader)))
    want_loader = json.loads(lj.read_text())
    assert written.pop("callset_mapping_file") == [str(res / ("partition_%d_t0_1_2.json" % p)) for p in range(3)]
    want_loader.pop("callset_mapping_file")
    assert written == want_loader
    # importing partition p with the written loader JSON gives the array file of importing it from the originals (same workspace: read in between)
    sizes = []
    for p in range(3):
        cells = []
        for loader in (lj, split_loader):
            r = subprocess.run([_tool(gdb), "--import-on-device", "-r", str(p), str(loader)], cwd=helpers.GOLDEN, capture_output=True, timeout=120)
            assert r.returncode == 0, r.stderr.decode()
            array_file = tmp_path / "ws_orig" / ("arr%d" % p) / "cells.bin"
            cells.append(array_file.read_bytes())
            array_file.unlink()
        assert cells[0] == cells[1], p
        sizes.append(len(cells[0]))
    assert sizes[0] > 0 and sizes[1] > 0      # (no record of t0, t1, t2 reaches 17385: partition 2 is empty on both sides)


def test_command_line_one_partition_refusals_and_failures(gdb, sets, tmp_path):
    vid, callsets, root, names, begins = sets["a"]
    model, parts = si.model_of(vid, root, names, begins)
    tool = _tool(gdb)
    res = tmp_path / "res"
    res.mkdir()
    lj = tmp_path / "loader.json"
    lj.write_text(json.dumps(_loader(tmp_path / "ws", os.path.join("inputs", "callsets", "t0_1_2.json"), begins)))
    r = subprocess.run([tool, "--split-files", "-r", "1", "--split-files-results-directory", str(res), str(lj)], cwd=helpers.GOLDEN, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert sorted(os.listdir(str(res))) == sorted("partition_1_%s%s" % (os.path.basename(fn), ext) for fn in names for ext in ("", ".tbi"))
    for fn in names:
        check_output(str(res / ("partition_1_%s" % os.path.basename(fn))), model[(fn, 1)])
    # a BCF2 input and a CSV input are refused by name, a failing input leaves no output: nothing is written in any of the three runs
    hand = tmp_path / "hand"
    v, c, hroot, _ = si.write_hand(str(hand))
    bad_lines = list(si.HAND_LINES)
    bad_lines[8] = bad_lines[8].replace("1\t995", "chrUn\t995")       # physical line 9
    cases = {}
    bcf = hand / "in.bcf"
    bcf.write_bytes(gzip.compress(b"BCF\x02\x02" + b"\x00" * 64))
    cases["bcf"] = ({"callsets": {"HA": {"row_idx": 0, "idx_in_file": 0, "filename": str(bcf)}}}, "in.bcf is BCF2")
    csv = hand / "cells.csv"
    csv.write_text("0,100,200\n")
    cases["csv"] = ({"callsets": {"HA": {"row_idx": 0, "idx_in_file": 0, "filename": str(csv)}}, "sorted_csv_files": [str(csv)]}, "cells.csv is a CSV cell file")
    bad = hand / "bad.vcf"
    bad.write_bytes("\n".join(bad_lines).encode())
    cases["line"] = ({"callsets": {"HA": {"row_idx": 0, "idx_in_file": 0, "filename": str(bad)}}}, "contig chrUn is not in the vid mapping (%s line 9)" % bad)
    for name, (cs, words) in cases.items():
        out = tmp_path / ("out_" + name)
        out.mkdir()
        cp = hand / (name + "_callsets.json")
        cp.write_text(json.dumps(cs))
        loader = _loader(tmp_path / "ws", str(cp), si.HAND_BEGINS)
        loader["vid_mapping_file"] = v
        lj = hand / (name + "_loader.json")
        lj.write_text(json.dumps(loader))
        r = subprocess.run([tool, "--split-files", "--split-all-partitions", "--split-files-results-directory", str(out), str(lj)], capture_output=True, timeout=120)
        assert r.returncode != 0 and words in r.stderr.decode(), (name, r.stderr.decode())
        assert os.listdir(str(out)) == [], name
    with pytest.raises(gdb.GenomicsDBException, match="chrUn"):
        gdb.split_files(v, str(hand / "line_callsets.json"), split_model.derive_partitions(si.HAND_BEGINS, si.LAST_END), results_directory=str(tmp_path / "out_line"))
    assert os.listdir(str(tmp_path / "out_line")) == []
