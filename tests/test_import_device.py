"""The device importer (csrc/kernels/gdb_import.hip; import_cells(..., device=0), vcf2tiledb --import-on-device) against the host
importer (csrc/host/vcf_importer.cc): the same bytes and counts on every fixture callset mapping without 2-dimensional fields, at
every text budget, on the hand-made VCF, on seeded synthetic gVCFs whole and as two partitions; loud errors that name file and line."""
import json
import os
import subprocess
import sys

import pytest

import helpers
from golden_cases import CASES

pytestmark = pytest.mark.gpu

INPUTS = os.path.join(helpers.GOLDEN, "inputs")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))


def _is_2d(vid):
    fields = json.load(open(os.path.join(INPUTS, vid)))["fields"]
    fields = fields.values() if isinstance(fields, dict) else fields        # (vid_as_array.json lists its fields)
    return any(isinstance(f.get("length"), list) or isinstance(f.get("type"), list) for f in fields)


PAIRS = sorted({(c[1], c[2]) for c in CASES if not _is_2d(c[2])})
HAND = ("import_hand.json", "vid_import_hand.json")
HAND_DEFERRED = 8       # counted by tests/test_import_bodies_cpu.py::test_hand_made_vcf


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


def _paths(callsets, vid):
    return os.path.join(INPUTS, vid), os.path.join(INPUTS, "callsets", callsets)


def _both(gdb, v, c, root, budget=0, **kw):
    want = gdb.import_cells(v, c, file_root=root, **kw)
    st = {}
    got = gdb.import_cells(v, c, file_root=root, device=0, text_budget_bytes=budget, stats=st, **kw)
    assert got[1] == want[1] and len(got[0]) == len(want[0])
    assert got[0] == want[0]
    assert st["num_cells"] == want[1] and st["num_bytes"] == len(want[0])
    return want, st


@pytest.mark.parametrize("budget", [256, 4096, 0], ids=["budget256", "budget4096", "default_budget"])
@pytest.mark.parametrize("callsets,vid", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_fixtures_on_the_device(gdb, callsets, vid, budget):
    v, c = _paths(callsets, vid)
    for treat in (True, False):
        want, st = _both(gdb, v, c, helpers.GOLDEN, budget, treat_deletions_as_intervals=treat)
        assert want[1] > 0 and st["num_deferred_values"] == 0
        if budget == 256:
            assert st["num_batches"] >= st["num_files"]
            if callsets == "t0_1_2.json":
                assert st["num_batches"] > st["num_files"]      # files are cut, and their lines are longer than 256 bytes
        if treat and budget == 0:
            assert want[0] == helpers.cells_for(callsets, vid)


@pytest.mark.parametrize("budget", [256, 0])
def test_fixture_partition_cut_on_the_device(gdb, budget):
    v, c = _paths("t0_1_2.json", "vid.json")
    _both(gdb, v, c, helpers.GOLDEN, budget, column_begin=0, column_end=12199)
    _, st = _both(gdb, v, c, helpers.GOLDEN, budget, column_begin=12200)
    assert st["num_spanning_cells"] > 0
    v, c = _paths("t0_overlapping.json", "vid.json")
    _both(gdb, v, c, helpers.GOLDEN, budget, column_begin=12202)


@pytest.mark.parametrize("stage_in_lds", ["0", "1"])
@pytest.mark.parametrize("budget", [256, 0])
def test_hand_made_vcf_on_the_device(gdb, budget, monkeypatch, stage_in_lds):
    monkeypatch.setenv("GDBAMD_IMPORT_STAGE_LDS", stage_in_lds)
    v, c = _paths(*HAND)
    for treat in (True, False):
        _, st = _both(gdb, v, c, helpers.GOLDEN, budget, treat_deletions_as_intervals=treat)
        assert st["num_deferred_values"] == HAND_DEFERRED and st["num_records"] == 4


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    import synth_gvcf_text
    d = str(tmp_path_factory.mktemp("synth_import"))
    v, c = synth_gvcf_text.write_inputs(d, n_files=6, n_lines=2000, multi=3)
    return d, v, c


@pytest.mark.parametrize("stage_in_lds", ["0", "1"], ids=["direct_stores", "cells_staged_in_lds"])
def test_synthetic_whole_and_two_partitions(gdb, synth, monkeypatch, stage_in_lds):
    monkeypatch.setenv("GDBAMD_IMPORT_STAGE_LDS", stage_in_lds)      # both variants of the write kernel (profiles/device_import.md)
    d, v, c = synth
    # 64 KiB batches: several per file, so sort ties and the partition-begin choice span batches
    want, st = _both(gdb, v, c, d, 65536)
    assert st["num_batches"] > 2 * st["num_files"] and st["num_deferred_values"] > 0 and want[1] >= 6 * 2000 + 3 * 2000
    _both(gdb, v, c, d, 0, treat_deletions_as_intervals=False)
    cut = 2500000           # inside contig "1", which the files write AFTER contig "2" (offset 5000000)
    lo, _ = _both(gdb, v, c, d, 65536, column_begin=0, column_end=cut - 1)
    hi, st_hi = _both(gdb, v, c, d, 65536, column_begin=cut)
    assert st_hi["num_spanning_cells"] > 0 and lo[1] + hi[1] == want[1] + st_hi["num_spanning_cells"]
    cut2 = 5000000 + 1234567
    _, st2 = _both(gdb, v, c, d, 0, column_begin=cut2)
    assert st2["num_spanning_cells"] > 0


def _broken(tmp_path, edit):
    """a small synthetic gVCF with `edit` applied to its lines -> (vid, callsets, root, path, index of the first record line)"""
    import synth_gvcf_text
    v, c = synth_gvcf_text.write_inputs(str(tmp_path), n_files=1, n_lines=120, multi=0, seed=5)
    p = tmp_path / "s0000.g.vcf"
    text = p.read_text().split("\n")
    first = next(i for i, l in enumerate(text) if l and not l.startswith("#"))
    p.write_text("\n".join(edit(text, first)))
    return v, c, str(tmp_path), str(p), first


def _set_col(line, k, value):
    cols = line.split("\t")
    cols[k] = value
    return "\t".join(cols)


@pytest.mark.parametrize("what,col,value,message", [("contig", 0, "chrUn_7", "contig chrUn_7 is not in the vid mapping"),
                                                     ("filter", 6, "PASS;NoSuchFilter", "FILTER NoSuchFilter is not in the vid mapping"),
                                                     ("short", None, None, "short record line")])
def test_errors_name_file_and_line(gdb, tmp_path, what, col, value, message):
    def edit(text, first):
        at = first + 40         # the line after it is broken too: the smaller line number must be reported
        for k in (at, at + 1):
            text[k] = "\t".join(text[k].split("\t")[:5]) if col is None else _set_col(text[k], col, value)
        return text
    v, c, root, path, first = _broken(tmp_path, edit)
    with pytest.raises(gdb.GenomicsDBException) as host:
        gdb.import_cells(v, c, file_root=root)
    assert message in str(host.value)
    for budget in (256, 0):
        with pytest.raises(gdb.GenomicsDBException) as e:
            gdb.import_cells(v, c, file_root=root, device=0, text_budget_bytes=budget)
        assert message in str(e.value) and path in str(e.value) and "line %d" % (first + 40 + 1) in str(e.value)


def test_bad_integer_is_deferred_then_thrown_by_the_host_parser(gdb, tmp_path):
    def edit(text, first):
        cols = text[first].split("\t")
        keys = cols[8].split(":")
        vals = cols[9].split(":")
        vals[keys.index("DP")] = "abc"
        cols[9] = ":".join(vals)
        text[first] = "\t".join(cols)
        return text
    v, c, root, path, first = _broken(tmp_path, edit)
    with pytest.raises(gdb.GenomicsDBException, match="not an integer: 'abc' in DP"):
        gdb.import_cells(v, c, file_root=root)
    with pytest.raises(gdb.GenomicsDBException, match="not an integer: 'abc' in DP") as e:
        gdb.import_cells(v, c, file_root=root, device=0)
    assert path in str(e.value) and "line %d" % (first + 1) in str(e.value)


def test_two_dimensional_vid_is_refused_before_any_launch(gdb):
    v, c = _paths("t0_1_2_all_asa.json", "vid_all_asa.json")
    assert gdb.import_cells(v, c, file_root=helpers.GOLDEN)[1] > 0
    with pytest.raises(gdb.GenomicsDBException, match=r"field \w+: .*not imported by the device importer"):
        gdb.import_cells(v, c, file_root=helpers.GOLDEN, device=0)


@pytest.mark.parametrize("case", ["t0_1_2_loading", "t0_overlapping_at_12202_partition_loading"])
def test_vcf2tiledb_import_on_device(gdb, tmp_path, case):
    name, callsets, vid, ov, golden, mode = [c for c in CASES if c[0] == case][0]
    tool = os.path.join(os.path.dirname(gdb.__file__), "vcf2tiledb")
    outs = {}
    for flag in ("host", "device"):
        ws = tmp_path / flag
        ws.mkdir()
        # the loader JSON of tests/test_gpu_parity.py::test_vcf2tiledb_cli_imports_and_combines_in_line, run from the fixture tree
        loader = {"row_based_partitioning": False, "produce_combined_vcf": True, "produce_tiledb_array": True,
                  "column_partitions": [{"begin": ov.get("partition_begin", 0), "workspace": str(ws), "array": "arr"}],
                  "callset_mapping_file": os.path.join("inputs", "callsets", callsets), "vid_mapping_file": os.path.join("inputs", vid),
                  "treat_deletions_as_intervals": True, "vcf_header_filename": os.path.join("inputs", "template_vcf_header.vcf"),
                  "reference_genome": os.path.join("inputs", "chr1_10MB.fasta.gz"), "num_parallel_vcf_files": 1, "do_ping_pong_buffering": False,
                  "size_per_column_partition": 3000, "offload_vcf_output_processing": False, "discard_vcf_index": True, "segment_size": 40}
        loader.update({k: x for k, x in ov.items() if k != "partition_begin"})
        lj = ws / "loader.json"
        lj.write_text(json.dumps(loader))
        r = subprocess.run([tool] + (["--import-on-device"] if flag == "device" else []) + [str(lj)], cwd=helpers.GOLDEN, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        timer = [l for l in r.stderr.decode().splitlines() if ",vcf2binary," in l][0]
        assert timer.endswith(",device,%d,deferred,0" % (1 if flag == "device" else 0))
        outs[flag] = (r.stdout, (ws / "arr" / "cells.bin").read_bytes())
    assert outs["device"][1] == outs["host"][1] and len(outs["host"][1]) > 0
    assert outs["device"][0] == outs["host"][0] == helpers.golden_text(golden)
