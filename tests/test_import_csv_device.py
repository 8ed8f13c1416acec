"""CSV cell files through the device importer (csrc/kernels/gdb_import.hip over ImpCsvSrc; import_cells(..., device=0),
vcf2tiledb --import-on-device): the checks of tests/test_import_csv_bodies_cpu.py on the device - the reference's own CSV file, the
round trip through tests/tools/cells2csv.py, the hand-made file with known answers, the errors, a mixed mapping - from files and
from streams= at the budgets 256 / 4096 / default, one synthetic shape, blocks of the write kernel beyond its LDS stage, and the
reference's own end-to-end case t0_1_2_csv (tests/run.py:367-395).  Expected bytes never come from the code under test."""
import json
import os
import subprocess

import pytest

import csv_inputs as ci
import helpers
from csv_inputs import cells2csv
from golden_cases import CALLS_CASES, CASES
from variants_cases import VARIANTS_CASES

pytestmark = pytest.mark.gpu

BUDGETS = pytest.mark.parametrize("budget", [256, 4096, 0], ids=["budget256", "budget4096", "default_budget"])


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


def dev_import(gdb, v, c, root, budget=0, **kw):
    st = {}
    cells, n = gdb.import_cells(v, c, file_root=root, device=0, text_budget_bytes=budget, stats=st, **kw)
    assert st["num_cells"] == n and st["num_bytes"] == len(cells)
    return cells, st


# ---- check 1 ---------------------------------------------------------------------------------------------------------------------
@BUDGETS
def test_reference_csv_file_gives_the_cells_of_the_vcfs(gdb, budget):
    v, text_mapping = ci.paths("t0_1_2.json", "vid.json")
    _, csv_mapping = ci.paths("t0_1_2_csv.json", "vid.json")
    want, ncells = gdb.import_cells(v, text_mapping, file_root=helpers.GOLDEN)
    raw = open(os.path.join(helpers.GOLDEN, "inputs", "callsets", "t0_1_2.csv"), "rb").read()
    for streams in (None, {"inputs/callsets/t0_1_2.csv": raw}):
        got, st = dev_import(gdb, v, csv_mapping, helpers.GOLDEN if streams is None else "/nonexistent", budget, streams=streams)
        assert got == want and got == helpers.cells_for("t0_1_2.json", "vid.json")
        assert st["num_cells"] == 5 and st["num_records"] == 5 and st["num_files"] == 1 and st["num_deferred_values"] == 0
        assert st["text_bytes"] == len(raw) and st["num_spanning_cells"] == 0
        assert (st["num_batches"] > 1) == (0 < budget < len(raw))
    text_cells, n_text = gdb.import_cells(v, text_mapping, file_root=helpers.GOLDEN, column_begin=12150)
    got, st = dev_import(gdb, v, csv_mapping, helpers.GOLDEN, budget, column_begin=12150)
    assert [ln.split(",")[1] for ln in cells2csv.cells_to_lines(got, v)] == ["17384"] * 3 and st["num_spanning_cells"] == 0
    assert n_text == 5 and text_cells.endswith(got) and len(text_cells) > len(got)


# ---- check 2 ---------------------------------------------------------------------------------------------------------------------
@BUDGETS
@pytest.mark.parametrize("callsets,vid", ci.PAIRS, ids=["%s-%s" % p for p in ci.PAIRS])
def test_round_trip_through_the_printer(gdb, tmp_path, callsets, vid, budget):
    v, c = ci.paths(callsets, vid)
    mapping = ci.csv_mapping(c, str(tmp_path))
    for treat in (True, False):
        cells, ncells = gdb.import_cells(v, c, file_root=helpers.GOLDEN, treat_deletions_as_intervals=treat)
        want, nans = ci.after_csv(cells, v)          # (info_ops.json: 3 NaN elements, see the CPU test's docstring)
        text = cells2csv.csv_text(cells, v, seed=11).encode("latin-1")
        (tmp_path / "cells.csv").write_bytes(text)
        got, st = dev_import(gdb, v, mapping, str(tmp_path), budget, treat_deletions_as_intervals=treat)
        assert got == want and st["num_cells"] == ncells and st["num_records"] == ncells and st["num_deferred_values"] == nans
        assert (st["num_batches"] > 1) == (0 < budget < len(text))
        got, _ = dev_import(gdb, v, mapping, "/nonexistent", budget, treat_deletions_as_intervals=treat, streams={"cells.csv": text})
        assert got == want


def test_every_line_ten_times_is_cut_at_both_budgets(gdb, tmp_path):
    v, c = ci.paths("t0_1_2_combined.json", "vid.json")
    cells, ncells = gdb.import_cells(v, c, file_root=helpers.GOLDEN)
    want = b"".join(x * 10 for x in ci.split_cells(cells))
    (tmp_path / "cells.csv").write_text(cells2csv.csv_text(cells, v, seed=3) * 10)
    mapping = ci.csv_mapping(c, str(tmp_path), key="sorted_csv_files")
    batches = []
    for budget in (0, 256, 4096):
        got, st = dev_import(gdb, v, mapping, str(tmp_path), budget)
        assert got == want and st["num_cells"] == 10 * ncells
        batches.append(st["num_batches"])
    assert batches[0] == 1 and batches[1] > batches[2] > 1


# ---- check 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage_in_lds", ["0", "1"], ids=["direct_stores", "cells_staged_in_lds"])
@pytest.mark.parametrize("budget", [0, 64])
def test_hand_made_file_with_known_answers(gdb, monkeypatch, budget, stage_in_lds):
    monkeypatch.setenv("GDBAMD_IMPORT_STAGE_LDS", stage_in_lds)
    v, c = ci.paths(*ci.HAND)
    raw = open(os.path.join(helpers.GOLDEN, "inputs", "callsets", "csv_hand.csv"), "rb").read()
    for begin, end in ((0, ci.COLUMN_END), ci.HAND_PARTITION):
        want, ncells = ci.hand_cells(begin, end)
        for streams in (None, {"inputs/callsets/csv_hand.csv": raw}):
            got, st = dev_import(gdb, v, c, helpers.GOLDEN, budget, column_begin=begin, column_end=end, streams=streams)
            assert got == want
            assert st["num_cells"] == ncells and st["num_records"] == ci.HAND_RECORDS and st["num_deferred_values"] == ci.HAND_DEFERRED
            assert st["num_spanning_cells"] == 0 and st["text_bytes"] == len(raw) and (st["num_batches"] > 1) == bool(budget)


# ---- check 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ci.LINE_ERRORS, ids=[c[0] for c in ci.LINE_ERRORS])
def test_line_errors_name_file_and_line(gdb, tmp_path, case):
    _, lines, words, line = case
    v, c, root = ci.write_case(str(tmp_path), lines)
    for budget in (0, 40):
        with pytest.raises(gdb.GenomicsDBException, match=words + r".*a\.csv line %d\)" % line):
            gdb.import_cells(v, c, file_root=root, device=0, text_budget_bytes=budget)


@pytest.mark.parametrize("case", ci.VID_REFUSALS, ids=[c[0] for c in ci.VID_REFUSALS])
def test_vids_the_csv_path_does_not_cover_are_refused_by_name(gdb, tmp_path, case):
    _, extra, words = case
    v, c, root = ci.write_case(str(tmp_path), [ci.GOOD], vid_fields=extra)
    with pytest.raises(gdb.GenomicsDBException, match=words):
        gdb.import_cells(v, c, file_root=root, device=0)


def test_id_vids_and_compressed_files_are_refused_by_name(gdb, tmp_path):
    import gzip
    for callsets, vid in ci.ID_PAIRS:
        v, c = ci.paths(callsets, vid)
        mapping = ci.csv_mapping(c, str(tmp_path / callsets))
        with pytest.raises(gdb.GenomicsDBException, match="field ID: a vid that declares ID is not imported from CSV cell files"):
            gdb.import_cells(v, mapping, file_root=str(tmp_path), device=0)
    data = gzip.compress((ci.GOOD + "\n").encode())
    v, c, root = ci.write_case(str(tmp_path / "gz"), None, raw=data)
    for streams in (None, {"a.csv": data}):
        with pytest.raises(gdb.GenomicsDBException, match=r"a\.csv is gzip or BGZF: compressed CSV cell files are not imported"):
            gdb.import_cells(v, c, file_root=root, device=0, streams=streams)


# ---- check 5 ---------------------------------------------------------------------------------------------------------------------
@BUDGETS
def test_mixed_mapping(gdb, tmp_path, budget):
    v, c = ci.paths("t0_1_2.json", "vid.json")
    want, ncells = gdb.import_cells(v, c, file_root=helpers.GOLDEN)
    lines = [ln for ln in cells2csv.cells_to_lines(want, v) if ln.split(",")[0] in ("0", "1")]
    mapping = ci.csv_mapping(c, str(tmp_path), name=str(tmp_path / "rows01.csv"), rows=(0, 1))
    (tmp_path / "rows01.csv").write_text("".join(ln + "\n" for ln in reversed(lines)))
    got, st = dev_import(gdb, v, mapping, helpers.GOLDEN, budget)
    assert got == want and st["num_cells"] == ncells and st["num_files"] == 2
    got, st = dev_import(gdb, v, mapping, helpers.GOLDEN, budget, column_begin=12150)
    assert [ln.split(",")[:2] for ln in cells2csv.cells_to_lines(got, v)] == [["0", "17384"], ["1", "17384"], ["2", "17384"]]
    assert gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=12150)[0].endswith(got)
    # the other way round: row 2 from CSV, the blocks of rows 0 and 1 (VCF) are replayed at the partition begin
    lines2 = [ln for ln in cells2csv.cells_to_lines(want, v) if ln.split(",")[0] == "2"]
    mapping = ci.csv_mapping(c, str(tmp_path / "b"), name=str(tmp_path / "row2.csv"), rows=(2,))
    (tmp_path / "row2.csv").write_text("".join(ln + "\n" for ln in lines2))
    got, st = dev_import(gdb, v, mapping, helpers.GOLDEN, budget, column_begin=12150)
    assert got == gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=12150)[0] and st["num_spanning_cells"] == 2


# ---- one synthetic shape, and blocks beyond the LDS stage -------------------------------------------------------------------------
def test_synthetic_8_samples_20kb(gdb, tmp_path):
    """cells of the generator genomicsdb_amd/synth (8 samples x 20 kb, about 1 600 cells) printed as CSV, lines shuffled, imported in
    batches of 16 KiB.  The generator makes cells, not VCF text, so the cells themselves are the expectation.  Its largest cell has
    185 bytes: no block of 256 lines reaches the write kernel's 64 KiB stage, at any budget or sample count - the test below does"""
    from genomicsdb_amd import synth
    B, L, N = 10_000_000, 20000, 8
    g = synth.Generator(N, B, L)
    cells, ncells = g.chunk_bytes(B + L)
    g.close()
    vp, cp = synth.write_metadata(str(tmp_path), N, os.path.join(ci.INPUTS, "vid.json"))
    mapping = ci.csv_mapping(cp, str(tmp_path))
    text = cells2csv.csv_text(cells, vp, seed=7).encode()
    (tmp_path / "cells.csv").write_bytes(text)
    got, st = dev_import(gdb, vp, mapping, str(tmp_path), 16384)
    assert got == cells and st["num_cells"] == ncells > 1000 and st["num_batches"] >= 3 and st["text_bytes"] == len(text)
    lo, _ = dev_import(gdb, vp, mapping, str(tmp_path), 16384, column_end=B + L // 2 - 1)
    hi, st_hi = dev_import(gdb, vp, mapping, str(tmp_path), 0, column_begin=B + L // 2)
    assert lo + hi == cells and st_hi["num_spanning_cells"] == 0


@pytest.mark.parametrize("stage_in_lds", ["0", "1"], ids=["direct_stores", "cells_staged_in_lds"])
def test_blocks_beyond_the_lds_stage(gdb, tmp_path, monkeypatch, stage_in_lds):
    """700 lines in one batch: in the first 512 the char attribute NM has 330 to 420 bytes, so both full blocks of 256 lines hold more
    than 64 KiB of cells, which k_imp_write stores directly; the last block (188 lines, NM of 100 to 190 bytes) is staged.  Known
    answers by struct.pack"""
    import struct
    monkeypatch.setenv("GDBAMD_IMPORT_STAGE_LDS", stage_in_lds)
    lines, cells = [], {}
    for k in range(700):
        nm = bytes(65 + (k + j) % 26 for j in range((100 if k >= 512 else 330) + k % 91))
        row, col = (0, 2)[k % 2], 1000 + (k * 37) % 500
        lines.append("%d,%d,%d,A,&,,0,%d,,0,%s,0,0,1,2,3,4" % (row, col, col, k, nm.decode()))
        body = (struct.pack("<q", col) + ci._s(b"A") + ci._s(b"&") + struct.pack("<I", ci.NULL_F) + ci._i(0) + ci._i(k) + struct.pack("<I", ci.NULL_F) + ci._i(0) + ci._s(nm)
                + ci._i(0) + ci._i(0) + ci._i(1, 2, 3, 4))
        cells.setdefault((col, row), []).append(ci._cell(row, col, body))
    sizes = [len(ln) for ln in lines]
    assert min(sum(sizes[b:b + 256]) for b in (0, 256)) > 65536 and sum(s + 60 for s in sizes[512:]) < 65536     # (a cell is its line plus < 60 bytes)
    want = b"".join(b"".join(cells[k]) for k in sorted(cells))
    v, c, root = ci.write_case(str(tmp_path), lines)
    got, st = dev_import(gdb, v, c, root, 0)
    assert got == want and st["num_cells"] == 700 and st["num_batches"] == 1
    got, st = dev_import(gdb, v, c, root, 100000)
    assert got == want and st["num_batches"] >= 3


# ---- end to end: the reference's own case t0_1_2_csv ------------------------------------------------------------------------------
def test_vcf2tiledb_loads_the_csv_mapping_and_the_array_answers_the_goldens(gdb, tmp_path):
    from test_print_calls import calls_query
    from test_query_variants import device_query_variants
    tool = os.path.join(os.path.dirname(gdb.__file__), "vcf2tiledb")
    ws = tmp_path / "ws"
    ws.mkdir()
    loader = {"row_based_partitioning": False, "produce_combined_vcf": True, "produce_tiledb_array": True,
              "column_partitions": [{"begin": 0, "workspace": str(ws), "array": "arr"}],
              "callset_mapping_file": os.path.join("inputs", "callsets", "t0_1_2_csv.json"), "vid_mapping_file": os.path.join("inputs", "vid.json"),
              "treat_deletions_as_intervals": True, "vcf_header_filename": os.path.join("inputs", "template_vcf_header.vcf"),
              "reference_genome": os.path.join("inputs", "chr1_10MB.fasta.gz"), "num_parallel_vcf_files": 1, "do_ping_pong_buffering": False,
              "size_per_column_partition": 3000, "offload_vcf_output_processing": False, "discard_vcf_index": True, "segment_size": 40}
    lj = tmp_path / "loader.json"
    lj.write_text(json.dumps(loader))
    r = subprocess.run([tool, str(lj)], cwd=helpers.GOLDEN, capture_output=True, timeout=120)
    assert r.returncode != 0 and b"t0_1_2.csv is a CSV cell file: CSV input needs the device importer" in r.stderr and not r.stdout
    r = subprocess.run([tool, "--import-on-device", str(lj)], cwd=helpers.GOLDEN, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == helpers.golden_text("t0_1_2_loading")
    cells = (ws / "arr" / "cells.bin").read_bytes()
    for name in ("t0_1_2_vcf_at_0", "t0_1_2_vcf_at_12150"):
        _, callsets, vid, ov, golden, mode = [c for c in CASES if c[0] == name][0]
        q, _ = helpers.query_json(callsets, vid, ov, mode)
        s = gdb.GenomicsDBQueryStream(query_json=q, cells=cells, buffer_capacity=1 << 16)
        got = b""
        while True:
            chunk = s.read(1 << 16)
            if not chunk:
                break
            got += chunk
        s.close()
        assert got == helpers.golden_text(golden), name
    _, callsets, vid, ranges, attributes = [c for c in CALLS_CASES if c[0] == "t0_1_2_calls_at_0"][0]
    eng = gdb.CombineEngine(calls_query(callsets, vid, ranges, attributes))
    eng.stage_cells(cells)
    try:
        assert eng.print_calls() == helpers.golden_text("t0_1_2_calls_at_0")
    finally:
        eng.close()
    _, callsets, vid, ranges, attributes = [c for c in VARIANTS_CASES if c[0] == "t0_1_2_variants_at_0"][0]
    assert device_query_variants(gdb, calls_query(callsets, vid, ranges, attributes), cells) == helpers.golden_text("t0_1_2_variants_at_0")
