"""Incremental import on the device: merge_cells (csrc/kernels/gdb_merge.hip) and the row bounds of import_cells(device=0).
The expected bytes never come from the code under test alone: for imported cells the yardstick is the WHOLE import of the mapping by
the host importer (held to the reference's goldens by tests/test_importer_cpu.py), for crafted opaque streams a Python
sorted(..., key=(col, row)) over the cells split by their size field (tests/merge_inputs.py)."""
import json
import os
import subprocess
import sys

import pytest

import helpers
import merge_inputs as mi
from golden_cases import CASES

pytestmark = pytest.mark.gpu

INPUTS = os.path.join(helpers.GOLDEN, "inputs")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
MAPPINGS = [("t0_1_2.json", 3), ("t6_7_8.json", 3), ("t0_overlapping.json", 1), ("t0_1_2_combined.json", 3)]      # (mapping, rows); vid.json, no 2-D fields
MAX = 2**63 - 2
MIXED = (0, 1, 15, 16, 17, 63, 64, 65)


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


@pytest.fixture(scope="module")
def tile(gdb):
    st = {}
    gdb.merge_cells([mi.cell(0, 0, b"")], stats=st)
    assert st["tile"] == 1024 and st["num_streams"] == 1 and st["cells_in"] == st["cells_out"] == 1 and st["bytes_out"] == 24
    return st["tile"]


def _paths(callsets, vid="vid.json"):
    return os.path.join(INPUTS, vid), os.path.join(INPUTS, "callsets", callsets)


def _merged(gdb, streams):
    st = {}
    got, n = gdb.merge_cells(streams, stats=st)
    assert st["cells_out"] == n == st["cells_in"] and st["bytes_out"] == len(got) == sum(len(s) for s in streams) and st["num_streams"] == len(streams)
    return got


# ---- fixture mappings at every split row ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("column_begin", [0, 12200])
@pytest.mark.parametrize("callsets,n_rows", MAPPINGS, ids=[m[0] for m in MAPPINGS])
def test_fixture_mappings_at_every_split_row(gdb, callsets, n_rows, column_begin):
    v, c = _paths(callsets)
    whole, n_whole = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=column_begin)
    assert n_whole > 0
    if column_begin == 0:
        assert whole == helpers.cells_for(callsets, "vid.json")
    makers = [dict(), dict(device=0, text_budget_bytes=256), dict(device=0)]
    for k in range(n_rows + 1):
        for kw in makers:
            lo = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=column_begin, ub_callset_row_idx=k - 1, **kw)[0] if k else b""
            hi = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=column_begin, lb_callset_row_idx=k, **kw)[0]
            assert lo == mi.rows_between(whole, 0, k - 1) and hi == mi.rows_between(whole, k, MAX), (k, kw)
            assert _merged(gdb, [lo, hi]) == whole, (k, kw)
            assert _merged(gdb, [hi, lo]) == whole, (k, kw)


# ---- synthetic input: three row ranges, and one multi-sample file split across two batches ---------------------------------------
@pytest.fixture(scope="module")
def synth(gdb, tmp_path_factory):
    import synth_gvcf_text
    d = str(tmp_path_factory.mktemp("synth_merge"))
    v, c = synth_gvcf_text.write_inputs(d, n_files=6, n_lines=2000, multi=3)
    whole, n = gdb.import_cells(v, c, file_root=d)
    rows = sorted(e["row_idx"] for e in json.load(open(c))["callsets"].values())
    return d, v, c, whole, n, rows


def test_synthetic_three_streams(gdb, synth, tile):
    d, v, c, whole, n, rows = synth
    assert rows == list(range(len(rows))) and len(rows) >= 8 and n > 4 * tile
    parts = []
    for lo, hi in ((0, 2), (3, 5), (6, MAX)):
        host = gdb.import_cells(v, c, file_root=d, lb_callset_row_idx=lo, ub_callset_row_idx=hi)[0]
        dev = gdb.import_cells(v, c, file_root=d, device=0, text_budget_bytes=65536, lb_callset_row_idx=lo, ub_callset_row_idx=hi)[0]
        assert host == dev == mi.rows_between(whole, lo, hi) and len(host) > 0
        parts.append(dev)
    assert _merged(gdb, parts) == whole
    assert _merged(gdb, parts[::-1]) == whole
    assert _merged(gdb, [parts[1], parts[2], parts[0]]) == whole


def test_synthetic_multi_sample_file_split_across_two_batches(gdb, synth):
    d, v, c, whole, n, rows = synth
    cut = rows[-2]          # the multi-sample file holds the last 3 rows: its first sample goes with batch one, the other two with batch two
    by_file = {}
    for e in json.load(open(c))["callsets"].values():
        by_file.setdefault(e["filename"], []).append(e["row_idx"])
    assert any(min(r) < cut <= max(r) for r in by_file.values()), "the cut must split a file"
    for kw in (dict(), dict(device=0)):
        one = gdb.import_cells(v, c, file_root=d, ub_callset_row_idx=cut - 1, **kw)[0]
        two = gdb.import_cells(v, c, file_root=d, lb_callset_row_idx=cut, **kw)[0]
        assert one == mi.rows_between(whole, 0, cut - 1) and two == mi.rows_between(whole, cut, MAX)
        assert _merged(gdb, [one, two]) == whole


# ---- crafted opaque streams ----------------------------------------------------------------------------------------------------
def test_degenerate_shapes(gdb, tile):
    a, b = mi.cell(3, 7, b"abc"), mi.cell(1, 7, b"")
    assert gdb.merge_cells([b""]) == (b"", 0)
    assert gdb.merge_cells([b"", b""]) == (b"", 0)
    assert _merged(gdb, [a]) == a
    assert _merged(gdb, [a, b""]) == a and _merged(gdb, [b"", a]) == a
    assert _merged(gdb, [a, b]) == b + a == _merged(gdb, [b, a])
    one = mi.crafted_stream(mi.rng(1), 300, (0, 1, 2), 50)
    assert _merged(gdb, [one]) == one == mi.sorted_merge([one])


@pytest.mark.parametrize("total", ["tile-1", "tile", "tile+1", "2*tile+1"])
def test_totals_around_the_tile_with_every_alignment(gdb, tile, total):
    n = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2*tile+1": 2 * tile + 1}[total]
    rng = mi.rng(n)
    for na in (n // 2, 1, n - 1, n // 3):
        A = mi.crafted_stream(rng, na, (0, 2, 4), 97, MIXED + (20000,) if na == n // 2 else MIXED)      # (one shape with cells beyond any LDS tile)
        B = mi.crafted_stream(rng, n - na, (1, 3), 97, MIXED)
        want = mi.sorted_merge([A, B])
        assert _merged(gdb, [A, B]) == want and _merged(gdb, [B, A]) == want, (na, n - na)
    # more than two streams: pairwise rounds, with an odd one carried over
    parts = [mi.crafted_stream(rng, n // 5 + (1 if s == 0 else 0) * (n - 5 * (n // 5)), (s,), 61, MIXED) for s in range(5)]
    assert sum(len(mi.split_cells(p)) for p in parts) == n
    assert _merged(gdb, parts) == mi.sorted_merge(parts)
    assert _merged(gdb, parts[:3]) == mi.sorted_merge(parts[:3])


def test_one_stream_before_the_other_and_alternation(gdb, tile):
    rng = mi.rng(5)
    lo = b"".join(mi.cell(i % 2, i // 2, rng.randbytes(rng.choice(MIXED))) for i in range(2 * tile + 3))
    hi = b"".join(mi.cell(2 + i % 2, 10**6 + i // 2, rng.randbytes(rng.choice(MIXED))) for i in range(tile + 7))
    assert _merged(gdb, [lo, hi]) == lo + hi == mi.sorted_merge([lo, hi])
    assert _merged(gdb, [hi, lo]) == lo + hi
    even = b"".join(mi.cell(0, i, rng.randbytes(rng.choice(MIXED))) for i in range(0, 2 * tile + 2, 2))
    odd = b"".join(mi.cell(1, i, rng.randbytes(rng.choice(MIXED))) for i in range(1, 2 * tile + 1, 2))
    want = mi.sorted_merge([even, odd])
    assert _merged(gdb, [even, odd]) == want == _merged(gdb, [odd, even])
    assert [r for r, _, _ in mi.split_cells(want)][:6] == [0, 1, 0, 1, 0, 1]


def test_equal_keys_inside_one_stream_keep_their_order(gdb, tile):
    rng = mi.rng(6)
    # runs of one key longer than a tile, every cell with a payload of its own; the other stream's keys fall before, between and behind
    runs = b"".join(mi.cell(0, 10, b"first run %d" % i) for i in range(tile + 300)) + b"".join(mi.cell(0, 20, b"second run %d" % i) for i in range(2 * tile + 1))
    other = mi.crafted_stream(rng, 500, (1, 2), 30, MIXED)
    want = mi.sorted_merge([runs, other])
    assert _merged(gdb, [runs, other]) == want == _merged(gdb, [other, runs])
    kept = [c for r, _, c in mi.split_cells(want) if r == 0]
    assert b"".join(kept) == runs


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_name_what_is_wrong(gdb):
    good = mi.crafted_stream(mi.rng(7), 2000, (0, 1), 500)
    cells = mi.split_cells(mi.crafted_stream(mi.rng(8), 1500, (2, 3), 500))
    i = next(k for k in range(700, 1499) if (cells[k][1], cells[k][0]) != (cells[k + 1][1], cells[k + 1][0]))
    cells[i], cells[i + 1] = cells[i + 1], cells[i]
    unsorted = b"".join(c for _, _, c in cells)
    with pytest.raises(gdb.GenomicsDBException, match=r"stream 1 is not sorted by \(column, row\): cell %d comes before cell %d" % (i + 1, i)):
        gdb.merge_cells([good, unsorted])
    with pytest.raises(gdb.GenomicsDBException, match=r"stream 0 is not sorted.*cell %d " % (i + 1)):
        gdb.merge_cells([unsorted, good])
    with pytest.raises(gdb.GenomicsDBException, match=r"stream 1: the size chain runs past the end of the stream.*byte offset %d" % (len(good) - len(mi.split_cells(good)[-1][2]))):
        gdb.merge_cells([mi.cell(5, 5, b""), good[:-1]])
    with pytest.raises(gdb.GenomicsDBException, match="stream 0: the size chain runs past the end of the stream.*byte offset 0"):
        gdb.merge_cells([good[:23]])
    a = mi.crafted_stream(mi.rng(9), 900, (0, 3, 5, 40, 41), 300)
    b = mi.crafted_stream(mi.rng(10), 1100, (1, 41, 5, 7), 300)
    with pytest.raises(gdb.GenomicsDBException, match=r"row 5 is in more than one stream"):
        gdb.merge_cells([a, b])
    c = mi.crafted_stream(mi.rng(11), 100, (8, 9), 300)
    with pytest.raises(gdb.GenomicsDBException, match=r"row 5 is in more than one stream"):
        gdb.merge_cells([c, a, b])
    with pytest.raises(gdb.GenomicsDBException, match=r"stream 1: cell 0 has a negative row"):
        gdb.merge_cells([c, mi.cell(-1, 0, b"")])


# ---- bounded import on the device against the host importer ------------------------------------------------------------------------
BOUNDS = [(0, 0), (1, 1), (1, 2), (2, MAX), (0, MAX), (2, 0), (-3, 1)]


@pytest.mark.parametrize("callsets", ["t0_1_2.json", "t0_1_2_combined.json"])
def test_bounded_import_of_text_bgzf_and_streams(gdb, callsets):
    v, c = _paths(callsets)
    files = sorted({e["filename"] for e in json.load(open(c))["callsets"].values()})
    raw = {f: open(os.path.join(helpers.GOLDEN, f), "rb").read() for f in files}
    for lb, ub in BOUNDS:
        hs = {}
        want = gdb.import_cells(v, c, file_root=helpers.GOLDEN, lb_callset_row_idx=lb, ub_callset_row_idx=ub, stats=hs)
        assert want[1] > 0
        for kw in (dict(inflate="auto"), dict(inflate="host"), dict(inflate="auto", text_budget_bytes=256), dict(streams=raw, file_root="/nonexistent")):
            st = {}
            args = dict(file_root=helpers.GOLDEN, device=0, lb_callset_row_idx=lb, ub_callset_row_idx=ub, stats=st)
            args.update(kw)
            assert gdb.import_cells(v, c, **args) == want, (lb, ub, kw)
            assert st["num_files"] == hs["num_files"]
            if kw.get("inflate") == "auto" and "streams" not in kw:
                assert st["num_device_members"] > 0 and st["num_host_inflated_files"] == 0      # the fixtures are bgzip files


def test_bounded_import_of_bcf2(gdb, tmp_path):
    import bcf_inputs
    v, c = _paths("t0_1_2.json")
    new_c, streams, _ = bcf_inputs.encode_mapping(v, c, helpers.GOLDEN, str(tmp_path / "plain"))
    for lb, ub in BOUNDS:
        want = gdb.import_cells(v, c, file_root=helpers.GOLDEN, lb_callset_row_idx=lb, ub_callset_row_idx=ub)
        st = {}
        assert gdb.import_cells(v, new_c, file_root=str(tmp_path / "plain"), device=0, lb_callset_row_idx=lb, ub_callset_row_idx=ub, stats=st) == want
        assert st["num_files"] == len({r for r, _, _ in mi.split_cells(want[0])})
        assert gdb.import_cells(v, new_c, file_root="/nonexistent", device=0, streams=streams, lb_callset_row_idx=lb, ub_callset_row_idx=ub) == want


def test_bounded_import_of_csv(gdb):
    v, text_mapping = _paths("t0_1_2.json")
    _, csv_mapping = _paths("t0_1_2_csv.json")
    raw = open(os.path.join(INPUTS, "callsets", "t0_1_2.csv"), "rb").read()
    for lb, ub in BOUNDS:
        want = gdb.import_cells(v, text_mapping, file_root=helpers.GOLDEN, lb_callset_row_idx=lb, ub_callset_row_idx=ub)
        for kw in (dict(file_root=helpers.GOLDEN), dict(file_root="/nonexistent", streams={"inputs/callsets/t0_1_2.csv": raw})):
            st = {}
            assert gdb.import_cells(v, csv_mapping, device=0, lb_callset_row_idx=lb, ub_callset_row_idx=ub, stats=st, **kw) == want
            assert st["num_files"] == 1


# ---- end to end: vcf2tiledb grows an array, gt_mpi_gather reads it ------------------------------------------------------------------
def _loader(ws, **more):
    loader = {"row_based_partitioning": False, "produce_tiledb_array": True, "column_partitions": [{"begin": 0, "workspace": str(ws), "array": "arr"}],
              "callset_mapping_file": os.path.join("inputs", "callsets", "t0_1_2.json"), "vid_mapping_file": os.path.join("inputs", "vid.json"),
              "treat_deletions_as_intervals": True, "vcf_header_filename": os.path.join("inputs", "template_vcf_header.vcf"),
              "reference_genome": os.path.join("inputs", "chr1_10MB.fasta.gz")}
    loader.update(more)
    lj = ws / "loader.json"
    lj.write_text(json.dumps(loader))
    return str(lj)


@pytest.mark.parametrize("flavour", ["host_import", "import_on_device"])
def test_vcf2tiledb_merges_a_batch_into_the_array(gdb, tmp_path, flavour):
    tool = os.path.join(os.path.dirname(gdb.__file__), "vcf2tiledb")
    flags = ["--import-on-device"] if flavour == "import_on_device" else []

    def run(ws, **more):
        r = subprocess.run([tool] + flags + [_loader(ws, **more)], cwd=helpers.GOLDEN, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        return r.stderr.decode()
    once, grown = tmp_path / "once", tmp_path / "grown"
    once.mkdir()
    grown.mkdir()
    run(once)
    one_shot = (once / "arr" / "cells.bin").read_bytes()
    assert one_shot == helpers.cells_for("t0_1_2.json", "vid.json")
    err = run(grown, lb_callset_row_idx=0, ub_callset_row_idx=1)
    assert "merge_tiledb_array" not in err
    first = (grown / "arr" / "cells.bin").read_bytes()
    assert first == mi.rows_between(one_shot, 0, 1)
    (grown / "arr" / "fragment.gdbamd").write_bytes(b"a columnar copy of the first batch")
    err = run(grown, lb_callset_row_idx=2, ub_callset_row_idx=2, delete_and_create_tiledb_array=False)
    timer = [l for l in err.splitlines() if ",merge_tiledb_array," in l]
    assert len(timer) == 1 and ",streams,2," in timer[0] and ",cells_out,%d," % len(mi.split_cells(one_shot)) in timer[0] and ",tile,1024," in timer[0]
    assert (grown / "arr" / "cells.bin").read_bytes() == one_shot
    assert sorted(os.listdir(grown / "arr")) == ["cells.bin"]          # the stale fragment and the temporary file are gone
    # the grown array answers the query like the one-shot array: the golden of the CASES entry of this mapping
    _, callsets, vid, ov, golden, mode = [c for c in CASES if c[0] == "t0_1_2_vcf_at_0"][0]
    q, _ = helpers.query_json(callsets, vid, ov, mode)
    q["workspace"], q["array"] = str(grown), "arr"
    qf = tmp_path / "query.json"
    qf.write_text(json.dumps(q))
    r = subprocess.run([os.path.join(helpers.ROOT, "genomicsdb_amd", "gt_mpi_gather"), "-j", str(qf), "--produce-Broad-GVCF"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == helpers.golden_text(golden)
    if flavour == "import_on_device":       # (what follows does not depend on where the batch was converted)
        return
    # "compress_tiledb_array" with the merge: the columnar file is rebuilt from the MERGED cells
    regrown = tmp_path / "regrown"
    regrown.mkdir()
    run(regrown, lb_callset_row_idx=0, ub_callset_row_idx=1)
    run(regrown, lb_callset_row_idx=2, ub_callset_row_idx=2, delete_and_create_tiledb_array=False, compress_tiledb_array=True)
    assert (regrown / "arr" / "cells.bin").read_bytes() == one_shot
    frag = regrown / "arr" / "fragment.gdbamd"
    assert frag.exists() and frag.read_bytes()[8:12] == b"\x03\x00\x00\x00"
    os.rename(regrown / "arr" / "cells.bin", regrown / "arr" / "cells.bin.away")      # (the query must come from the columnar file)
    q["workspace"] = str(regrown)
    qf.write_text(json.dumps(q))
    r = subprocess.run([os.path.join(helpers.ROOT, "genomicsdb_amd", "gt_mpi_gather"), "-j", str(qf), "--produce-Broad-GVCF"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == helpers.golden_text(golden)
    # without the key (or with true) the tool overwrites, as it always did
    err = run(grown, lb_callset_row_idx=2, ub_callset_row_idx=2)
    assert "merge_tiledb_array" not in err and (grown / "arr" / "cells.bin").read_bytes() == mi.rows_between(one_shot, 2, 2)
    err = run(grown, lb_callset_row_idx=0, ub_callset_row_idx=0, delete_and_create_tiledb_array=True)
    assert "merge_tiledb_array" not in err and (grown / "arr" / "cells.bin").read_bytes() == mi.rows_between(one_shot, 0, 0)
