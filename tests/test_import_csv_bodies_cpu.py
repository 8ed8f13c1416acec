"""The CSV path of the device importer on the CPU, through the harness tests/hostsim_import_csv (batches, line index, measure,
write, deferred tokens, sort and gather as plain loops around the bodies of csrc/core/gdb_import_csv.hpp and the host share
csrc/host/import_common.hpp).  The expected cells never come from the code under test:
  check 1  the reference's own CSV file of t0_1_2 gives the host TEXT importer's cells of t0_1_2;
  check 2  cells -> tests/tools/cells2csv.py (an independent printer) -> CSV path == the same cells, lines shuffled, three budgets;
  check 3  a hand-made file whose cells are written out here with struct.pack;
  check 4  every refusal and line error by its words and line number;
  check 5  one mapping that mixes a CSV file and a bgzipped VCF.
One figure differs from the plain round trip and is derived in csv_inputs.after_csv: info_ops.json holds float vectors with a
missing element (NaN bits 0x7f800001); %.9g prints "nan", strtof reads the default NaN 0x7fc00000, so those 3 elements are expected
as 0x7fc00000 - and as 3 deferred tokens.  Host code only - no device."""
import ctypes
import os
import subprocess

import pytest

import csv_inputs as ci
import helpers
from csv_inputs import cells2csv


@pytest.fixture(scope="module")
def gdb():
    from genomicsdb_amd import build as b
    b.build_native()
    import genomicsdb_amd
    return genomicsdb_amd


@pytest.fixture(scope="module")
def built():
    from genomicsdb_amd import build as b
    return b.build_hostsim_import_csv()


@pytest.fixture(scope="module")
def sim(built):
    L = ctypes.CDLL(built[0])
    L.hsc_last_error.restype = ctypes.c_char_p
    L.hsc_free.argtypes = [ctypes.c_void_p]
    return L


STATS = ("files", "records", "cells", "spanning", "deferred", "batches", "text_bytes")


def sim_import(L, vid, callsets, root, treat=True, begin=0, end=ci.COLUMN_END, budget=0, streams=None):
    """-> (bytes, stats); raises RuntimeError with the harness's message"""
    c = ctypes
    streams = streams or {}
    n = len(streams)
    names = (c.c_char_p * max(n, 1))(*[os.fsencode(k) for k in streams])
    datas = (c.c_char_p * max(n, 1))(*[bytes(v) for v in streams.values()])
    sizes = (c.c_uint64 * max(n, 1))(*[len(v) for v in streams.values()])
    p, nb = c.c_void_p(), c.c_uint64()
    st = (c.c_int64 * len(STATS))()
    rc = L.hsc_import(os.fsencode(vid), os.fsencode(callsets), os.fsencode(root), 1 if treat else 0, c.c_int64(begin), c.c_int64(end), c.c_uint64(budget), names, datas,
                      sizes, n, c.byref(p), c.byref(nb), st)
    if rc != 0:
        raise RuntimeError(L.hsc_last_error().decode())
    try:
        return c.string_at(p.value, nb.value), dict(zip(STATS, st))
    finally:
        L.hsc_free(p)


# ---- check 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [0, 256])
def test_reference_csv_file_gives_the_cells_of_the_vcfs(gdb, sim, budget):
    v, text_mapping = ci.paths("t0_1_2.json", "vid.json")
    _, csv_mapping = ci.paths("t0_1_2_csv.json", "vid.json")
    want, ncells = gdb.import_cells(v, text_mapping, file_root=helpers.GOLDEN)
    got, st = sim_import(sim, v, csv_mapping, helpers.GOLDEN, budget=budget)
    assert ncells == 5 and got == want and got == helpers.cells_for("t0_1_2.json", "vid.json")
    assert st["cells"] == 5 and st["records"] == 5 and st["files"] == 1 and st["deferred"] == 0 and st["spanning"] == 0
    if budget:
        assert st["batches"] > 1
    # the partition that begins at 12150: the three cells at 17384 only.  The text importer replays the two reference blocks that
    # reach into it; the reference's CSV reader looks at the column alone
    text_cells, n_text = gdb.import_cells(v, text_mapping, file_root=helpers.GOLDEN, column_begin=12150)
    got, st = sim_import(sim, v, csv_mapping, helpers.GOLDEN, begin=12150, budget=budget)
    full = cells2csv.cells_to_lines(want, v)
    assert [ln.split(",")[1] for ln in cells2csv.cells_to_lines(got, v)] == ["17384"] * 3 and st["cells"] == 3 and st["spanning"] == 0
    assert n_text == 5 and text_cells.endswith(got) and len(text_cells) > len(got)
    assert cells2csv.cells_to_lines(text_cells, v)[2:] == full[2:]


def test_host_importer_names_the_csv_file(gdb):
    v, csv_mapping = ci.paths("t0_1_2_csv.json", "vid.json")
    with pytest.raises(gdb.GenomicsDBException, match=r"t0_1_2\.csv is a CSV cell file: CSV input needs the device importer"):
        gdb.import_cells(v, csv_mapping, file_root=helpers.GOLDEN)


# ---- check 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("callsets,vid", ci.PAIRS, ids=["%s-%s" % p for p in ci.PAIRS])
def test_round_trip_through_the_printer(gdb, sim, tmp_path, callsets, vid):
    v, c = ci.paths(callsets, vid)
    mapping = ci.csv_mapping(c, str(tmp_path))
    for treat in (True, False):
        cells, ncells = gdb.import_cells(v, c, file_root=helpers.GOLDEN, treat_deletions_as_intervals=treat)
        want, nans = ci.after_csv(cells, v)
        assert (nans == 3) if callsets == "info_ops.json" else (nans == 0 and want == cells)
        text = cells2csv.csv_text(cells, v, seed=11).encode("latin-1")
        (tmp_path / "cells.csv").write_bytes(text)
        for budget in (0, 256, 4096):
            got, st = sim_import(sim, v, mapping, str(tmp_path), treat, budget=budget)
            assert got == want and st["cells"] == ncells and st["records"] == ncells and st["deferred"] == nans
            if budget and len(text) > budget:
                assert st["batches"] > 1
        # the same bytes from memory, under the name the mapping gives the file
        assert sim_import(sim, v, mapping, "/nonexistent", treat, budget=256, streams={"cells.csv": text})[0] == want


def test_every_line_ten_times_is_cut_at_both_budgets(gdb, sim, tmp_path):
    """the fixtures are shorter than 4096 bytes: t0_1_2_combined with every line ten times is not.  Lines with equal (column, row)
    keep file order, so every cell is expected ten times in a row"""
    v, c = ci.paths("t0_1_2_combined.json", "vid.json")
    cells, ncells = gdb.import_cells(v, c, file_root=helpers.GOLDEN)
    want = b"".join(x * 10 for x in ci.split_cells(cells))
    text = cells2csv.csv_text(cells, v, seed=3) * 10
    (tmp_path / "cells.csv").write_text(text)
    mapping = ci.csv_mapping(c, str(tmp_path), key="sorted_csv_files")
    batches = []
    for budget in (0, 256, 4096):
        got, st = sim_import(sim, v, mapping, str(tmp_path), budget=budget)
        assert got == want and st["cells"] == 10 * ncells
        batches.append(st["batches"])
    assert batches[0] == 1 and batches[1] > batches[2] > 1


@pytest.mark.parametrize("callsets,vid", ci.ID_PAIRS, ids=["%s-%s" % p for p in ci.ID_PAIRS])
def test_a_vid_that_declares_id_is_refused(sim, tmp_path, callsets, vid):
    v, c = ci.paths(callsets, vid)
    mapping = ci.csv_mapping(c, str(tmp_path))
    (tmp_path / "cells.csv").write_text("0,1,1,A,&\n")
    with pytest.raises(RuntimeError, match="field ID: a vid that declares ID is not imported from CSV cell files"):
        sim_import(sim, v, mapping, str(tmp_path))


# ---- check 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [0, 64])
def test_hand_made_file_with_known_answers(sim, budget):
    v, c = ci.paths(*ci.HAND)
    for begin, end in ((0, ci.COLUMN_END), ci.HAND_PARTITION):
        want, ncells = ci.hand_cells(begin, end)
        got, st = sim_import(sim, v, c, helpers.GOLDEN, begin=begin, end=end, budget=budget)
        assert got == want
        assert st["cells"] == ncells and st["records"] == ci.HAND_RECORDS and st["deferred"] == ci.HAND_DEFERRED and st["spanning"] == 0
        assert st["text_bytes"] == os.path.getsize(os.path.join(helpers.GOLDEN, "inputs", "callsets", "csv_hand.csv"))
        if budget:
            assert st["batches"] > 1
    assert ci.hand_cells(*ci.HAND_PARTITION)[1] == 3 and ci.hand_cells()[1] == 5


def test_numbers_taken_on_the_device_are_the_c_library_s(sim):
    """every token the bodies take themselves has the bits of strtoll(base 0) / strtof; imp_csv_integer IS strtoll(base 0)"""
    import random
    import struct
    rng = random.Random(5)
    toks = ["0", "-0", "7", "-7", "+7", "007", "010", "0x1f", "0X1F", "0x", "0xg", "08", " 5", "\t-5", "12abc", "abc", "", "-", "+", "1e3", "9223372036854775807",
            "9223372036854775808", "-9223372036854775808", "-9223372036854775809", "2147483648", "1.5", ".5", "5.", ".", "1e-3", "1e30", "1e-30", "nan", "inf", "-inf",
            "0x1p3", "1.5abc", "1e", "1e+", "3.4028235e38", "1e39", "16777217", "0.1", "33554433", "8388608.5", "4.7683716e-7"]
    for _ in range(3000):
        mant = rng.randrange(1, 2**24) * 2 + 1          # 25 significant bits: exactly half way between two floats
        toks.append(str(mant << rng.randrange(0, 20)))
        toks.append("%d.%0*d" % (rng.randrange(0, 10**rng.randrange(1, 8)), rng.randrange(1, 8), rng.randrange(0, 10**7) % 10**7))
        toks.append("%.*e" % (rng.randrange(0, 12), rng.uniform(-1e6, 1e6) * 10.0**rng.randrange(-20, 20)))
        toks.append(str(rng.randrange(-2**40, 2**40)))
    blob, offs = b"", []
    for t in toks:
        offs.append(len(blob))
        blob += t.encode() + b"\0"
    n = len(toks)
    c = ctypes
    u8, i64, u32 = (c.c_uint8 * n), (c.c_int64 * n), (c.c_uint32 * n)
    int_taken, int_value, full_ok, full_value, ref_int_ok, ref_int = u8(), i64(), u8(), i64(), u8(), i64()
    float_taken, float_bits, ref_float_ok, ref_float_bits = u8(), u32(), u8(), u32()
    sim.hsc_check_numbers(blob, (c.c_uint32 * n)(*offs), n, int_taken, int_value, full_ok, full_value, ref_int_ok, ref_int, float_taken, float_bits, ref_float_ok, ref_float_bits)
    taken_i = taken_f = half_way = 0
    for k, t in enumerate(toks):
        if int_taken[k]:
            taken_i += 1
            assert ref_int_ok[k] and int_value[k] == ref_int[k], t
        if full_ok[k] == 1:
            assert ref_int_ok[k] and full_value[k] == ref_int[k], t
        elif full_ok[k] == 0:
            assert not ref_int_ok[k], t
        else:
            assert ref_int_ok[k] and abs(ref_int[k]) >= 2**63 - 1, t         # strtoll saturated
        if float_taken[k]:
            taken_f += 1
            assert ref_float_ok[k] and float_bits[k] == ref_float_bits[k], t
        elif t.isdigit() and struct.unpack("<f", struct.pack("<I", ref_float_bits[k]))[0] != int(t):
            half_way += 1
    assert taken_i > 3000 and taken_f > 6000 and half_way > 1000
    for t, want in (("7", 1), ("-7", 1), ("-0", 1), ("+7", 0), ("007", 0), ("0x1f", 0), (" 5", 0), ("12abc", 0)):
        assert int_taken[toks.index(t)] == want, t
    for t, want in (("1.5", 1), ("1e-3", 1), ("1e30", 0), ("nan", 0), ("1.5abc", 0), ("0x1p3", 0), ("16777217", 0)):
        assert float_taken[toks.index(t)] == want, t


# ---- check 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ci.LINE_ERRORS, ids=[c[0] for c in ci.LINE_ERRORS])
def test_line_errors_name_file_and_line(sim, tmp_path, case):
    _, lines, words, line = case
    v, c, root = ci.write_case(str(tmp_path), lines)
    for budget in (0, 40):
        with pytest.raises(RuntimeError, match=words + r".*a\.csv line %d\)" % line):
            sim_import(sim, v, c, root, budget=budget)


@pytest.mark.parametrize("case", ci.VID_REFUSALS, ids=[c[0] for c in ci.VID_REFUSALS])
def test_vids_the_csv_path_does_not_cover_are_refused_by_name(sim, tmp_path, case):
    _, extra, words = case
    v, c, root = ci.write_case(str(tmp_path), [ci.GOOD], vid_fields=extra)
    with pytest.raises(RuntimeError, match=words):
        sim_import(sim, v, c, root)


def test_compressed_csv_is_refused_by_name(sim, tmp_path):
    import gzip
    v, c, root = ci.write_case(str(tmp_path), None, raw=gzip.compress((ci.GOOD + "\n").encode()))
    with pytest.raises(RuntimeError, match=r"a\.csv is gzip or BGZF: compressed CSV cell files are not imported"):
        sim_import(sim, v, c, root)


def test_a_listed_file_that_no_callset_names_is_ignored(sim, tmp_path):
    v, c = ci.paths(*ci.HAND)        # its mapping lists inputs/callsets/no_callset_names_this.csv, which does not exist
    assert not os.path.exists(os.path.join(helpers.GOLDEN, "inputs", "callsets", "no_callset_names_this.csv"))
    assert sim_import(sim, v, c, helpers.GOLDEN)[1]["files"] == 1


# ---- check 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [0, 256])
def test_mixed_mapping(gdb, sim, tmp_path, budget):
    v, c = ci.paths("t0_1_2.json", "vid.json")
    want, ncells = gdb.import_cells(v, c, file_root=helpers.GOLDEN)
    lines = [ln for ln in cells2csv.cells_to_lines(want, v) if ln.split(",")[0] in ("0", "1")]
    mapping = ci.csv_mapping(c, str(tmp_path), name=str(tmp_path / "rows01.csv"), rows=(0, 1))       # (an absolute name: file_root serves the VCF)
    (tmp_path / "rows01.csv").write_text("".join(ln + "\n" for ln in reversed(lines)))
    got, st = sim_import(sim, v, mapping, helpers.GOLDEN, budget=budget)
    assert got == want and st["cells"] == ncells and st["files"] == 2
    # a partition begin: the reference blocks of rows 0 and 1 reach into it, but they are CSV lines and are not replayed
    got, st = sim_import(sim, v, mapping, helpers.GOLDEN, begin=12150, budget=budget)
    text_cells, _ = gdb.import_cells(v, c, file_root=helpers.GOLDEN, column_begin=12150)
    assert [ln.split(",")[:2] for ln in cells2csv.cells_to_lines(got, v)] == [["0", "17384"], ["1", "17384"], ["2", "17384"]]
    assert text_cells.endswith(got)


# ---- the sanitizers ----------------------------------------------------------------------------------------------------------------
def test_fixtures_under_the_sanitizers(built):
    """the harness source as a stand-alone program (never loaded into Python), built with the address and undefined-behaviour
    sanitizers: the hand fixture and the reference fixture at three budgets; a report would end it with a non-zero status"""
    for callsets, vid, cells, deferred in (ci.HAND + (5, ci.HAND_DEFERRED), ("t0_1_2_csv.json", "vid.json", 5, 0)):
        v, c = ci.paths(callsets, vid)
        r = subprocess.run([built[1], v, c, helpers.GOLDEN, "0", "64", "300"], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        rows = [ln.split() for ln in r.stdout.decode().splitlines()]
        assert [x[0] for x in rows] == ["0", "64", "300"] and all(int(x[1]) == cells and int(x[3]) == deferred for x in rows)
        assert len({x[2] for x in rows}) == 1 and int(rows[1][4]) > 1
