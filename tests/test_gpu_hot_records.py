"""The workgroup-per-record site kernel (k_site_huge) on the hand-made hot records of tests/hot_record_inputs.py: single-column and
few-column intervals in which a record with 25 calls already gets a workgroup of its own.  Every case compares the device's bytes with the
oracle's twice - in the default mode and under GDBAMD_NO_HUGE_SITES=1 (the serial walk alone) - and asserts the counters that say which
path wrote them: gdbamd_interval_stats.huge_records (records given to the kernel) and huge_fallbacks (the ones it handed back to the serial
walk: two alleles with one hash, a full table, several FILTER ids).  Without the counters "default == serial" passes vacuously whenever the
record never qualified.  tests/test_hot_records_cpu.py runs the same inputs through the oracle and the kernel bodies and asserts what is
known about them by hand."""
import struct

import pytest

import helpers
import hot_record_inputs as hri

pytestmark = pytest.mark.gpu
ARENA = 1 << 22


def _device(q, cells, ivs, monkeypatch, no_huge, is_bcf=False):
    """[(text of the interval, statistics)] of one engine over the case's intervals, with or without the workgroup kernel"""
    import bcf2text
    import genomicsdb_amd
    if no_huge:
        monkeypatch.setenv("GDBAMD_NO_HUGE_SITES", "1")
    else:
        monkeypatch.delenv("GDBAMD_NO_HUGE_SITES", raising=False)
    e = genomicsdb_amd.CombineEngine(q, is_bcf=is_bcf)
    try:
        e.stage_cells(cells)
        out = []
        for iv in ivs:
            body, st = e.run_interval(iv["begin"], iv["end"], arena_bytes=ARENA, host_cap=ARENA)
            if is_bcf:
                h = bcf2text.Header(e.header.decode())
                at, lines = 0, []
                while at < len(body):
                    l_shared, l_indiv = struct.unpack_from("<II", body, at)
                    lines.append(bcf2text.record_to_text(h, body[at:at + 8 + l_shared + l_indiv], helpers.format_float))
                    at += 8 + l_shared + l_indiv
                body = ("\n".join(lines) + "\n").encode()
            out.append((body, st))
        return out
    finally:
        e.close()
        monkeypatch.delenv("GDBAMD_NO_HUGE_SITES", raising=False)


def _check_case(name, tmp_path, monkeypatch, bcf=False):
    cells, q, facts = hri.CASES[name][0](tmp_path)
    ivs = hri.check_case(name, facts)
    want = [helpers.oracle_run(hri.query_for(q, iv), cells, with_header=False)[0] for iv in ivs]
    for no_huge in (False, True):
        for iv, w, (got, st) in zip(ivs, want, _device(q, cells, ivs, monkeypatch, no_huge)):
            assert got == w, (name, iv["begin"], "serial walk alone" if no_huge else "default")
            assert st.num_records == iv["num_records"] and st.num_heavy_incidences == iv["heavy"]
            if no_huge:
                assert st.huge_records == 0 and st.huge_fallbacks == 0
            else:
                assert (st.huge_records, st.huge_fallbacks) == (iv["huge_records"], iv["huge_fallbacks"]), (name, iv["begin"])
    if bcf:
        for no_huge in (False, True):
            for iv, w, (got, st) in zip(ivs, want, _device(q, cells, ivs, monkeypatch, no_huge, is_bcf=True)):
                assert got == w, (name, iv["begin"], "BCF2", no_huge)
                assert st.huge_records == (0 if no_huge else iv["huge_records"])
    return facts, want


@pytest.mark.parametrize("name", ["selection_24_calls", "selection_25_calls", "selection_257_and_256_calls_among_30_records"])
def test_selection_of_hot_records(tmp_path, monkeypatch, name):
    """more than 24 calls when the interval averages 24 and more a record, more than 256 otherwise"""
    facts, _ = _check_case(name, tmp_path, monkeypatch)
    iv = facts["intervals"][0]
    assert iv["threshold"] == (256 if name.startswith("selection_257") else 24)
    if name.startswith("selection_257"):
        assert sorted(iv["calls"].values())[-3:] == [3, 256, 257] and iv["heavy"] // iv["num_records"] < 24


@pytest.mark.parametrize("name", ["first_appearance", "suffix_extension"])
def test_merged_alleles_in_order_of_first_appearance(tmp_path, monkeypatch, name):
    facts, want = _check_case(name, tmp_path, monkeypatch, bcf=True)
    hri.check_merged_lists(want[0], facts["intervals"][0])
    if name == "suffix_extension":
        rec = hri.record_lines(want[0])[0]
        assert rec[3] == facts["by_hand_ref"] and rec[4].split(",") == facts["by_hand_alt"]


@pytest.mark.parametrize("name", ["collision_equal_length", "collision_unequal_length", "collision_after_extension", "collision_in_one_of_two_records"])
def test_two_alleles_with_one_hash_go_back_to_the_serial_walk(tmp_path, monkeypatch, name):
    facts, want = _check_case(name, tmp_path, monkeypatch, bcf=True)
    iv = facts["intervals"][0]
    assert iv["huge_fallbacks"] == 1 and iv["huge_records"] == (2 if name == "collision_in_one_of_two_records" else 1)
    hri.check_merged_lists(want[0], iv)


@pytest.mark.parametrize("name,fallbacks", [("marker_hash_alone", 0), ("marker_hash_with_remap_target", 1)])
def test_allele_whose_hash_is_the_empty_marker(tmp_path, monkeypatch, name, fallbacks):
    """GGTTAAAGCAACAA hashes to 0xFFFFFFFF, the table's empty marker, and is filed under 0xFFFFFFFE: an ordinary allele unless another one
    hashes to that"""
    facts, want = _check_case(name, tmp_path, monkeypatch, bcf=True)
    iv = facts["intervals"][0]
    assert iv["huge_fallbacks"] == fallbacks and hri.MARKER_ALLELE in iv["merged_alt"][iv["begin"]]
    hri.check_merged_lists(want[0], iv)


def test_most_merged_alleles_a_record_may_have(tmp_path, monkeypatch):
    facts, want = _check_case("cap_126_alts", tmp_path, monkeypatch, bcf=True)
    rec = hri.record_lines(want[0])[0]
    assert len(rec[4].split(",")) == hri.MAX_MERGED_ALT + 1 and "PL" not in rec[8].split(":")


@pytest.mark.parametrize("name", list(hri.TOO_MANY))
def test_too_many_merged_alleles_is_the_same_error_on_both_paths(tmp_path, monkeypatch, name):
    """one allele more than the cap, and more distinct alleles than the kernel's table has slots: an error, no output, no hang"""
    import genomicsdb_amd
    builder, calls = hri.TOO_MANY[name]
    cells, q, facts = builder(tmp_path)
    iv = facts["intervals"][0]
    assert iv["heavy"] == calls and iv["huge_records"] == 1 and iv["distinct"][iv["begin"]] > hri.MAX_MERGED_ALT
    for no_huge in (False, True):
        with pytest.raises(genomicsdb_amd.api.GenomicsDBException, match=hri.TOO_MANY_MERGED_TEXT):
            _device(q, cells, [iv], monkeypatch, no_huge)


@pytest.mark.parametrize("name", ["spanning_deletions_min_pl_gt", "spanning_deletions_plain_gt"])
def test_spanning_deletions_at_a_hot_record(tmp_path, monkeypatch, name):
    facts, want = _check_case(name, tmp_path, monkeypatch)
    rec = hri.record_lines(want[0])[0]
    assert rec[4].split(",")[0] == "*" and len({s.split(":")[0].count("/") for s in rec[9:]}) == 3


def test_scalar_reducers_of_hot_records(tmp_path, monkeypatch):
    """sum, mean and median of an int and a float field each: a float sum that depends on the order of the calls, medians of odd and even
    counts with negative values, of equal values, of one value among missing ones and of none, and zeros of both signs tied at the middle of
    25, 26, 27 and 64 values"""
    from test_hot_records_cpu import check_reducer_text
    facts, want = _check_case("reducers_small", tmp_path, monkeypatch)
    assert len(want) == len(hri.REDUCER_COLUMN_NAMES)
    for w, col in zip(want, facts["columns"]):
        check_reducer_text(w, col)


@pytest.mark.parametrize("n", [2048, 2049, 2050])
def test_float_sum_in_call_order_across_the_staging_chunk(tmp_path, monkeypatch, n):
    """2 048 values are one LDS staging chunk of the float sum: the sum of 1e8, 1, -1e8, 1, ... must be carried from chunk to chunk"""
    from test_hot_records_cpu import check_reducer_text
    facts, want = _check_case("reducers_%d" % n, tmp_path, monkeypatch)
    check_reducer_text(want[0], facts["columns"][0])


def test_seeded_fuzz_of_hot_records(tmp_path, monkeypatch):
    """30 seeds (tests/test_hot_records_cpu.py checks that the oracle accepts every one)"""
    import genomicsdb_amd
    huge = fallbacks = 0
    for seed in hri.FUZZ_SEEDS:
        d = tmp_path / ("s%d" % seed)
        d.mkdir()
        cells, q, facts = hri.fuzz(d, seed)
        ivs = facts["intervals"]
        want, nrec, _ = helpers.oracle_run(hri.query_for_all(q, ivs), cells, with_header=False)
        want = want.splitlines(True)
        assert nrec == len(ivs) == len(want)
        e = genomicsdb_amd.CombineEngine(q)             # one engine per seed: the knob is read anew for every interval
        try:
            e.stage_cells(cells)
            for no_huge in (False, True):
                if no_huge:
                    monkeypatch.setenv("GDBAMD_NO_HUGE_SITES", "1")
                else:
                    monkeypatch.delenv("GDBAMD_NO_HUGE_SITES", raising=False)
                for iv, w in zip(ivs, want):
                    got, st = e.run_interval(iv["begin"], iv["end"], arena_bytes=ARENA, host_cap=ARENA)
                    assert got == w, (seed, iv["begin"], no_huge)
                    assert st.num_records == 1 and st.num_heavy_incidences == iv["heavy"]
                    if no_huge:
                        assert st.huge_records == 0 and st.huge_fallbacks == 0
                    else:
                        assert (st.huge_records, st.huge_fallbacks) == (1, iv["huge_fallbacks"]), (seed, iv["begin"])
                        huge += st.huge_records
                        fallbacks += st.huge_fallbacks
        finally:
            e.close()
            monkeypatch.delenv("GDBAMD_NO_HUGE_SITES", raising=False)
    assert huge >= 30 and 1 <= fallbacks < huge
