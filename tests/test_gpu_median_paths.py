"""Every piece of code that takes a median, at the thresholds where prepare_interval changes from one to the next.  The `median` reducer
of INFO fields and QUAL is computed by four pieces of code, chosen from the counts of the interval (T variant calls, P records, n calls of
one record):
  sorted                 k_median_keys + a device-wide radix sort + the binary search of reduce_scalar: T > 16 P, or GDBAMD_SORTED_MEDIAN
  workgroup per record   k_big_records + k_big_medians: not sorted, 48 < n <= 4096, and fewer than 4096 such records listed before this one
  workgroup site kernel  k_site_huge (radix select): n > 256, or n > 24 when T / P >= 24 - asked only when the record has no big entry
  per-thread scan        the quadratic loop of reduce_scalar: everything else
All four must print the oracle's bytes.  The inputs (tests/hot_record_inputs.py: MEDIAN_CASES) put hot columns among columns of one call
each, so that the interval's average stands where the case wants it, and every case predicts from its input lines alone which path runs;
every run asserts gdbamd_interval_stats.sorted_median_fields / big_median_records / big_median_unlisted / huge_records / huge_fallbacks
against that prediction - without the counters "same bytes" passes vacuously whenever the path under test never ran.  Every hot column
carries IMED, FMED (INFO: deletions that began before the record do not count) and QUAL (they do): three median slots.  Each case runs in
the default mode, under GDBAMD_NO_HUGE_SITES=1 and under GDBAMD_SORTED_MEDIAN=1.  tests/test_hot_records_cpu.py runs the same inputs
through the oracle and the per-thread scan of the kernel bodies and asserts the medians known by hand.
NaN is in none of the inputs: the paths order it differently by construction (`<` against bit order), and the reference's nth_element on
NaN is unspecified."""
import pytest

import helpers
import hot_record_inputs as hri
from test_gpu_hot_records import _device

pytestmark = pytest.mark.gpu
COUNTERS = ("sorted_median_fields", "big_median_records", "big_median_unlisted", "huge_records", "huge_fallbacks")


def _case(name, tmp_path):
    """(cells, query, the interval, the oracle's bytes) of a case whose predictions hold on its input lines"""
    cells, q, facts = hri.MEDIAN_CASES[name][0](tmp_path)
    iv, = hri.check_case(name, facts)
    want, nrec, _ = helpers.oracle_run(hri.query_for(q, iv), cells, with_header=False)
    assert nrec == iv["num_records"]
    return cells, q, iv, want


def _run(name, case, monkeypatch, mode, is_bcf=False):
    cells, q, iv, want = case
    assert mode in hri.MEDIAN_MODES
    import genomicsdb_amd
    for knob, on in (("GDBAMD_SORTED_MEDIAN", mode == "sorted"), ("GDBAMD_NO_HUGE_SITES", mode == "no_huge")):
        if on:
            monkeypatch.setenv(knob, "1")
        else:
            monkeypatch.delenv(knob, raising=False)
    try:
        if is_bcf:
            (got, st), = _device(q, cells, [iv], monkeypatch, mode == "no_huge", is_bcf=True)
        else:                                                       # one run: the host buffer holds the largest case's text
            e = genomicsdb_amd.CombineEngine(q)
            try:
                e.stage_cells(cells)
                got, st = e.run_interval(iv["begin"], iv["end"], arena_bytes=1 << 22, host_cap=1 << 26)
            finally:
                e.close()
    finally:
        monkeypatch.delenv("GDBAMD_SORTED_MEDIAN", raising=False)
        monkeypatch.delenv("GDBAMD_NO_HUGE_SITES", raising=False)
    counters = tuple(getattr(st, c) for c in COUNTERS)
    print(name, mode, "BCF2" if is_bcf else "text", dict(zip(COUNTERS, counters)), "records", st.num_records, "calls", st.num_heavy_incidences)
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        assert False, (name, mode, "records that differ (POS, device / oracle up to the samples):",
                       [(w[i].split(b"\t")[1], g[i].split(b"\t")[5:8], w[i].split(b"\t")[5:8]) for i in bad[:6]], len(bad), len(g), len(w))
    assert st.num_records == iv["num_records"] and st.num_heavy_incidences == iv["heavy"]
    assert counters == hri.median_counters(iv, mode), (name, mode, dict(zip(COUNTERS, counters)))
    return st


SMALL = [n for n in hri.MEDIAN_CASES if n not in ("median_capacity", "median_list_overflow")]


@pytest.mark.parametrize("mode", hri.MEDIAN_MODES)
@pytest.mark.parametrize("name", SMALL)
def test_median_paths_at_their_thresholds(tmp_path, monkeypatch, name, mode):
    """48 / 49 calls; T = 16 P / 16 P + 1; sorted with one record and with the hot record last of four; values inside the workgroup
    medians; spanning deletions; more big records than workgroups; one record that is big and huge"""
    case = _case(name, tmp_path)
    st = _run(name, case, monkeypatch, mode)
    iv = case[2]
    if mode != "sorted":                                            # what each case is there for, stated once more by hand
        want = {"median_48_49": (0, 1, 0), "median_average_16": (0, 1, 0), "median_average_16_and_one_call": (3, 0, 0),
                "median_sorted_single_record": (3, 0, 0), "median_sorted_last_of_4_records": (3, 0, 0), "median_values": (0, 13, 0),
                "median_spanning": (0, 2, 0), "median_grid_stride": (0, 70, 0), "median_big_and_huge": (0, 1, 0),
                "median_big_and_huge_tied_zeros": (0, 1, 0)}[name]
        assert (st.sorted_median_fields, st.big_median_records, st.big_median_unlisted) == want
        assert st.huge_records == (1 if name.startswith("median_big_and_huge") and mode == "default" else 0)
    else:
        assert st.sorted_median_fields == 3 and st.big_median_records == 0
    assert iv["heavy"] <= 16 * iv["num_records"] or iv["sorted"]


@pytest.mark.parametrize("mode", hri.MEDIAN_MODES)
def test_median_values_as_bcf2(tmp_path, monkeypatch, mode):
    """the value columns once more with BCF2 pages: the medians as typed values, missing for "no valid value" """
    _run("median_values", _case("median_values", tmp_path), monkeypatch, mode, is_bcf=True)


@pytest.fixture(scope="module")
def capacity_case(tmp_path_factory):
    return _case("median_capacity", tmp_path_factory.mktemp("median_capacity"))


@pytest.mark.parametrize("mode", hri.MEDIAN_MODES)
def test_median_of_4096_and_4097_calls(capacity_case, monkeypatch, mode):
    """4096 calls fill the LDS of k_big_medians; the record with 4097 is not listed: its medians come from k_site_huge, and under
    GDBAMD_NO_HUGE_SITES=1 from the per-thread scan.  (Input and oracle, once per module: 4097 sample files, 1.5 - 3.5 s on a CPU)"""
    st = _run("median_capacity", capacity_case, monkeypatch, mode)
    if mode != "sorted":
        assert st.big_median_records == 1 and st.big_median_unlisted == 0 and st.huge_records == (2 if mode == "default" else 0)


@pytest.fixture(scope="module")
def overflow_case(tmp_path_factory):
    return _case("median_list_overflow", tmp_path_factory.mktemp("median_list_overflow"))


def test_more_big_records_than_the_list_holds(overflow_case, monkeypatch):
    """4100 big records: 4096 are listed, four get index -1 while the counter goes on to 4100, and their medians come from the per-thread
    scan.  One run, in the default mode.  (Input and oracle: 210 000 input lines and 13 120 records, 6 - 8 s on a CPU -the sizes are the kernel's constants)"""
    st = _run("median_list_overflow", overflow_case, monkeypatch, "default")
    assert (st.big_median_records, st.big_median_unlisted, st.sorted_median_fields, st.huge_records) == (4096, 4, 0, 0)
