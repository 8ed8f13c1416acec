"""The hand-made hot records of tests/hot_record_inputs.py through the oracle and through the kernel bodies (the serial walk of
site_emit: the workgroup-per-record kernel k_site_huge has no body on the CPU harness), byte for byte - which pins the serial walk, the
reference of tests/test_gpu_hot_records.py's fallbacks, on exactly these inputs.  With nine and more merged alleles the serial walk looks
alleles up through its 256-entry MergeIndex, where only the string compare separates the colliding pair CTGGTCGA / AGCGTCCT.  What is known
by hand about each input - merged REF, merged ALT order, which allele becomes '*', the value of an order-dependent float sum - is asserted on
the oracle's text, and the facts every case predicts (calls, distinct alleles, counters) against the ones derived from its input lines."""
import pytest

import helpers
import hot_record_inputs as hri


def _both(q, cells, iv):
    qi = hri.query_for(q, iv)
    want, nrec, _ = helpers.oracle_run(qi, cells, with_header=False)
    assert nrec == iv["num_records"]
    got, err = helpers.hostsim_run(qi, cells, with_header=False, rows_per_chunk=16, records_per_run=5)
    assert err == 0 and got == want
    return want


@pytest.mark.parametrize("name", [n for n in hri.CASES if not n.startswith("reducers")])
def test_oracle_and_kernel_bodies_on_hot_records(tmp_path, name):
    cells, q, facts = hri.CASES[name][0](tmp_path)
    for iv in hri.check_case(name, facts):
        want = _both(q, cells, iv)
        hri.check_merged_lists(want, iv)


def test_merged_lists_known_by_hand(tmp_path):
    cells, q, facts = hri.suffix_extension(tmp_path)
    iv = facts["intervals"][0]
    want, _, _ = helpers.oracle_run(hri.query_for(q, iv), cells, with_header=False)
    rec = hri.record_lines(want)[0]
    assert rec[3] == facts["by_hand_ref"] == "GACT" and rec[4].split(",") == facts["by_hand_alt"]
    # first appearance: (row, token) order, <NON_REF> last although most calls list it
    cells, q, facts = hri.first_appearance(tmp_path)
    iv = facts["intervals"][0]
    want, _, _ = helpers.oracle_run(hri.query_for(q, iv), cells, with_header=False)
    alt = hri.record_lines(want)[0][4].split(",")
    assert alt[-1] == "<NON_REF>" and set(alt[:-1]) <= set(facts["pool"]) and len(alt) - 1 == iv["distinct"][iv["begin"]] > 20
    assert alt == iv["merged_alt"][iv["begin"]]


@pytest.mark.parametrize("name", ["collision_equal_length", "collision_unequal_length", "collision_after_extension", "marker_hash_with_remap_target"])
def test_colliding_alleles_stay_two_alleles(tmp_path, name):
    """both alleles of the pair are in the merged list (nine and more merged alleles: the serial walk found them through MergeIndex)"""
    cells, q, facts = hri.CASES[name][0](tmp_path)
    iv = facts["intervals"][0]
    merged = iv["merged_alt"][iv["begin"]]
    pair = [a for a in merged if [hri.fixed_hash(b) for b in merged].count(hri.fixed_hash(a)) == 2]
    assert len(pair) == 2 and pair[0] != pair[1] and len(merged) >= 9
    want = _both(q, cells, iv)
    alt = hri.record_lines(want)[0][4].split(",")
    assert pair[0] in alt and pair[1] in alt
    if name == "collision_after_extension":
        assert sorted(pair) == sorted(hri.EQUAL_LENGTH_PAIR) and hri.record_lines(want)[0][3] == "GA"


@pytest.mark.parametrize("min_pl_gt", [True, False])
def test_spanning_deletions_become_star(tmp_path, min_pl_gt):
    cells, q, facts = hri.spanning_deletions(tmp_path, min_pl_gt)
    iv = facts["intervals"][0]
    want = _both(q, cells, iv)
    rec = hri.record_lines(want)[0]
    alt = rec[4].split(",")
    assert alt[0] == "*" and alt[-1] == "<NON_REF>"          # row 0 is a deletion from the column before: '*' appears first
    assert len(rec) == 9 + 48 and rec[3] == "G"
    gts = [s.split(":")[0] for s in rec[9:]]
    assert len({g.count("/") for g in gts}) == 3                # ploidy 1, 2 and 3 side by side


def test_cap_of_merged_alleles(tmp_path):
    """126 ALT alleles (128 with REF and <NON_REF>) is the most find_or_add_merged accepts: more than 50, so PL is dropped"""
    cells, q, facts = hri.CASES["cap_126_alts"][0](tmp_path)
    iv = hri.check_case("cap_126_alts", facts)[0]
    want = _both(q, cells, iv)
    rec = hri.record_lines(want)[0]
    assert len(rec[4].split(",")) == 127 and "PL" not in rec[8].split(":")


@pytest.mark.parametrize("name", list(hri.TOO_MANY))
def test_too_many_merged_alleles_is_an_error_of_the_kernel_bodies(tmp_path, name):
    builder, calls = hri.TOO_MANY[name]
    cells, q, facts = builder(tmp_path)
    iv = facts["intervals"][0]
    assert iv["heavy"] == calls and iv["huge_records"] == 1 and iv["distinct"][iv["begin"]] > hri.MAX_MERGED_ALT
    assert iv["huge_fallbacks"] == (1 if calls > hri.HUGE_TABLE else 0)
    _, err = helpers.hostsim_run(hri.query_for(q, iv), cells, with_header=False, rows_per_chunk=16, records_per_run=5)
    assert err & hri.GDB_ERR_TOO_MANY_MERGED_ALLELES


def _is_float_text(text, v):
    """text is the reference's text of the float v; of a zero only that it is one (the sign of a tied zero: the oracle's bytes)"""
    return float(text) == 0 if v == 0 else text == helpers.format_float(v)


def check_reducer_text(want, col, pos=None):
    """what is known by hand about the reducers of one column, on the oracle's line (the first one, or the record at POS pos): a value that
    is missing or - INFO fields only - sits on a deletion that began before the record does not count (hri.valid_values); the median is
    sorted(valid)[len(valid) // 2], a field without a valid value is absent; QUAL as the vid's median when the column carries one"""
    if isinstance(want, dict):
        line = want[pos]                                                    # (check_median_columns: {POS: line})
    else:
        lines = want.decode().splitlines()
        line = lines[0] if pos is None else [l for l in lines if l.split("\t", 2)[1] == str(pos)][0]
    fsum = hri.valid_values(col, "FSUM")
    if fsum and fsum[:4] == hri.order_dependent_floats(4):
        in_order, by_size = hri.float32_sum(fsum), hri.float32_sum(sorted(fsum))
        assert in_order != by_size                                          # otherwise the input proves nothing
        assert hri.info_value(line, "FSUM") == helpers.format_float(in_order) != helpers.format_float(by_size)
    for f in hri.REDUCER_FIELDS:
        if not hri.valid_values(col, f):
            assert hri.info_value(line, f) is None
    isum = hri.valid_values(col, "ISUM")
    if isum:
        assert hri.info_value(line, "ISUM") == str(sum(isum))
    imean = hri.valid_values(col, "IMEAN")
    if imean and sum(imean) < 0:                                            # the reference's int / unsigned
        q32 = (sum(imean) & 0xFFFFFFFF) // len(imean)
        assert hri.info_value(line, "IMEAN") == str(q32 - (1 << 32) if q32 >= 1 << 31 else q32) and q32 > 1000
    imed = hri.valid_values(col, "IMED")
    if imed:
        assert hri.info_value(line, "IMED") == str(hri.median_by_hand(imed))
    fmed = hri.valid_values(col, "FMED")
    if fmed:
        assert _is_float_text(hri.info_value(line, "FMED"), hri.median_by_hand(fmed)), (hri.info_value(line, "FMED"), hri.median_by_hand(fmed))
    if "QUAL" in col:
        qual = hri.valid_values(col, "QUAL")
        text = line.split("\t")[5]
        assert (text == "." if not qual else _is_float_text(text, hri.median_by_hand(qual))), (text, hri.median_by_hand(qual))


@pytest.mark.parametrize("name", ["reducers_small", "reducers_2049"])
def test_oracle_and_kernel_bodies_on_reducer_columns(tmp_path, name):
    cells, q, facts = hri.CASES[name][0](tmp_path)
    ivs = hri.check_case(name, facts)
    for iv, col in zip(ivs, facts["columns"]):
        want = _both(q, cells, iv)
        check_reducer_text(want, col)
    if name == "reducers_small":
        zeros = facts["columns"][-4:]
        for col in zeros:                                                   # zeros of both signs around the middle
            v = sorted(x for x in col["FMED"])
            assert v[len(v) // 2] == 0 and any(str(x) == "-0.0" for x in v) and any(str(x) == "0.0" for x in v)


def test_fuzz_seeds_are_accepted_and_hot(tmp_path):
    """every seed of the GPU fuzz: the oracle and the kernel bodies agree, no seed hits a cap, the seeds together hold 30 and more hot
    records of which some but not all need the fallback"""
    huge = fallbacks = 0
    for seed in hri.FUZZ_SEEDS:
        d = tmp_path / ("s%d" % seed)
        d.mkdir()
        cells, q, facts = hri.fuzz(d, seed)
        hri.check_facts(facts)
        ivs = facts["intervals"]
        qa = hri.query_for_all(q, ivs)
        want, nrec, _ = helpers.oracle_run(qa, cells, with_header=False)       # one record per interval, in column order
        got, err = helpers.hostsim_run(qa, cells, with_header=False, rows_per_chunk=16, records_per_run=5)
        assert err == 0 and got == want and nrec == len(ivs)
        for iv, line in zip(ivs, want.splitlines(True)):
            col = iv["begin"]
            assert 25 <= iv["calls"][col] <= 80 and iv["distinct"][col] <= hri.MAX_MERGED_ALT and iv["huge_records"] == 1
            assert iv["merged_ref"][col] != ""                                  # a call starts here: the record's REF is its own
            hri.check_merged_lists(line, iv)
            huge += iv["huge_records"]
            fallbacks += iv["huge_fallbacks"]
    assert huge >= 30 and 1 <= fallbacks < huge


# ---- which code takes a median: the inputs of tests/test_gpu_median_paths.py ------------------------------------------------------------------
# The kernel bodies of this harness take every median with the per-thread scan of reduce_scalar (no MedianOrder, no BigMedians, no k_site_huge):
# what is pinned here is that scan, the predictions of every case and the by-hand medians - the other three paths only the GPU tests reach.
# NaN is in none of these inputs: the paths order it differently by construction (`<` against bit order) and the reference's nth_element on
# NaN is unspecified.
def check_median_columns(want, facts):
    by_pos = {int(l.split("\t", 2)[1]): l for l in want.decode().splitlines()}
    for pos, col in zip(facts["positions"], facts["columns"]):
        check_reducer_text(by_pos, col, pos)


def _zero_signs(values):
    return {str(v) for v in values if v == 0}


@pytest.mark.parametrize("name", list(hri.MEDIAN_CASES))
def test_oracle_and_kernel_bodies_on_median_path_inputs(tmp_path, name):
    """median_capacity takes 1.5 - 5 s (4097 sample files), median_list_overflow 6 - 10 s (210 000 input lines), nearly all of it input
    building: the oracle and the kernel bodies take half a second each.  Their sizes are the kernel's constants"""
    cells, q, facts = hri.MEDIAN_CASES[name][0](tmp_path)
    iv, = hri.check_case(name, facts)
    assert iv["begin"] == hri.HOT - 1 and len(facts["positions"]) == len(facts["columns"])
    want = _both(q, cells, iv)
    check_median_columns(want, facts)


def test_median_path_predictions_stand_on_the_thresholds(tmp_path):
    """the predictions, from the counts of the input lines alone: 48 / 49 calls, T = 16 P / 16 P + 1, 4096 / 4097 calls, 4096 + 4 records"""
    f = hri.median_path_facts
    assert f({0: 48, 1: 49, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1})["big_records"] == [1]
    assert f({0: 49, 1: 13, 2: 1, 3: 1}) == {"sorted": False, "big_records": [0], "big_listed": 1, "big_unlisted": 0}
    assert f({0: 49, 1: 13, 2: 1, 3: 2}) == {"sorted": True, "big_records": [], "big_listed": 0, "big_unlisted": 0}
    pad = {10 + j: 1 for j in range(545)}
    assert f({0: 4096, 1: 4097, **pad})["big_records"] == [0] and not f({0: 4096, 1: 4097, **pad})["sorted"]
    many = {j: 49 for j in range(4100)}
    many.update({5000 + j: 1 for j in range(9020)})
    assert sum(many.values()) == 16 * len(many)
    assert (f(many)["sorted"], f(many)["big_listed"], f(many)["big_unlisted"]) == (False, 4096, 4)
    many[5000] = 2
    assert f(many)["sorted"]
    for name in ("median_48_49", "median_average_16", "median_average_16_and_one_call", "median_sorted_single_record", "median_sorted_last_of_4_records"):
        (tmp_path / name).mkdir()
        cells, q, facts = hri.MEDIAN_CASES[name][0](tmp_path / name)
        iv, = hri.check_case(name, facts)
        hot = [iv["calls"][pos - 1] for pos in facts["positions"]]
        if name == "median_48_49":
            assert hot == [48, 49] and iv["big_records"] == [facts["positions"][1] - 1] and iv["heavy"] <= 16 * iv["num_records"]
        elif name.startswith("median_average_16"):
            assert hot == [49, 13] and iv["heavy"] - 16 * iv["num_records"] == (1 if name.endswith("one_call") else 0)
        elif name == "median_sorted_single_record":
            assert hot == [20] and iv["num_records"] == 1 and iv["huge_records"] == 0
        else:
            assert hot == [70] and iv["num_records"] == 4 and max(iv["calls"]) == facts["positions"][0] - 1 and iv["huge_records"] == 0


def test_median_value_columns_hold_what_their_names_say(tmp_path):
    cells, q, facts = hri.median_values(tmp_path)
    iv, = hri.check_case("median_values", facts)
    cols = dict(zip(hri.MEDIAN_VALUE_COLUMN_NAMES, facts["columns"]))
    assert len(cols) == len(facts["columns"]) == 13 and all(48 < iv["calls"][pos - 1] <= 64 for pos in facts["positions"])
    valid = lambda name, f: hri.valid_values(cols[name], f)            # noqa: E731
    for f in hri.MEDIAN_FIELDS:
        assert [len(valid(n, f)) for n in ("odd49", "even50", "even50_among_53", "all_equal", "one_valid", "none_valid")] == [49, 50, 50, 49, 1, 0]
        assert len(set(valid("all_equal", f))) == 1 and min(valid("odd49", f)) < hri.median_by_hand(valid("odd49", f))
    assert min(valid("odd49", "IMED")) < 0 and min(valid("even50", "FMED")) < 0
    ext = cols["extremes"]
    assert min(ext["IMED"]) == -2147483646 and max(ext["IMED"]) == 2147483647 and hri.median_by_hand(ext["IMED"]) == -2147483646 + 25
    assert min(ext["FMED"]) < -2.9e38 and 0 < -hri.median_by_hand(ext["FMED"]) < 1.1754944e-38 and 0 < hri.median_by_hand(ext["QUAL"]) < 1.1754944e-38
    assert all(hri.f32(v) == v for v in ext["FMED"] + ext["QUAL"])
    for f in ("FMED", "QUAL"):
        for name in ("zeros49", "zeros50", "zeros51"):                  # the middle lies in the run of zeros, both signs present
            v = sorted(valid(name, f))
            assert len(v) == int(name[5:]) and v[len(v) // 2] == 0 and _zero_signs(v) == {"0.0", "-0.0"}
        v = valid("both_zero_signs_beside_the_median", f)
        assert _zero_signs(v) == {"0.0", "-0.0"} and hri.median_by_hand(v) > 0
        assert _zero_signs(valid("zero_median_plus_only", f)) == {"0.0"} and hri.median_by_hand(valid("zero_median_plus_only", f)) == 0
        assert _zero_signs(valid("zero_median_minus_only", f)) == {"-0.0"} and hri.median_by_hand(valid("zero_median_minus_only", f)) == 0


def test_spanning_deletions_move_the_medians_under_the_wrong_rule(tmp_path):
    """INFO medians leave the deletions that began before the record out, the QUAL median counts them: in both records of median_spanning
    either median would be another one under the other field's rule, and the oracle prints the ones of the right rule"""
    cells, q, facts = hri.median_spanning(tmp_path)
    iv, = hri.check_case("median_spanning", facts)
    for pos, col, calls, valid in zip(facts["positions"], facts["columns"], (60, 62), (48, 50)):
        assert iv["calls"][pos - 1] == calls > hri.BIG_RECORD and len(col["spanning"]) == 12 and pos - 1 in iv["big_records"]
        assert len(hri.valid_values(col, "IMED")) == len(hri.valid_values(col, "FMED")) == valid and len(hri.valid_values(col, "QUAL")) == calls
        for f in hri.MEDIAN_FIELDS:
            everything = [v for v in col[f] if v is not None]
            starting_here = [v for row, v in enumerate(col[f]) if row not in col["spanning"]]
            assert hri.median_by_hand(everything) != hri.median_by_hand(starting_here)
            assert hri.median_by_hand(hri.valid_values(col, f)) == hri.median_by_hand(everything if f == "QUAL" else starting_here)
    assert len(hri.valid_values(facts["columns"][0], "IMED")) <= hri.BIG_RECORD
    want, _, _ = helpers.oracle_run(hri.query_for(q, iv), cells, with_header=False)
    check_median_columns(want, facts)
    assert facts["positions"][1] - 2 in iv["calls"] and iv["calls"][facts["positions"][1] - 2] == 12      # the deletions' own record


def test_grid_stride_and_overflow_inputs_have_distinct_medians(tmp_path):
    cells, q, facts = hri.median_grid_stride(tmp_path)
    iv, = hri.check_case("median_grid_stride", facts)
    assert len(iv["big_records"]) == 70 > 64
    for f in hri.MEDIAN_FIELDS:
        counts = [len(hri.valid_values(c, f)) for c in facts["columns"]]
        assert counts == [hri.GRID_STRIDE_VALID[i % 4] for i in range(70)]
        medians = [hri.median_by_hand(hri.valid_values(c, f)) for c in facts["columns"] if hri.valid_values(c, f)]
        assert len(set(medians)) == len(medians) and len({helpers.format_float(m) for m in medians}) == len(medians)
