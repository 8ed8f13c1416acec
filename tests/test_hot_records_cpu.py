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


def check_reducer_text(want, col):
    """what is known by hand about the reducers of one column, on the oracle's line"""
    line = want.decode().splitlines()[0]
    fsum = [v for v in col["FSUM"] if v is not None]
    if fsum and fsum[:4] == hri.order_dependent_floats(4):
        in_order, by_size = hri.float32_sum(fsum), hri.float32_sum(sorted(fsum))
        assert in_order != by_size                                          # otherwise the input proves nothing
        assert hri.info_value(line, "FSUM") == helpers.format_float(in_order) != helpers.format_float(by_size)
    for f in hri.REDUCER_FIELDS:
        if all(v is None for v in col[f]):
            assert hri.info_value(line, f) is None
    isum = [v for v in col["ISUM"] if v is not None]
    if isum:
        assert hri.info_value(line, "ISUM") == str(sum(isum))
    imean = [v for v in col["IMEAN"] if v is not None]
    if imean and sum(imean) < 0:                                            # the reference's int / unsigned
        q32 = (sum(imean) & 0xFFFFFFFF) // len(imean)
        assert hri.info_value(line, "IMEAN") == str(q32 - (1 << 32) if q32 >= 1 << 31 else q32) and q32 > 1000
    imed = sorted(v for v in col["IMED"] if v is not None)
    if imed:
        assert hri.info_value(line, "IMED") == str(imed[len(imed) // 2])
    fmed = sorted(v for v in col["FMED"] if v is not None)
    if fmed:
        assert float(hri.info_value(line, "FMED")) == fmed[len(fmed) // 2]  # (the sign of a tied zero: the bytes of the kernel bodies)


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
