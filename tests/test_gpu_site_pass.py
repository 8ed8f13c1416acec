"""The site pass (k_site_size / k_site_size_bcf, k_site_write, k_bcf_shared) on hand-made records, byte for byte against the oracle: the
places where its register-only number text, its packed 8-byte stores into the LDS strip and the tail slot, and the first-cell table of
site_first_ref can go wrong.  Inputs are small gVCFs made with the helpers of tests/hot_record_inputs.py (at most 64 samples, at most 300
columns an interval); site_pass_inputs() below builds each case once for the text and the BCF2 test."""
import gzip
import json
import os
import random
import struct

import pytest

import helpers
import hot_record_inputs as hri
from hot_record_inputs import Call

pytestmark = pytest.mark.gpu
ARENA = 1 << 22
HOT = hri.HOT
NULL_CHAR = 0x7F              # GDB_TILEDB_NULL_CHAR
KSITE_CAP, KSPILL_TAIL = 128, 512      # kSiteCap, kSpillTail (kernels/gdb_pipeline.hip, core/gdb_core.hpp)


class CallOn(Call):
    """a call on another contig than "1" """

    def __init__(self, chrom, *a, **kw):
        Call.__init__(self, *a, **kw)
        self.chrom = chrom

    def line(self, rnd):
        text = Call.line(self, rnd)
        assert text.startswith("1\t")
        return self.chrom + text[1:]


def fixed_columns(line):
    """bytes of CHROM .. FORMAT of one VCF line: what the site pass formats"""
    return len(b"\t".join(line.rstrip(b"\n").split(b"\t")[:9]))


def device_text(q, cells, begin, end, is_bcf=False):
    import bcf2text
    import genomicsdb_amd
    e = genomicsdb_amd.CombineEngine(q, is_bcf=is_bcf)
    try:
        e.stage_cells(cells)
        body, st = e.run_interval(begin, end, arena_bytes=ARENA, host_cap=ARENA)
        if is_bcf:
            h = bcf2text.Header(e.header.decode())
            at, lines = 0, []
            while at < len(body):
                l_shared, l_indiv = struct.unpack_from("<II", body, at)
                lines.append(bcf2text.record_to_text(h, body[at:at + 8 + l_shared + l_indiv], helpers.format_float))
                at += 8 + l_shared + l_indiv
            body = ("\n".join(lines) + "\n").encode()
        return body, st
    finally:
        e.close()


def oracle_text(q, cells, begin, end):
    return helpers.oracle_run(dict(q, query_column_ranges=[[[begin, end]]]), cells, with_header=False)[0]


def names(n, skip=0):
    """n distinct insertions behind G with distinct hashes (hot_record_inputs.distinct_alts' scheme)"""
    out, seen, i = [], set(), skip * 7
    while len(out) < n:
        a = "G" + "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(5))
        i += 1
        if hri.fixed_hash(a) not in seen:
            seen.add(hri.fixed_hash(a))
            out.append(a)
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def allele_counts(tmp_path):
    """one interval of 60 columns: records with 13, 14, 15 and 16 distinct ALT alleles (<NON_REF> aside), the 14 with a deletion from the
    column before among them ('*'), and plain reference records between them.  The site pass has ONE merged-allele table (128 entries): a
    16-entry table for short records would divide the records exactly here, but none is built, so these counts are no boundary of the
    code as it stands - they take the indexed path of merged_find_or_add (more than kMergeScan = 8 entries) in one launch with plain records."""
    nrows = 12
    samples = [[] for _ in range(nrows)]
    want = {}
    for j, n in enumerate((13, 14, 15, 16)):
        pos = HOT + 10 * j
        pool = names(n - (1 if n == 14 else 0), skip=j)
        row = 0
        if n == 14:
            samples[0].append(Call(pos - 1, "TGA", ["T"], hom_pl={1: 7}))       # covers pos: '*' there, first in the list (row 0)
            row = 1
        at = 0
        while at < len(pool):
            take = pool[at:at + 2]
            samples[row].append(Call(pos, "G", take, nr=row % 3 != 2))
            at += len(take)
            row += 1
        want[pos - 1] = n
        for r in range(nrows):
            if r % 4 == j:
                samples[r].append(Call(pos + 4, "C", []))                          # a plain reference record (ALT <NON_REF> alone)
    cells, q = hri._import(tmp_path, samples, 61)
    q["max_diploid_alt_alleles_that_can_be_genotyped"] = 50
    return cells, q, HOT - 2, HOT + 57, want


def fixed_column_lengths(tmp_path):
    """six records whose fixed columns take exactly 127 / 128 / 129 bytes (the LDS strip of the site pass holds 128) and 128 + 511 / 512 /
    513 (the record's tail slot holds 512): one insertion each, as long as it takes.  The first build measures, the second one hits."""
    targets = [KSITE_CAP - 1, KSITE_CAP, KSITE_CAP + 1, KSITE_CAP + KSPILL_TAIL - 1, KSITE_CAP + KSPILL_TAIL, KSITE_CAP + KSPILL_TAIL + 1]
    lengths = [20] * len(targets)
    for attempt in range(2):
        d = tmp_path / ("build%d" % attempt)
        d.mkdir()
        rnd = random.Random(5)
        samples = [[Call(HOT + 10 * j, "G", ["G" + "".join(rnd.choice("ACGT") for _ in range(lengths[j]))])] for j in range(len(targets))]
        cells, q = hri._import(d, samples, 62)
        lines = oracle_text(q, cells, HOT - 1, HOT + 10 * len(targets)).splitlines(True)
        assert len(lines) == len(targets)
        got = [fixed_columns(l) for l in lines]
        if attempt == 0:
            lengths = [lengths[j] + targets[j] - got[j] for j in range(len(targets))]
            assert min(lengths) > 0
    assert got == targets, got
    return cells, q, HOT - 1, HOT + 10 * len(targets), targets


BIG = "big"
BIG_OFFSET = 5_000_000_000          # above 2^32


def long_positions(tmp_path):
    """a contig at column offset 5 000 000 000 with reference blocks and variants at POS 12 345 678 / 123 456 789 / 1 234 567 890 and END
    = POS + 11: POS and END= of 8, 9 and 10 digits, from columns above 2^32"""
    vid = json.load(open(os.path.join(helpers.GOLDEN, "inputs", "vid.json")))
    vid["contigs"] = {"1": vid["contigs"]["1"], BIG: {"length": 2_000_000_000, "tiledb_column_offset": BIG_OFFSET}}
    vidp = str(tmp_path / "vid_big.json")
    with open(vidp, "w") as f:
        json.dump(vid, f)
    samples = [[], [], []]
    positions = [12_345_678, 123_456_789, 1_234_567_890, 99_999_989, 999_999_989]     # the last two: END crosses to one digit more
    for pos in positions:
        samples[0].append(CallOn(BIG, pos, "G", [], info={"END": str(pos + 11)}))
        samples[1].append(CallOn(BIG, pos + 3, "A", ["T"]))
        samples[2].append(CallOn(BIG, pos, "G", ["C", "GT"]))
    cells, q = _import_with_vid(tmp_path, samples, 63, vidp)
    return cells, q, positions


def _import_with_vid(tmp_path, samples, seed, vidp):
    """hot_record_inputs._import with another vid mapping (the header gets the contig's line)"""
    import genomicsdb_amd
    cells, q = hri._import(tmp_path, [[] for _ in samples], seed)      # the query's skeleton and the callset files' places
    rnd = random.Random(seed)
    head = hri._head().replace("#CHROM", "##contig=<ID=%s,length=2000000000>\n#CHROM" % BIG)
    for row, calls in enumerate(samples):
        with gzip.open(tmp_path / ("s%d.vcf.gz" % row), "wt", compresslevel=1) as f:
            f.write(head.replace("@SAMPLE@", "S%05d" % row) + "".join(c.line(rnd) for c in sorted(calls, key=lambda c: c.pos)))
    cells, ncells = genomicsdb_amd.import_cells(vidp, q["callset_mapping_file"])
    assert ncells == sum(len(s) for s in samples)
    q = dict(q, vid_mapping_file=vidp)
    del q["reference_genome"]
    return cells, q


def first_record_without_a_cell(tmp_path, null_refs=False):
    """row 0: a reference block HOT - 20 .. HOT + 20; the interval begins at HOT, in the middle of it, where no cell begins: the first record's
    base comes from the reference genome; more records follow where one, two and no cells begin.  null_refs: at HOT + 5 and HOT + 9 two
    cells begin, and the lowest row's REF is taken out of the cells (TileDB null characters)."""
    samples = [[Call(HOT - 20, "G", [], info={"END": str(HOT + 20)})],
               [Call(HOT + 5, "C", ["T"])],
               [Call(HOT + 5, "CA", ["C", "CAT"]), Call(HOT + 9, "A", ["G"])],
               [Call(HOT + 9, "A", ["T"])]]
    cells, q = hri._import(tmp_path, samples, 64)
    if null_refs:
        cells = without_ref(cells, row=1, col=HOT + 5 - 1)
        cells = without_ref(cells, row=2, col=HOT + 9 - 1)
    return cells, q, HOT - 1, HOT + 30


def without_ref(cells, row, col):
    """the cells with the REF of cell (row, col) overwritten by TileDB null characters (layout: tests/tools/cells2csv.py)"""
    out, at, hit = bytearray(cells), 0, 0
    while at < len(out):
        r, c, size = struct.unpack_from("<qqQ", out, at)
        if (r, c) == (row, col):
            (n,) = struct.unpack_from("<i", out, at + 32)
            out[at + 36:at + 36 + n] = bytes([NULL_CHAR]) * n
            hit += 1
        at += size
    assert hit == 1 and at == len(out)
    return bytes(out)


_made = {}


def site_pass_inputs(name, tmp_path_factory):
    if name not in _made:
        _made[name] = {"allele_counts": allele_counts, "fixed_column_lengths": fixed_column_lengths, "long_positions": long_positions,
                       "first_record_without_a_cell": first_record_without_a_cell,
                       "first_cell_without_ref": lambda t: first_record_without_a_cell(t, null_refs=True)}[name](tmp_path_factory.mktemp(name))
    return _made[name]


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
def test_records_of_13_to_16_distinct_alleles_in_one_interval(tmp_path_factory):
    cells, q, begin, end, want = site_pass_inputs("allele_counts", tmp_path_factory)
    text = oracle_text(q, cells, begin, end)
    recs = {int(f[1]) - 1: f for f in hri.record_lines(text)}
    for col, n in want.items():
        alts = recs[col][4].split(",")
        assert len([a for a in alts if a != "<NON_REF>"]) == n, (col, alts)
    assert "*" in recs[HOT + 10 - 1][4].split(",") and recs[HOT + 10 - 1][4].split(",")[0] == "*"
    assert sum(1 for f in recs.values() if f[4] == "<NON_REF>") >= 4             # the plain records among them
    got, st = device_text(q, cells, begin, end)
    assert got == text
    assert st.huge_records == 0


def test_fixed_columns_at_the_ends_of_the_strip_and_of_the_tail_slot(tmp_path_factory):
    cells, q, begin, end, targets = site_pass_inputs("fixed_column_lengths", tmp_path_factory)
    text = oracle_text(q, cells, begin, end)
    assert [fixed_columns(l) for l in text.splitlines(True)] == [127, 128, 129, 639, 640, 641] == targets
    got, _ = device_text(q, cells, begin, end)
    assert got == text


def test_pos_and_end_of_8_9_and_10_digits_above_column_2_32(tmp_path_factory):
    cells, q, positions = site_pass_inputs("long_positions", tmp_path_factory)
    assert BIG_OFFSET > 2**32
    for pos in positions:
        begin, end = BIG_OFFSET + pos - 1 - 2, BIG_OFFSET + pos - 1 + 20
        text = oracle_text(q, cells, begin, end)
        recs = hri.record_lines(text)
        assert all(f[0] == BIG for f in recs) and str(pos) in [f[1] for f in recs]
        ends = [kv[4:] for f in recs for kv in f[7].split(";") if kv.startswith("END=")]
        assert ends and all(len(e) in (8, 9, 10) for e in ends)
        got, _ = device_text(q, cells, begin, end)
        assert got == text, pos
    digits = {len(str(p)) for p in positions} | {len(str(p + 11)) for p in positions}
    assert digits == {8, 9, 10}


def test_first_record_where_no_cell_begins(tmp_path_factory):
    cells, q, begin, end = site_pass_inputs("first_record_without_a_cell", tmp_path_factory)
    text = oracle_text(q, cells, begin, end)
    recs = hri.record_lines(text)
    assert int(recs[0][1]) == HOT and recs[0][3] in ("A", "C", "G", "T") and recs[0][4] == "<NON_REF>"     # the genome's base
    by_pos = {int(f[1]): f for f in recs}
    assert by_pos[HOT + 5][3] == "CA" and by_pos[HOT + 9][3] == "A" and HOT + 6 in by_pos and HOT + 7 in by_pos
    got, _ = device_text(q, cells, begin, end)
    assert got == text


def test_first_cell_of_a_record_without_a_valid_ref(tmp_path_factory):
    """The lowest-row cell that begins at a record has a REF of TileDB null characters.  The reference never asks whether a REF is valid
    (merge_reference_allele appends whatever the string holds), and the oracle follows it, so for such a cell - which no importer writes -
    the oracle's text is not what the kernel bodies print, with the first-cell table or without it: the bodies skip the cell's REF.  The
    device (table) is therefore held to the bodies on the CPU (tests/hostsim: site_first_ref's binary search), byte for byte."""
    cells, q, begin, end = site_pass_inputs("first_cell_without_ref", tmp_path_factory)
    qi = dict(q, query_column_ranges=[[[begin, end]]])
    want = helpers.hostsim_run(qi, cells, with_header=False)
    want = want[0] if isinstance(want, tuple) else want
    by_pos = {int(f[1]): f for f in hri.record_lines(want)}
    assert by_pos[HOT + 5][3] == "CA" and by_pos[HOT + 9][3] == "A"        # the other call's REF
    got, _ = device_text(q, cells, begin, end)
    assert got == want


@pytest.mark.parametrize("name", ["allele_counts", "fixed_column_lengths", "first_record_without_a_cell"])
def test_the_same_intervals_as_bcf2(tmp_path_factory, name):
    made = site_pass_inputs(name, tmp_path_factory)
    cells, q, begin, end = made[:4]
    text = oracle_text(q, cells, begin, end)
    got, _ = device_text(q, cells, begin, end, is_bcf=True)
    assert got == text
