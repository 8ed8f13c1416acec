"""Hand-made cells for the records the workgroup-per-record site kernel (k_site_huge, kernels/gdb_pipeline.hip) takes: small gVCFs, one
per sample, turned into cells by the host importer like tests/test_many_input_alleles.py does (same header, same query).  A single-column
interval on a site where 25 samples start a variant has P = 1 record and T = 25 calls, so T / P >= 24 and the record is "huge": everything the
kernel does - merged REF, the allele merge through its 512-slot hash table keyed by allele_hash, the LUTs / spanning-deletion flags / min-PL
genotypes, the scalar INFO reducers - is reachable with a few dozen samples, the table's fallbacks included.

Every builder returns (cells, query, facts).  facts["intervals"] is a list of dicts, one per column interval a test runs:
  begin, end            the interval's columns (0-based: POS - 1)
  calls                 {column: variant calls live at that record} for the hot records of the interval
  distinct              {column: distinct merged ALT alleles (without <NON_REF>)}
  merged_alt            {column: the merged ALT list derived here from the input lines, <NON_REF> included}
  merged_ref            {column: merged REF}
  num_records, heavy    IntervalStats.num_records / num_heavy_incidences the interval must report
  huge_records, huge_fallbacks   the counters of the default mode
  sorted, big_records, big_listed, big_unlisted   which code takes the medians (median_path_facts)
A test asserts the facts it states by hand against these before it compares any bytes (check_facts does the part every case shares)."""
import gzip
import json
import os
import random
from math import comb

import helpers
from test_many_input_alleles import _header

MASK = 0xFFFFFFFF
HUGE_TABLE = 512          # kHugeTable
HUGE_EMPTY = 0xFFFFFFFF   # kHugeEmpty
MAX_MERGED_ALT = 126      # GDB_MAX_MERGED_ALLELES = 128 with REF and <NON_REF> (gdb_core.hpp: find_or_add_merged)


def allele_hash(text):
    """allele_hash of core/gdb_core.hpp (FNV-1a, 32 bit) over the allele's text with the merged REF's suffix already appended"""
    h = 2166136261
    for ch in text.encode():
        h = ((h ^ ch) * 16777619) & MASK
    return h


def fixed_hash(text):
    """huge_fix_hash: the table's empty marker is no key"""
    h = allele_hash(text)
    return 0xFFFFFFFE if h == HUGE_EMPTY else h


EQUAL_LENGTH_PAIR = ("CTGGTCGA", "AGCGTCCT")
UNEQUAL_LENGTH_PAIR = ("TGGACCG", "GATTCAGC")
SECOND_PAIR = ("AGCGTCCA", "CTGGTCGT")
MARKER_ALLELE = "GGTTAAAGCAACAA"
MARKER_REMAP_PAIR = ("TCTTGACTACGGTATT", "TTTACGTCTGGATTAA")
# a change of the hash function makes every colliding input an ordinary one: fail here, loudly, instead of testing nothing
assert allele_hash("CTGGTCGA") == allele_hash("AGCGTCCT") == 0x36953CC5
assert allele_hash("TGGACCG") == allele_hash("GATTCAGC") == 0x17F7EBBB
assert allele_hash("AGCGTCCA") == allele_hash("CTGGTCGT") == 0x41954E16
assert allele_hash(MARKER_ALLELE) == 0xFFFFFFFF
assert allele_hash("TCTTGACTACGGTATT") == allele_hash("TTTACGTCTGGATTAA") == 0xFFFFFFFE
assert fixed_hash(MARKER_ALLELE) == fixed_hash(MARKER_REMAP_PAIR[0])

GDB_ERR_TOO_MANY_MERGED_ALLELES = 1 << 1      # core/gdb_types.h
TOO_MANY_MERGED_TEXT = "more than GDB_MAX_MERGED_ALLELES alleles in one record"

REDUCER_FIELDS = {"ISUM": ("int", "sum"), "IMEAN": ("int", "mean"), "IMED": ("int", "median"),
                  "FSUM": ("float", "sum"), "FMEAN": ("float", "mean"), "FMED": ("float", "median")}


def n_genotypes(n_alleles, ploidy):
    return comb(n_alleles + ploidy - 1, ploidy)


def hom_index(a, ploidy):
    """index of the genotype a/a/../a in the VCF order of the PL vector"""
    return sum(comb(a + k - 1, k) for k in range(1, ploidy + 1))


class Call:
    """one gVCF line of one sample (the sample's row is its place in the list a builder hands to _import)"""

    def __init__(self, pos, ref, alts, nr=True, ploidy=2, pl=True, info=None, hom_pl=None, filt=".", qual="100"):
        self.pos, self.ref, self.alts, self.nr, self.ploidy, self.pl, self.info, self.hom_pl, self.filt, self.qual = \
            pos, ref, list(alts), nr, ploidy, pl, info or {}, hom_pl or {}, filt, qual      # qual: the column's text ("." is a missing QUAL)

    def is_symbolic(self, a):
        return a == "*" or (a.startswith("<") and a.endswith(">")) or "[" in a or "]" in a

    def has_deletion(self):
        return len(self.ref) > 1 and any(not self.is_symbolic(a) and len(a) < len(self.ref) for a in self.alts)

    def end(self):
        return self.pos + len(self.ref) - 1

    def line(self, rnd):
        alleles = self.alts + (["<NON_REF>"] if self.nr else [])
        na = len(alleles) + 1
        ad = [rnd.randint(0, 60) for _ in range(na)]
        gt = "/".join(str(x) for x in sorted(rnd.randint(0, len(self.alts)) for _ in range(self.ploidy)))
        fmt, val = ["GT", "AD", "DP", "GQ"], [gt, ",".join(map(str, ad)), str(sum(ad)), str(rnd.randint(0, 99))]
        if self.pl:
            ng = n_genotypes(na, self.ploidy)
            pl = [rnd.randint(100, 3000) for _ in range(ng)]
            pl[rnd.randrange(ng)] = 50
            for a, v in self.hom_pl.items():
                pl[hom_index(a, self.ploidy)] = v
            fmt.append("PL")
            val.append(",".join(map(str, pl)))
        info = ["DP=%d" % sum(ad), "MQ=40.5"] + ["%s=%s" % kv for kv in self.info.items()]
        return "1\t%d\t.\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n" % (self.pos, self.ref, ",".join(alleles), self.qual, self.filt, ";".join(info), ":".join(fmt), ":".join(val))


def live_index(samples):
    """{pos: [(row, call) live there, in row order]}: what merge_at finds call by call, for inputs of many columns"""
    index = {}
    for row, calls in enumerate(samples):
        for c in calls:
            for pos in range(c.pos, (c.end() if c.has_deletion() else c.pos) + 1):
                index.setdefault(pos, []).append((row, c))
    return index


def merge_at(samples, pos, index=None):
    """(calls live at pos in row order, merged REF, merged ALT list without <NON_REF>, any <NON_REF>) as merge_alt_alleles leaves them:
    the longest REF among the calls that start at pos (the lowest row at equal length); every ALT extended by the part of the merged REF
    its own REF lacks, symbolic ones as they are, a deletion that began earlier as '*'; first appearance in (row, token) order"""
    live = []
    if index is not None:
        live = index.get(pos, [])
    else:
        for row, calls in enumerate(samples):
            for c in calls:
                if c.pos == pos or (c.pos < pos <= c.end() and c.has_deletion()):
                    live.append((row, c))
    mref = ""
    for row, c in live:
        if c.pos == pos and len(c.ref) > len(mref):
            mref = c.ref
    merged, any_nr = [], False
    for row, c in live:
        any_nr |= c.nr
        ext = ["*"] if c.pos < pos else [a if c.is_symbolic(a) else a + mref[len(c.ref):] for a in c.alts]
        for a in ext:
            if a not in merged:
                merged.append(a)
    return live, mref, merged, any_nr


def expects_fallback(merged):
    """what sends a record of k_site_huge back to the serial walk: two different alleles with one (fixed) hash, or more distinct hashes than
    the table has slots"""
    hashes = [fixed_hash(a) for a in merged]
    return len(set(hashes)) < len(hashes) or len(set(hashes)) > HUGE_TABLE


def huge_threshold(T, P):
    return 24 if (P > 0 and T // P >= 24 and P <= 8192) else 256


SORTED_MEDIAN_THRESHOLD = 16    # kSortedMedianThreshold
BIG_RECORD = 48                 # kBigRecord
BIG_CAPACITY = 4096             # kBigCapacity
MAX_BIG_RECORDS = 4096          # kMaxBigRecords


def median_path_facts(calls):
    """which code takes the medians of an interval whose records have calls = {column: variant calls}: every median field is ordered by one
    device-wide sort when the interval averages more than 16 calls a record (T > 16 P); otherwise the records with 49 .. 4096 calls are
    listed for one workgroup each (k_big_records / k_big_medians), the first 4096 of them"""
    P, T = len(calls), sum(calls.values())
    is_sorted = T > SORTED_MEDIAN_THRESHOLD * P
    big = [] if is_sorted else sorted(col for col, n in calls.items() if BIG_RECORD < n <= BIG_CAPACITY)
    return {"sorted": is_sorted, "big_records": big, "big_listed": min(len(big), MAX_BIG_RECORDS), "big_unlisted": max(len(big) - MAX_BIG_RECORDS, 0)}


def interval_facts(samples, begin_pos, end_pos):
    """the facts of the column interval [begin_pos - 1, end_pos - 1], derived from the input lines alone"""
    starts = sorted({c.pos for calls in samples for c in calls if begin_pos <= c.pos <= end_pos} | {begin_pos})
    index = live_index(samples)
    recs = {}
    for pos in starts:
        live, mref, merged, any_nr = merge_at(samples, pos, index)
        if live:
            recs[pos] = (live, mref, merged, any_nr)
    P, T = len(recs), sum(len(r[0]) for r in recs.values())
    thr = huge_threshold(T, P)
    hot = {pos: r for pos, r in recs.items() if len(r[0]) > thr}
    return {**median_path_facts({pos - 1: len(r[0]) for pos, r in recs.items()}),
            "begin": begin_pos - 1, "end": end_pos - 1, "num_records": P, "heavy": T, "threshold": thr,
            "calls": {pos - 1: len(r[0]) for pos, r in recs.items()},
            "distinct": {pos - 1: len(r[2]) for pos, r in recs.items()},
            "merged_ref": {pos - 1: r[1] for pos, r in recs.items()},
            "merged_alt": {pos - 1: r[2] + (["<NON_REF>"] if r[3] else []) for pos, r in recs.items()},
            "huge_records": len(hot),
            "huge_fallbacks": sum(1 for r in hot.values() if expects_fallback(r[2]))}


def check_facts(facts):
    """no interval of a case is empty, and every interval says what it expects"""
    assert facts["intervals"]
    for iv in facts["intervals"]:
        assert iv["num_records"] >= 1 and iv["heavy"] == sum(iv["calls"].values())
        assert 0 <= iv["huge_fallbacks"] <= iv["huge_records"] <= iv["num_records"]
        assert iv["big_listed"] + iv["big_unlisted"] == len(iv["big_records"]) <= iv["num_records"] and not (iv["sorted"] and iv["big_records"])


_head_text = None


def _head():
    """the header of test_many_input_alleles' inputs (without the one line that is most of its bytes), the sample's name left open"""
    global _head_text
    if _head_text is None:
        _head_text = "".join(l for l in _header("@SAMPLE@").splitlines(True) if not l.startswith("##GATKCommandLine"))
    return _head_text


def _import(tmp_path, samples, seed, reducers=False, attributes=None, reference=True, qual_median=False):
    """samples[row] = [Call, ...] -> (cells, query): one .vcf.gz per sample through the host importer.  reference=False: the query names no
    reference genome (every record of the case has a call that starts at it and brings its REF along; the oracle reads the genome anew on
    every run, a tenth of a second).  qual_median: the vid gives QUAL the median reducer and the query asks for QUAL"""
    import genomicsdb_amd
    rnd = random.Random(seed)
    vid = os.path.join(helpers.GOLDEN, "inputs", "vid.json")
    extra = ""
    if reducers:
        v = json.load(open(vid))
        for name, (typ, op) in REDUCER_FIELDS.items():
            v["fields"][name] = {"vcf_field_class": ["INFO"], "type": typ, "VCF_field_combine_operation": op}
            extra += '##INFO=<ID=%s,Number=1,Type=%s,Description="x">\n' % (name, "Integer" if typ == "int" else "Float")
        if qual_median:
            v["fields"]["QUAL"] = {"type": "float", "VCF_field_combine_operation": "median"}
        vid = str(tmp_path / "vid.json")
        with open(vid, "w") as f:
            json.dump(v, f)
    callsets = {"callsets": {}}
    ncalls = 0
    head = _head().replace("#CHROM", extra + "#CHROM")
    for row, calls in enumerate(samples):
        name = "S%05d" % row
        p = tmp_path / ("s%d.vcf.gz" % row)
        with gzip.open(p, "wt", compresslevel=1) as f:
            f.write(head.replace("@SAMPLE@", name) + "".join(c.line(rnd) for c in sorted(calls, key=lambda c: c.pos)))
        ncalls += len(calls)
        callsets["callsets"][name] = {"row_idx": row, "idx_in_file": 0, "filename": str(p)}
    cs = tmp_path / "callsets.json"
    cs.write_text(json.dumps(callsets))
    cells, ncells = genomicsdb_amd.import_cells(vid, str(cs))
    assert ncells == ncalls
    attrs = attributes or ["REF", "ALT", "DP", "MQ", "GT", "AD", "GQ", "PL", "DP_FORMAT", "MIN_DP"]
    if reducers:
        attrs = attrs + list(REDUCER_FIELDS) + (["QUAL"] if qual_median else [])
    q = {"vid_mapping_file": vid, "callset_mapping_file": str(cs),
         "vcf_header_filename": os.path.join(helpers.GOLDEN, "inputs", "template_vcf_header.vcf"),
         "reference_genome": os.path.join(helpers.GOLDEN, "inputs", "chr1_10MB.fasta.gz"),
         "query_column_ranges": [[[0, 1_000_000_000]]], "query_row_ranges": [{"range_list": [{"low": 0, "high": len(samples) - 1}]}],
         "attributes": attrs, "produce_GT_field": True}
    if not reference:
        del q["reference_genome"]
    return cells, q


def query_for(q, iv):
    """the query of one interval of a case"""
    return dict(q, query_column_ranges=[[[iv["begin"], iv["end"]]]])


def query_for_all(q, ivs):
    """one query over all intervals of a case: their records one after the other"""
    return dict(q, query_column_ranges=[[[iv["begin"], iv["end"]] for iv in ivs]])


def _pool(rnd, n, anchor="G", lo=1, hi=6):
    """n distinct insertions behind the anchor base, none with a hash another one has"""
    out, seen = [], set()
    while len(out) < n:
        a = anchor + "".join(rnd.choice("ACGT") for _ in range(rnd.randint(lo, hi)))
        if a not in out and fixed_hash(a) not in seen and fixed_hash(a + "A") not in seen:
            out.append(a)
            seen.add(fixed_hash(a))
    return out


HOT = 20100      # POS of the hot record of the single-record cases


# ---- selection -------------------------------------------------------------------------------------------------------------------------
def selection_single(tmp_path, ncalls):
    """one record with ncalls SNV calls: 24 is not huge, 25 is (T / P >= 24 and n > 24)"""
    samples = [[Call(HOT, "G", [["T"], ["C"], ["A", "T"]][row % 3])] for row in range(ncalls)]
    cells, q = _import(tmp_path, samples, ncalls)
    return cells, q, {"intervals": [interval_facts(samples, HOT, HOT)]}


def selection_absolute_threshold(tmp_path):
    """30 records: one with 257 calls, one with 256, 28 with 3 - on average fewer than 24 calls a record, so only more than 256 calls count"""
    samples = [[] for _ in range(257)]
    for row in range(257):
        samples[row].append(Call(HOT, "G", [["T"], ["C"], ["A", "T"]][row % 3]))
        if row < 256:
            samples[row].append(Call(HOT + 10, "A", [["T"], ["C"]][row % 2]))
        if row < 3:
            for j in range(28):
                samples[row].append(Call(HOT + 20 + 2 * j, "C", ["T"]))
    cells, q = _import(tmp_path, samples, 257)
    return cells, q, {"intervals": [interval_facts(samples, HOT, HOT + 20 + 2 * 27)]}


# ---- allele merge ------------------------------------------------------------------------------------------------------------------------
def first_appearance(tmp_path, seed=11):
    """40 calls that list 1-3 of 30 insertions in permuted orders, every fourth call without <NON_REF>"""
    rnd = random.Random(seed)
    pool = _pool(rnd, 30)
    samples = [[Call(HOT, "G", rnd.sample(pool, rnd.randint(1, 3)), nr=row % 4 != 1)] for row in range(40)]
    cells, q = _import(tmp_path, samples, seed)
    return cells, q, {"intervals": [interval_facts(samples, HOT, HOT)], "pool": pool}


def suffix_extension(tmp_path):
    """REFs G, GA, GAC, GACT (and GACA in a higher row: a tie for the longest) at one column; TACT written as T under G, TA under GA, TAC
    under GAC and TACT under GACT; a symbolic ALT that takes no suffix"""
    forms = [("G", ["T"]), ("GACT", ["TACT", "<DEL>"]), ("GACA", ["GACAT"]), ("GAC", ["TAC", "TCT"]), ("GA", ["TA", "GAA"]),
             ("G", ["C", "T"]), ("GACT", ["GACTT"]), ("GAC", ["TCT"]), ("GA", ["CA"]), ("G", ["GT"])]
    samples = [[Call(HOT, *forms[row % len(forms)], nr=row % 5 != 2)] for row in range(30)]
    cells, q = _import(tmp_path, samples, 12)
    facts = {"intervals": [interval_facts(samples, HOT, HOT)],
             "by_hand_ref": "GACT",        # rows 1 and 2 tie at four bases: the lower row's text
             # row 0: T+ACT; row 1: TACT (known), <DEL> as it is; row 2: GACAT (its REF is as long as the merged one: no suffix);
             # row 3: TAC+T (known), TCT+T; row 4: TA+CT (known), GAA+CT; row 5: C+ACT, T+ACT (known); row 6: GACTT; row 7: TCT+T (known);
             # row 8: CA+CT (known: row 5's); row 9: GT+ACT
             "by_hand_alt": ["TACT", "<DEL>", "GACAT", "TCTT", "GAACT", "CACT", "GACTT", "GTACT", "<NON_REF>"]}
    return cells, q, facts


def _with_specials(tmp_path, seed, specials, ncalls=30, at=(7, 19), second_column=False):
    """ncalls calls with 1-2 of 12 ordinary insertions each; call at[i] carries specials[i] = (REF, ALT) as well.  second_column: the same
    ordinary calls once more ten columns on, without the specials (a hot record that needs no fallback)"""
    rnd = random.Random(seed)
    pool = _pool(rnd, 12)
    samples = []
    for row in range(ncalls):
        alts = rnd.sample(pool, rnd.randint(1, 2))
        ref = "G"
        if row in at[:len(specials)]:
            ref, a = specials[at.index(row)]
            alts = [x + ref[1:] for x in alts]           # the same ordinary alleles under the longer REF
            alts.insert(rnd.randint(0, len(alts)), a)
        samples.append([Call(HOT, ref, alts)])
        if second_column:
            samples[row].append(Call(HOT + 10, "G", rnd.sample(pool, rnd.randint(1, 2))))
    cells, q = _import(tmp_path, samples, seed)
    return cells, q, {"intervals": [interval_facts(samples, HOT, HOT + (10 if second_column else 0))], "pool": pool}


def collision_equal_length(tmp_path):
    return _with_specials(tmp_path, 21, [("G", EQUAL_LENGTH_PAIR[0]), ("G", EQUAL_LENGTH_PAIR[1])])


def collision_unequal_length(tmp_path):
    return _with_specials(tmp_path, 22, [("G", UNEQUAL_LENGTH_PAIR[0]), ("G", UNEQUAL_LENGTH_PAIR[1])])


def collision_after_extension(tmp_path):
    """CTGGTCG under REF G becomes CTGGTCGA under the merged REF GA and only then shares its hash with AGCGTCCT (REF GA)"""
    return _with_specials(tmp_path, 23, [("G", "CTGGTCG"), ("GA", "AGCGTCCT")])


def collision_in_one_of_two_records(tmp_path):
    return _with_specials(tmp_path, 24, [("G", SECOND_PAIR[0]), ("G", SECOND_PAIR[1])], second_column=True)


def marker_hash_alone(tmp_path):
    return _with_specials(tmp_path, 25, [("G", MARKER_ALLELE)])


def marker_hash_with_remap_target(tmp_path):
    return _with_specials(tmp_path, 26, [("G", MARKER_ALLELE), ("G", MARKER_REMAP_PAIR[0])])


def distinct_alts(tmp_path, ncalls, ndistinct):
    """ncalls calls with one ALT each, ndistinct different ones (the calls behind the ndistinct-th repeat the first ones)"""
    names = []
    i = 0
    seen = set()
    while len(names) < ndistinct:       # G + the number in base 4, five letters: distinct by construction; distinct hashes checked
        a = "G" + "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(5))
        i += 1
        if fixed_hash(a) not in seen:
            seen.add(fixed_hash(a))
            names.append(a)
    samples = [[Call(HOT, "G", [names[row % ndistinct]], pl=False)] for row in range(ncalls)]
    cells, q = _import(tmp_path, samples, ndistinct)
    q["max_diploid_alt_alleles_that_can_be_genotyped"] = 50
    return cells, q, {"intervals": [interval_facts(samples, HOT, HOT)]}


def spanning_deletions(tmp_path, min_pl_gt, seed=31):
    """48 calls: 24 deletions that begin one column earlier and cover the hot column - two or three deletion alleles each, the lowest hom-PL
    on the second one - and 24 calls that start there; with and without <NON_REF>, with and without PL, ploidy 1, 2 and 3 in every
    combination on both kinds"""
    rnd = random.Random(seed)
    pool = _pool(rnd, 8, anchor="G")
    combos = [(nr, pl, ploidy) for nr in (True, False) for pl in (True, False) for ploidy in (1, 2, 3)]
    samples = []
    for row in range(48):
        nr, pl, ploidy = combos[(row // 2) % 12]
        if row % 2 == 0:
            alts = [["T", "TG", "TGAA"], ["TG", "T"], ["TGAC", "TG", "T"]][(row // 2) % 3]
            second_del = [a for a in range(1, len(alts) + 1) if len(alts[a - 1]) < 3][1]
            samples.append([Call(HOT - 1, "TGA", alts, nr=nr, ploidy=ploidy, pl=pl, hom_pl={second_del: 7})])
        else:
            samples.append([Call(HOT, "G", rnd.sample(pool, rnd.randint(1, 2)), nr=nr, ploidy=ploidy, pl=pl)])
    cells, q = _import(tmp_path, samples, seed)
    q["produce_GT_with_min_PL_value_for_spanning_deletions"] = bool(min_pl_gt)
    return cells, q, {"intervals": [interval_facts(samples, HOT, HOT)]}


# ---- reducers ------------------------------------------------------------------------------------------------------------------------------
def _fmt(v):
    if isinstance(v, float):
        return repr(v) if v != int(v) or abs(v) >= 1e15 else ("-" if str(v)[0] == "-" else "") + "%d.0" % abs(int(v))
    return str(v)


def reducer_columns(tmp_path, columns, seed=41):
    """columns: [{field: [value or None per call]}]; column i is POS HOT + 10 i, its calls are rows 0 .. len - 1 (one SNV each)"""
    nrows = max(len(next(iter(col.values()))) for col in columns)
    samples = [[] for _ in range(nrows)]
    for i, col in enumerate(columns):
        n = len(next(iter(col.values())))
        assert all(len(v) == n for v in col.values())
        for row in range(n):
            info = {f: _fmt(v[row]) for f, v in col.items() if v[row] is not None}
            samples[row].append(Call(HOT + 10 * i, "G", ["T"], pl=False, info=info))
    cells, q = _import(tmp_path, samples, seed, reducers=True, attributes=["REF", "ALT", "GT", "DP"], reference=False)
    return cells, q, {"intervals": [interval_facts(samples, HOT + 10 * i, HOT + 10 * i) for i in range(len(columns))], "columns": columns}


def order_dependent_floats(n):
    """1e8, 1, -1e8, 1 over and over (and 0.5 behind the last full group): in float arithmetic 1e8 + 1 is 1e8, so every group leaves the sum
    in call order at 1, while the sorted values cancel to 0 - the ones are lost in the negative figures first"""
    return [(1e8, 1.0, -1e8, 1.0)[i % 4] if i < n - n % 4 else 0.5 for i in range(n)]


def float32_sum(values):
    import numpy as np
    s = np.float32(0)
    for v in values:
        s = np.float32(s + np.float32(v))
    return float(s)


def info_value(text_line, name):
    for kv in text_line.split("\t")[7].split(";"):
        if kv.startswith(name + "="):
            return kv[len(name) + 1:]
    return None


# ---- seeded fuzz -----------------------------------------------------------------------------------------------------------------------------
def fuzz(tmp_path, seed):
    """1-4 hot columns of 25-80 calls: REF lengths 1-4, 1-4 ALTs out of a pool that holds the colliding pair AGCGTCCA / CTGGTCGT at about
    a third of the columns and one allele of it at the others, ploidy 1-3,
    missing PL / <NON_REF>, and deletions that begin one column before a hot column"""
    rnd = random.Random(1000 + seed)
    plain = _pool(rnd, 14, anchor="", lo=1, hi=5)
    ncols = rnd.randint(1, 4)
    nrows = 80
    samples = [[] for _ in range(nrows)]
    refs = ["G", "GA", "GAC", "GACT"]
    for i in range(ncols):
        pos = HOT + 20 * i
        rows = rnd.sample(range(nrows), rnd.randint(25, 80))
        pool = plain + list(SECOND_PAIR[:2 if rnd.random() < 0.3 else 1])      # about a third of the columns can see both alleles of the pair
        for row in rows:
            ploidy, nr, pl = rnd.randint(1, 3), rnd.random() < 0.8, rnd.random() < 0.7
            if rnd.random() < 0.2:      # a deletion from the column before
                alts = rnd.sample(["T", "TG", "TGAA", "TGC"], rnd.randint(1, 3))
                if all(len(a) >= 3 for a in alts):
                    alts.append("T")
                dels = [a + 1 for a in range(len(alts)) if len(alts[a]) < 3]
                samples[row].append(Call(pos - 1, "TGA", alts, nr=nr, ploidy=ploidy, pl=pl, hom_pl={dels[-1]: 3}))
            else:
                ref = refs[rnd.randint(0, 3)]
                alts = [a for a in rnd.sample(pool, rnd.randint(1, 4)) if a != ref]
                samples[row].append(Call(pos, ref, alts, nr=nr, ploidy=ploidy, pl=pl))
    cells, q = _import(tmp_path, samples, seed, reference=False)
    q["produce_GT_with_min_PL_value_for_spanning_deletions"] = seed % 2 == 0
    return cells, q, {"intervals": [interval_facts(samples, HOT + 20 * i, HOT + 20 * i) for i in range(ncols)]}


FUZZ_SEEDS = list(range(30))


# ---- the reducer inputs ----------------------------------------------------------------------------------------------------------------------
def _tied_zero_column(rnd, n):
    """n float values whose middle lies in a run of zeros of both signs (n / 3 negative, n / 3 positive ones around them)"""
    k = n // 3
    vals = [-(1.5 + i) for i in range(k)] + [(0.25 + i) for i in range(k)] + [(-0.0, 0.0)[i % 2] for i in range(n - 2 * k)]
    rnd.shuffle(vals)
    return vals


REDUCER_COLUMN_NAMES = ["order30", "even", "all_equal", "one_valid", "all_missing", "zeros25", "zeros26", "zeros27", "zeros64"]


def reducers_small(tmp_path):
    """nine columns over 64 samples, every field of REDUCER_FIELDS on each: see REDUCER_COLUMN_NAMES"""
    rnd = random.Random(43)
    ints = lambda n: [rnd.randint(-900, 300) for _ in range(n)]                      # noqa: E731
    floats = lambda n: [rnd.randint(-4000, 2000) / 8.0 for _ in range(n)]            # noqa: E731
    def col(n, **over):
        c = {"ISUM": ints(n), "IMEAN": ints(n), "IMED": ints(n), "FSUM": floats(n), "FMEAN": floats(n), "FMED": floats(n)}
        c.update(over)
        return c
    odd = ints(30)
    odd[4] = None                                                                     # 29 valid values
    fodd = floats(30)
    fodd[11] = None
    lone = [None] * 30
    lone_i, lone_f = list(lone), list(lone)
    lone_i[17], lone_f[17] = -41, -2.75
    columns = [col(30, FSUM=order_dependent_floats(30), FMEAN=order_dependent_floats(30), IMEAN=[-50] + [0] * 29, IMED=odd, FMED=fodd),
               col(30),
               col(30, IMED=[-3] * 30, FMED=[-2.5] * 30, ISUM=[7] * 30, FSUM=[0.1] * 30),
               {f: list(lone_i if REDUCER_FIELDS[f][0] == "int" else lone_f) for f in REDUCER_FIELDS},
               {f: list(lone) for f in REDUCER_FIELDS}]
    for n in (25, 26, 27, 64):
        columns.append(col(n, FMED=_tied_zero_column(rnd, n)))
    return reducer_columns(tmp_path, columns)


def reducers_large(tmp_path, n):
    """one column of n calls (2 048 values are one LDS staging chunk of the float sum)"""
    rnd = random.Random(n)
    col = {"ISUM": [rnd.randint(-900, 300) for _ in range(n)], "IMEAN": [rnd.randint(-9, 3) for _ in range(n)],
           "IMED": [rnd.randint(-900, 300) if i % 7 else None for i in range(n)],
           "FSUM": order_dependent_floats(n), "FMEAN": order_dependent_floats(n)[1:] + [None],
           "FMED": _tied_zero_column(rnd, n)}
    return reducer_columns(tmp_path, [col], seed=n)


# ---- reducer columns among other records: which code takes a median ------------------------------------------------------------------------
# The median of a record comes from one of four pieces of code, chosen from the counts of the INTERVAL (median_path_facts; the workgroup
# site kernel k_site_huge and the per-thread scan of reduce_scalar are the other two).  A single-column interval with 25 and more calls is
# always sorted; these inputs put the hot columns among `pad` columns of one call each, so that the average can be set at will.
MEDIAN_FIELDS = ("IMED", "FMED", "QUAL")      # three median slots: two INFO fields (spanning deletions do not count) and QUAL (they do)


def f32(x):
    """x rounded to a float: what a cell stores"""
    import numpy as np
    return float(np.float32(x))


def reducer_interval(tmp_path, columns, pad, pad_first=False, seed=47):
    """columns as reducer_columns takes them; besides the fields of REDUCER_FIELDS a column may carry "QUAL": [value or None per call] (100
    without it) and "spanning": the rows whose call is a deletion that begins one column earlier (REF TG, ALT T: it ends at the hot column).
    The hot columns (ten apart) and the pad columns (two apart, SNVs without reducer fields, QUAL 100) are queried as ONE interval that
    begins at HOT.  pad: a number of columns with one call each, in row j modulo the rows of the hot columns, or a list of calls per
    column, in rows 0 .. calls - 1.  pad_first: the pad columns come first, the last hot column is the last record"""
    counts = [len(next(v for k, v in col.items() if k != "spanning")) for col in columns]
    nrows = max(counts)
    pads = [(j % nrows,) for j in range(pad)] if isinstance(pad, int) else [tuple(range(c)) for c in pad]
    nrows = max([nrows] + [len(rows) for rows in pads])
    hot0 = HOT + 2 * len(pads) + 10 if pad_first else HOT
    pad0 = HOT if pad_first else HOT + 10 * len(columns)
    positions = [hot0 + 10 * i for i in range(len(columns))]
    samples = [[] for _ in range(nrows)]
    for pos, col, n in zip(positions, columns, counts):
        spanning = col.get("spanning", ())
        assert all(len(v) == n for k, v in col.items() if k != "spanning") and all(0 <= r < n for r in spanning)
        for row in range(n):
            info = {f: _fmt(col[f][row]) for f in REDUCER_FIELDS if f in col and col[f][row] is not None}
            qual = "100" if "QUAL" not in col else "." if col["QUAL"][row] is None else _fmt(col["QUAL"][row])
            if row in spanning:
                samples[row].append(Call(pos - 1, "TG", ["T"], pl=False, info=info, qual=qual))
            else:
                samples[row].append(Call(pos, "G", ["T"], pl=False, info=info, qual=qual))
    for j, rows in enumerate(pads):
        for row in rows:
            samples[row].append(Call(pad0 + 2 * j, "A", ["C"], pl=False))
    cells, q = _import(tmp_path, samples, seed, reducers=True, attributes=["REF", "ALT", "GT", "DP"], reference=False, qual_median=True)
    last = max(positions[-1], pad0 + 2 * (len(pads) - 1))
    return cells, q, {"intervals": [interval_facts(samples, HOT, last)], "columns": columns, "positions": positions}


def valid_values(col, field):
    """the values of one column that count for a field's reducer: not missing, and for an INFO field not on a spanning deletion"""
    if field not in col:
        return [100.0] * len(col["IMED"]) if field == "QUAL" else []
    skip = () if field == "QUAL" else col.get("spanning", ())
    return [v for row, v in enumerate(col[field]) if v is not None and row not in skip]


def median_by_hand(values):
    """the reference's median: std::nth_element at size / 2"""
    return sorted(values)[len(values) // 2] if values else None


def _mcol(rnd, n, **over):
    """a column of n calls with ordinary values on every reducer field and on QUAL"""
    ints = lambda: [rnd.randint(-900, 300) for _ in range(n)]                        # noqa: E731
    floats = lambda: [rnd.randint(-4000, 2000) / 8.0 for _ in range(n)]              # noqa: E731
    c = {"ISUM": ints(), "IMEAN": ints(), "IMED": ints(), "FSUM": floats(), "FMEAN": floats(), "FMED": floats(),
         "QUAL": [rnd.randint(1, 8000) / 8.0 for _ in range(n)]}
    c.update(over)
    return c


def _shuffled(rnd, values):
    values = list(values)
    rnd.shuffle(values)
    return values


def _among_missing(rnd, n, values):
    """values on random rows of n calls, the other rows missing"""
    out = [None] * n
    for row, v in zip(rnd.sample(range(n), len(values)), values):
        out[row] = v
    return out


def median_48_49(tmp_path):
    """48 calls are no big record, 49 are; five pad columns: T = 102 <= 16 x 7"""
    rnd = random.Random(51)
    return reducer_interval(tmp_path, [_mcol(rnd, 48), _mcol(rnd, 49)], 5)


def median_average_16(tmp_path, one_more):
    """P = 4 records with 49 + 13 + 1 + 1 = 64 = 16 P calls: the 49 are a big record; one call more on a pad column and the medians are sorted"""
    rnd = random.Random(52)
    return reducer_interval(tmp_path, [_mcol(rnd, 49), _mcol(rnd, 13)], [1, 2 if one_more else 1])


def median_sorted_single(tmp_path):
    """P = 1 record with 20 calls: sorted (the key holds no record bits) and no record for k_site_huge"""
    rnd = random.Random(54)
    return reducer_interval(tmp_path, [_mcol(rnd, 20, IMED=_among_missing(rnd, 20, [rnd.randint(-900, 300) for _ in range(18)]))], 0)


def median_sorted_last_of_4(tmp_path):
    """P = 4, a power of two, and the 70 calls are the LAST record (k = 3: both record bits of the sort key set); T = 73 > 64, T / P < 24"""
    rnd = random.Random(55)
    return reducer_interval(tmp_path, [_mcol(rnd, 70, FMED=_among_missing(rnd, 70, [rnd.randint(-4000, 2000) / 8.0 for _ in range(64)]))], 3, pad_first=True)


MEDIAN_VALUE_COLUMN_NAMES = ["odd49", "even50", "even50_among_53", "all_equal", "one_valid", "none_valid", "extremes", "zeros49", "zeros50", "zeros51",
                             "both_zero_signs_beside_the_median", "zero_median_plus_only", "zero_median_minus_only"]


def median_values(tmp_path):
    """thirteen big records of 49 - 55 calls among 30 pad columns (T = 683 <= 16 x 43): see MEDIAN_VALUE_COLUMN_NAMES.  extremes: ints from
    -2147483646, the smallest valid one (INT32_MIN is "missing", INT32_MIN + 1 "vector end"), to 2147483647; floats around -3e38 and
    denormals of both signs, the median a denormal"""
    rnd = random.Random(53)
    ints = lambda n: [rnd.randint(-900, 300) for _ in range(n)]                      # noqa: E731
    floats = lambda n: [rnd.randint(-4000, 2000) / 8.0 for _ in range(n)]            # noqa: E731
    quals = lambda n: [rnd.randint(1, 8000) / 8.0 for _ in range(n)]                 # noqa: E731
    lone = lambda v: [v if row == 17 else None for row in range(55)]                 # noqa: E731
    around = lambda zero: _shuffled(rnd, [-(1.5 + i) for i in range(10)] + [0.25 + i for i in range(10)] + [zero] * 29)     # noqa: E731
    beside = lambda: _shuffled(rnd, [-0.0, 0.0] + [1.0 + i / 8.0 for i in range(47)])                                     # noqa: E731
    columns = [_mcol(rnd, 49), _mcol(rnd, 50),
               _mcol(rnd, 53, IMED=_among_missing(rnd, 53, ints(50)), FMED=_among_missing(rnd, 53, floats(50)), QUAL=_among_missing(rnd, 53, quals(50))),
               _mcol(rnd, 49, IMED=[-3] * 49, FMED=[-2.5] * 49, QUAL=[7.25] * 49),
               _mcol(rnd, 55, IMED=lone(-41), FMED=lone(-2.75), QUAL=lone(3.5)),
               _mcol(rnd, 49, IMED=[None] * 49, FMED=[None] * 49, QUAL=[None] * 49),
               _mcol(rnd, 51, IMED=_shuffled(rnd, [-2147483646 + i for i in range(26)] + [2147483647 - i for i in range(25)]),
                     FMED=_shuffled(rnd, [f32(-3.0e38 + i * 1e37) for i in range(20)] + [f32(-(i + 1) * 1e-41) for i in range(10)] + [f32((i + 1) * 1e-42) for i in range(21)]),
                     QUAL=_shuffled(rnd, [f32((i + 1) * 1e-41) for i in range(30)] + [f32(3.0e38 - i * 1e37) for i in range(21)]))]
    for n in (49, 50, 51):
        columns.append(_mcol(rnd, n, FMED=_tied_zero_column(rnd, n), QUAL=_tied_zero_column(rnd, n)))
    columns += [_mcol(rnd, 49, FMED=beside(), QUAL=beside()), _mcol(rnd, 49, FMED=around(0.0), QUAL=around(0.0)), _mcol(rnd, 49, FMED=around(-0.0), QUAL=around(-0.0))]
    return reducer_interval(tmp_path, columns, 30)


def median_spanning(tmp_path):
    """two big records of which rows 0 - 11 are deletions that begin one column earlier.  Their INFO and QUAL values lie below all others:
    counting them would move an INFO median down (they must not count), leaving them out would move the QUAL median up (they must
    count).  The first record keeps 48 valid INFO values of 60 calls - it is listed all the same, a record is big by its calls - the second
    50 of 62; the deletions of the second begin inside the interval and are a record of 12 calls themselves"""
    rnd = random.Random(59)
    columns = []
    for n in (60, 62):
        k = n - 12
        columns.append(_mcol(rnd, n, spanning=set(range(12)),
                             IMED=[-1000 - r for r in range(12)] + _shuffled(rnd, range(1, k + 1)),
                             FMED=[-500.5 - r for r in range(12)] + _shuffled(rnd, [i + 0.5 for i in range(1, k + 1)]),
                             QUAL=[1.5 + r for r in range(12)] + _shuffled(rnd, [100.0 + i for i in range(1, k + 1)])))
    return reducer_interval(tmp_path, columns, 6)


GRID_STRIDE_VALID = (49, 2, 1, 0)


def median_grid_stride(tmp_path):
    """70 big records for the 64 workgroups of k_big_medians: six workgroups take a second record.  Consecutive records have 49, 2, 1 and 0
    valid values (what a workgroup left in LDS for the record before must not count) and no two records one median"""
    rnd = random.Random(61)
    columns = []
    for i in range(70):
        v = GRID_STRIDE_VALID[i % 4]
        columns.append(_mcol(rnd, 49, IMED=_among_missing(rnd, 49, [100 * i + k for k in range(v)]),
                             FMED=_among_missing(rnd, 49, [100 * i + k + 0.5 for k in range(v)]),
                             QUAL=_among_missing(rnd, 49, [10000 + 100 * i + k + 0.25 for k in range(v)])))
    return reducer_interval(tmp_path, columns, 155)


def median_big_and_huge(tmp_path, tied):
    """300 calls among 19 pad columns (T = 319 <= 16 x 20, so only more than 256 calls make a record of k_site_huge): big and huge at once,
    the big table is asked first.  tied: zeros of both signs at the middle - the big table says 2, the workgroup site kernel says 2, and
    the site thread runs the reference's selection"""
    rnd = random.Random(67)
    over = dict(FMED=_tied_zero_column(rnd, 300), QUAL=_tied_zero_column(rnd, 300)) if tied else {}
    return reducer_interval(tmp_path, [_mcol(rnd, 300, **over)], 19)


def median_capacity(tmp_path):
    """4096 calls fill the LDS of k_big_medians, 4097 are too many: that record's medians come from k_site_huge, and without it from the
    per-thread scan.  545 pad columns: T = 8738 <= 16 x 547"""
    rnd = random.Random(71)
    columns = [_mcol(rnd, n, IMED=[rnd.randint(-900, 300) if i % 7 else None for i in range(n)], FMED=_tied_zero_column(rnd, n)) for n in (4096, 4097)]
    return reducer_interval(tmp_path, columns, [1] * 545)


def median_list_overflow(tmp_path):
    """4100 big records of 49 calls and 9020 pad columns (T = 209920 = 16 P): the list of k_big_records holds 4096, four records find it
    full - which four depends on the order of the atomics, so no two records have one median"""
    rnd = random.Random(73)
    columns = [{"IMED": _shuffled(rnd, [64 * i + k for k in range(49)]), "FMED": _shuffled(rnd, [64 * i + k + 0.5 for k in range(49)]),
                "QUAL": _shuffled(rnd, [10.25 + 64 * i + k for k in range(49)]), "ISUM": [i % 1000] * 49, "FMEAN": [0.5 * (i % 100)] * 49}
               for i in range(4100)]
    return reducer_interval(tmp_path, columns, 9020)


def _paths(calls, num_records, is_sorted, big, unlisted=0, huge_records=0):
    return [dict(calls=calls, num_records=num_records, sorted=is_sorted, big_listed=big, big_unlisted=unlisted, huge_records=huge_records, huge_fallbacks=0)]


# name -> (builder, the prediction of the interval): calls T, records P, sorted (T > 16 P), big records listed / unlisted, records of k_site_huge
MEDIAN_CASES = {
    "median_48_49": (median_48_49, _paths(48 + 49 + 5, 7, False, 1)),
    "median_average_16": (lambda t: median_average_16(t, False), _paths(64, 4, False, 1)),
    "median_average_16_and_one_call": (lambda t: median_average_16(t, True), _paths(65, 4, True, 0)),
    "median_sorted_single_record": (median_sorted_single, _paths(20, 1, True, 0)),
    "median_sorted_last_of_4_records": (median_sorted_last_of_4, _paths(73, 4, True, 0)),
    "median_values": (median_values, _paths(653 + 30, 43, False, 13)),
    "median_spanning": (median_spanning, _paths(60 + 12 + 62 + 6, 9, False, 2)),
    "median_grid_stride": (median_grid_stride, _paths(70 * 49 + 155, 225, False, 70)),
    "median_big_and_huge": (lambda t: median_big_and_huge(t, False), _paths(319, 20, False, 1, huge_records=1)),
    "median_big_and_huge_tied_zeros": (lambda t: median_big_and_huge(t, True), _paths(319, 20, False, 1, huge_records=1)),
    "median_capacity": (median_capacity, _paths(4096 + 4097 + 545, 547, False, 1, huge_records=2)),
    "median_list_overflow": (median_list_overflow, _paths(4100 * 49 + 9020, 13120, False, 4096, unlisted=4)),
}
MEDIAN_MODES = ("default", "no_huge", "sorted")       # nothing set, GDBAMD_NO_HUGE_SITES=1, GDBAMD_SORTED_MEDIAN=1


def median_counters(iv, mode):
    """(sorted_median_fields, big_median_records, big_median_unlisted, huge_records, huge_fallbacks) an interval of MEDIAN_CASES must report"""
    is_sorted = iv["sorted"] or mode == "sorted"
    huge = (0, 0) if mode == "no_huge" else (iv["huge_records"], iv["huge_fallbacks"])
    return ((len(MEDIAN_FIELDS), 0, 0) if is_sorted else (0, iv["big_listed"], iv["big_unlisted"])) + huge


# ---- the cases both test files run: name -> (builder, what the case predicts for its intervals, in order) ---------------------------------
def _one(calls, huge_records, huge_fallbacks, **more):
    return [dict(calls=calls, huge_records=huge_records, huge_fallbacks=huge_fallbacks, **more)]


CASES = {
    "selection_24_calls": (lambda t: selection_single(t, 24), _one(24, 0, 0)),
    "selection_25_calls": (lambda t: selection_single(t, 25), _one(25, 1, 0)),
    "selection_257_and_256_calls_among_30_records": (selection_absolute_threshold, _one(257 + 256 + 28 * 3, 1, 0, num_records=30)),
    "first_appearance": (first_appearance, _one(40, 1, 0)),
    "suffix_extension": (suffix_extension, _one(30, 1, 0, distinct=8)),
    "collision_equal_length": (collision_equal_length, _one(30, 1, 1, distinct=14)),
    "collision_unequal_length": (collision_unequal_length, _one(30, 1, 1, distinct=14)),
    "collision_after_extension": (collision_after_extension, _one(30, 1, 1, distinct=14)),
    "collision_in_one_of_two_records": (collision_in_one_of_two_records, _one(60, 2, 1, num_records=2)),
    "marker_hash_alone": (marker_hash_alone, _one(30, 1, 0, distinct=13)),
    "marker_hash_with_remap_target": (marker_hash_with_remap_target, _one(30, 1, 1, distinct=14)),
    "cap_126_alts": (lambda t: distinct_alts(t, 130, MAX_MERGED_ALT), _one(130, 1, 0, distinct=126)),
    "spanning_deletions_min_pl_gt": (lambda t: spanning_deletions(t, True), _one(48, 1, 0)),
    "spanning_deletions_plain_gt": (lambda t: spanning_deletions(t, False), _one(48, 1, 0)),
    "reducers_small": (reducers_small, [dict(calls=n, huge_records=1, huge_fallbacks=0) for n in (30, 30, 30, 30, 30, 25, 26, 27, 64)]),
    "reducers_2048": (lambda t: reducers_large(t, 2048), _one(2048, 1, 0)),
    "reducers_2049": (lambda t: reducers_large(t, 2049), _one(2049, 1, 0)),
    "reducers_2050": (lambda t: reducers_large(t, 2050), _one(2050, 1, 0)),
}
MERGE_CASES = ["first_appearance", "suffix_extension", "collision_equal_length", "collision_unequal_length", "collision_after_extension",
               "collision_in_one_of_two_records", "marker_hash_alone", "marker_hash_with_remap_target", "cap_126_alts"]
# inputs the serial walk and the workgroup kernel must both refuse: (builder, calls)
TOO_MANY = {"cap_127_alts": (lambda t: distinct_alts(t, 130, MAX_MERGED_ALT + 1), 130),
            "table_overflow_520_alts": (lambda t: distinct_alts(t, 520, 520), 520)}


def check_case(name, facts):
    """the case's stated predictions against the facts derived from its input lines; returns the intervals"""
    check_facts(facts)
    predicted = (CASES.get(name) or MEDIAN_CASES[name])[1]
    assert len(predicted) == len(facts["intervals"]), name
    for want, iv in zip(predicted, facts["intervals"]):
        if "sorted" in want:
            assert (iv["sorted"], iv["big_listed"], iv["big_unlisted"]) == (want["sorted"], want["big_listed"], want["big_unlisted"]), (name, iv["sorted"], iv["big_records"])
        assert iv["heavy"] == want["calls"], (name, iv["heavy"])
        assert iv["num_records"] == want.get("num_records", 1), (name, iv["num_records"])
        assert iv["huge_records"] == want["huge_records"] and iv["huge_fallbacks"] == want["huge_fallbacks"], (name, iv)
        if "distinct" in want:
            assert list(iv["distinct"].values())[0] == want["distinct"], (name, iv["distinct"])
    return facts["intervals"]


def record_lines(text):
    return [l.split("\t") for l in text.decode().splitlines() if l and not l.startswith("#")]


def check_merged_lists(text, iv):
    """REF and ALT of every record of the oracle's text against the lists derived from the input lines"""
    recs = record_lines(text)
    assert len(recs) == iv["num_records"]
    for f in recs:
        col = int(f[1]) - 1
        assert f[3] == iv["merged_ref"][col], (col, f[3])
        assert f[4].split(",") == iv["merged_alt"][col], (col, f[4])
