"""The plain-Python model of vcfdiff (tests/tools/vcfdiff_model.py) against known answers worked by hand from the reference's lines
(tools/src/vcfdiff.cc, tools/include/vcfdiff.h) and from the rule in DESIGN.md, "Comparing two VCFs".  Each case names its lines.
Host code only - nothing of the product runs here."""
from types import SimpleNamespace as NS

import helpers  # noqa: F401
import vcfdiff_inputs as vi  # noqa: F401  (puts tests/tools on the path)
import vcfdiff_model as vm

HEAD = """##fileformat=VCFv4.2
##INFO=<ID=END,Number=1,Type=Integer,Description="e">
##INFO=<ID=DP,Number=1,Type=Integer,Description="d">
##INFO=<ID=XS,Number=1,Type=String,Description="s">
##INFO=<ID=DB,Number=0,Type=Flag,Description="f">
##INFO=<ID=MQ,Number=1,Type=Float,Description="m">
##FORMAT=<ID=GT,Number=1,Type=String,Description="g">
##FORMAT=<ID=PL,Number=G,Type=Integer,Description="p">
##FORMAT=<ID=PGT,Number=1,Type=String,Description="p">
##contig=<ID=1,length=1000>
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB
"""


def diff(tmp_path, gold_lines, test_lines, **kw):
    gp, tp = str(tmp_path / "g.vcf"), str(tmp_path / "t.vcf")
    for p, lines in ((gp, gold_lines), (tp, test_lines)):
        with open(p, "w") as f:
            f.write(HEAD + "".join(x + "\n" for x in lines))
    return vm.model(gp, tp, **kw)


def line(pos=5, ref="G", alt="A,T", qual=".", flt=".", info=".", fmt="GT:PL", a="./.:1,2,3,4,5,6", b=".:.", ident="."):
    return "\t".join(["1", str(pos), ident, ref, alt, qual, flt, info, fmt, a, b])


def test_genotype_maps_for_a_swapped_alt_pair():
    """vcfdiff.h:57-72: diploid genotype (i <= j) sits at j(j+1)/2 + i.  With REF,A,T against REF,T,A the map is [0, 2, 1]; the genotypes
    00 01 11 02 12 22 go to 00 02 22 01 12 11, that is to the indices 0 3 5 1 4 2"""
    amap = [0, 2, 1]
    assert [vm.map_index("G", k, amap, 2) for k in range(6)] == [0, 3, 5, 1, 4, 2]
    # triploid, the same alleles: 000 001 011 111 002 012 112 022 122 222 go to 000 002 022 222 001 012 122 011 112 111
    assert [vm.map_index("G", k, amap, 3) for k in range(10)] == [0, 4, 7, 9, 1, 5, 8, 2, 6, 3]
    assert [vm.map_index("G", k, amap, 1) for k in range(3)] == [0, 2, 1]
    # vcfdiff.h:100: an index beyond the genotypes, and ploidy 0, map to themselves
    assert vm.map_index("G", 6, amap, 2) == 6 and vm.map_index("G", 4, amap, 0) == 4
    # :438-443: A is map[k + 1] - 1, R is map[k]
    assert [vm.map_index("A", k, amap, 2) for k in range(2)] == [1, 0] and [vm.map_index("R", k, amap, 2) for k in range(3)] == [0, 2, 1]
    # the order of the genotypes, written out for 4 alleles: the diploid index of (2, 3) is 3 * 4 / 2 + 2 = 8
    assert vm.genotype_index([3, 2]) == 8 and vm.genotype_of(8, 2, 4) == [2, 3]


def test_pl_through_the_map(tmp_path):
    gold = [line(a="./.:10,11,12,13,14,15")]
    assert diff(tmp_path, gold, [line(alt="T,A", a="./.:10,13,15,11,14,12")])["events"] == []
    ev = diff(tmp_path, gold, [line(alt="T,A", a="./.:10,11,12,13,14,15")])["events"]
    assert len(ev) == 1 and ev[0]["format"]["DIFFERS"] == ["PL"] and ev[0]["flags"] == []
    # :406-408: the alleles differ, so a G field differs outright; :688-711
    ev = diff(tmp_path, gold, [line(alt="T,C", a="./.:10,11,12,13,14,15")])["events"]
    assert ev[0]["flags"] == ["ALLELES"] and ev[0]["format"]["DIFFERS"] == ["PL"]


def test_float_quirks():
    """:366-376: diff > t and rel > t, rel = |diff / a| with a first, 0 when a is 0; NaN compares false"""
    t = 1e-5
    assert vm.float_differs("1", "1.1", t)
    assert not vm.float_differs("1.0", "1.000001", t)            # diff 1e-6
    assert not vm.float_differs("100000", "100000.5", t)         # diff 0.5, rel 5e-6
    assert not vm.float_differs("0", "5", t) and vm.float_differs("5", "0", t)      # a == 0: rel is 0
    assert not vm.float_differs(".", "3", t) and not vm.float_differs("3", ".", t) and not vm.float_differs(".", ".", t)
    assert not vm.float_differs("1.5e30", "1.50e30", t) and vm.float_differs("1.5e30", "2.5e30", t)


def test_qual_takes_test_first(tmp_path):
    """:714: compare_unequal(test QUAL, gold QUAL)"""
    assert diff(tmp_path, [line(qual="0")], [line(qual="5")])["events"][0]["flags"] == ["QUAL"]      # a = 5
    assert diff(tmp_path, [line(qual="5")], [line(qual="0")])["events"] == []                          # a = 0
    assert diff(tmp_path, [line(qual="5")], [line(qual=".")])["events"] == []


def test_empty_field_rule(tmp_path):
    """:501-509, :583-591, bcf_is_empty_field: a field one line lacks counts only when some value of it is not missing; :521-523 Flags"""
    g = line(info="DP=5;XS=.;DB;MQ=3")
    assert diff(tmp_path, [g], [line(info="DP=5;MQ=3")])["events"] == []
    ev = diff(tmp_path, [g], [line(info="XS=.;DB;MQ=3")])["events"]
    assert ev[0]["info"] == {"MISSING_IN_TEST": ["DP"], "ADDED_IN_TEST": [], "TYPE_DIFFERS": [], "DIFFERS": []}
    ev = diff(tmp_path, [line(info="MQ=3")], [line(info="DP=7;MQ=3")])["events"]
    assert ev[0]["info"]["ADDED_IN_TEST"] == ["DP"]
    assert diff(tmp_path, [line(fmt="GT:PL:PGT", a="./.:1,2,3,4,5,6:.", b=".:.")], [line()])["events"] == []
    ev = diff(tmp_path, [line(fmt="GT:PL:PGT", a="./.:1,2,3,4,5,6:.", b=".:.:0|1")], [line()])["events"]
    assert ev[0]["format"]["MISSING_IN_TEST"] == ["PGT"]
    # :357-362: '.' is './.'; separators are compared where both have them
    assert diff(tmp_path, [line(b="./.:.")], [line(b=".:.")])["events"] == []
    assert diff(tmp_path, [line(b="0/0:.")], [line(b="0|0:.")])["events"][0]["format"]["DIFFERS"] == ["GT"]
    # ID: sets of tokens split at ';' and ',' (:596-610); FILTER: the counts, then test's among gold's (:718-735)
    assert diff(tmp_path, [line(ident="rs1;rs2")], [line(ident="rs2,rs1")])["events"] == []
    assert diff(tmp_path, [line(ident="rs1;rs2")], [line(ident="rs1")])["events"][0]["flags"] == ["ID"]
    assert diff(tmp_path, [line(flt="PASS")], [line(flt=".")])["events"][0]["flags"] == ["FILTER"]


def rec(contig, pos, end, refblock=False, long_ref=False):
    return NS(contig=contig, pos=pos, end=end, refblock=refblock, long_ref=long_ref)


def kinds(events):
    return [(k, (g.pos, g.end) if g else None, (t.pos, t.end) if t else None) for k, g, t in events]


def test_walk_branches():
    C = ["1"]
    # 1. equal keys
    assert kinds(vm.walk([rec("1", 5, 5)], [rec("1", 5, 5)], C, C)) == [("COMPARED", (5, 5), (5, 5))]
    # 2. reference blocks that overlap (:1150-1160); the smaller end advances, both when equal (:1222-1236)
    g, t = [rec("1", 10, 20, True)], [rec("1", 10, 15, True), rec("1", 16, 20, True)]
    assert kinds(vm.walk(g, t, C, C)) == [("REF_BLOCKS_OVERLAP", (10, 20), (10, 15)), ("REF_BLOCKS_OVERLAP", (10, 20), (16, 20))]
    # 3. no overlap: the file with the smaller pos seeks to its first record whose end reaches the other's pos (:1165-1168)
    g, t = [rec("1", 5, 5), rec("1", 7, 8), rec("1", 10, 10)], [rec("1", 10, 10)]
    assert kinds(vm.walk(g, t, C, C)) == [("DIFFERENT_POSITIONS", (5, 5), (10, 10)), ("COMPARED", (10, 10), (10, 10))]
    g, t = [rec("1", 10, 10)], [rec("1", 2, 3), rec("1", 10, 10)]
    assert kinds(vm.walk(g, t, C, C)) == [("DIFFERENT_POSITIONS", (10, 10), (2, 3)), ("COMPARED", (10, 10), (10, 10))]
    # overlap, test ends later: test advances only with a long REF that begins at or before gold (:1177-1210), else gold does
    g, t = [rec("1", 10, 10), rec("1", 12, 12)], [rec("1", 10, 12, long_ref=True), rec("1", 12, 12)]
    assert kinds(vm.walk(g, t, C, C)) == [("DIFFERENT_POSITIONS", (10, 10), (10, 12)), ("DIFFERENT_POSITIONS", (10, 10), (12, 12)), ("COMPARED", (12, 12), (12, 12))]
    g, t = [rec("1", 10, 10), rec("1", 11, 14)], [rec("1", 10, 14)]
    assert kinds(vm.walk(g, t, C, C)) == [("DIFFERENT_POSITIONS", (10, 10), (10, 14)), ("DIFFERENT_POSITIONS", (11, 14), (10, 14))]
    # the mirror image: gold ends later and has the long REF
    g, t = [rec("1", 10, 12, long_ref=True), rec("1", 13, 13)], [rec("1", 11, 11), rec("1", 13, 13)]
    assert kinds(vm.walk(g, t, C, C)) == [("DIFFERENT_POSITIONS", (10, 12), (11, 11)), ("DIFFERENT_POSITIONS", (13, 13), (11, 11)), ("COMPARED", (13, 13), (13, 13))]
    # 4. one file runs out: one EXTRA_LINES with its current record
    g, t = [rec("1", 5, 5), rec("1", 6, 6), rec("1", 7, 7)], [rec("1", 5, 5)]
    assert kinds(vm.walk(g, t, C, C)) == [("COMPARED", (5, 5), (5, 5)), ("EXTRA_LINES", (6, 6), None)]


def test_order_of_work():
    """:801: the common contigs in ascending byte order of their names, then gold's own, then test's own"""
    gc, tc = ["2", "10", "G", "1"], ["1", "T", "2", "10"]
    g = [rec("2", 1, 1), rec("10", 2, 2), rec("G", 3, 3), rec("1", 4, 4)]
    t = [rec("1", 4, 4), rec("T", 5, 5), rec("T", 6, 6), rec("2", 1, 1), rec("10", 2, 2)]
    assert kinds(vm.walk(g, t, gc, tc)) == [("COMPARED", (4, 4), (4, 4)), ("COMPARED", (2, 2), (2, 2)), ("COMPARED", (1, 1), (1, 1)), ("EXTRA_LINES", (3, 3), None),
                                             ("EXTRA_LINES", None, (5, 5))]


def test_regions_syntax():
    """:807-848: chr, chr:pos, chr:from-to, chr:from-; the first entry per contig counts; 1-based on the command line"""
    big = 2**62
    assert vm.parse_regions("1,2:5,3:7-9,4:11-,1:3") == {"1": (0, big), "2": (4, 4), "3": (6, 8), "4": (10, big)}
    assert vm.parse_regions("HLA:A") == {"HLA:A": (0, big)} and vm.parse_regions("") == {}


def test_keys_of_a_record(tmp_path):
    """pos = POS - 1; end = END - 1 with INFO END (the last one counts), else pos + len(REF) - 1; refblock, long_ref"""
    p = str(tmp_path / "k.vcf")
    lines = [line(pos=5, ref="GAC"), line(pos=9, alt="<NON_REF>", info="END=3;DP=1;END=20", a="./.:1,2,3"), line(pos=30, alt="<NON_REF>,A")]
    with open(p, "w") as f:
        f.write(HEAD + "".join(x + "\n" for x in lines))
    text = vm.read_text(p)
    r = vm.parse_records(p, text, vm.Header(text))
    assert [(x.pos, x.end, x.refblock, x.long_ref, x.line_no) for x in r] == [(4, 6, False, True, 12), (8, 19, True, False, 13), (29, 29, False, False, 14)]
