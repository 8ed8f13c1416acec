"""vcfdiff on the device (csrc/kernels/gdb_vcfdiff.hip; vcfdiff(...), the vcfdiff tool) against the plain-Python model
tests/tools/vcfdiff_model.py: the reports are equal, exactly.  Every case also asserts from the statistics that the kernels ran: the pairs
compared are the model's, every pair took one of the two per-sample paths, and the wavefront-per-sample path ran exactly on the allele-rich
shapes whose ALTs are permuted.  Inputs: the generator of tests/vcfdiff_inputs.py as plain text, gzip and BGZF, once with a text budget
of 4096 bytes so that pairs straddle batches; every VCF text golden against itself; t0_1_2_vcf_at_0 against a copy with A,T swapped."""
import glob
import os
import subprocess

import pytest

import helpers  # noqa: F401
import vcfdiff_inputs as vi
import vcfdiff_model as vm

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outputs")


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


def vcf_goldens():
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "*"))):
        with open(p, "rb") as f:
            if f.read(16).startswith(b"##fileformat=VCF"):
                out.append(os.path.basename(p))
    return out


def check_stats(st, want, heavy):
    assert st["pairs_compared"] == want["compared"] and st["pairs_light"] + st["pairs_heavy"] == want["compared"]
    assert st["events"] == len(want["events"]) and st["num_batches"] >= 2
    assert (st["pairs_heavy"] > 0) == heavy, st


@pytest.mark.parametrize("ns,na,lines,transform", vi.pair_cases())
def test_generated_pair(gdb, tmp_path, ns, na, lines, transform):
    g, t, expected = vi.make_pair(vi.seed_of(ns, na, transform), ns, na, transform, lines, exponent_floats=True)
    want = None
    for how in ("plain", "gzip", "bgzf"):
        gp, tp = vi.write_as(str(tmp_path / ("g." + how)), g, how), vi.write_as(str(tmp_path / ("t." + how)), t, how)
        if want is None:
            want = vm.model(gp, tp)
            assert vi.summarize(want) == expected
        st = {}
        got = gdb.vcfdiff(gp, tp, stats=st)
        assert got == want, how
        check_stats(st, want, heavy=na > 3 and transform in vi.PERMUTING)


def test_pairs_straddle_batches(gdb, tmp_path):
    g, t, _ = vi.make_pair(5, 65, 7, "permuted_change_pl", 24)
    gp, tp = vi.write_as(str(tmp_path / "g.vcf.gz"), g, "bgzf"), vi.write_as(str(tmp_path / "t.vcf"), t, "plain")
    want = vm.model(gp, tp)
    st = {}
    assert gdb.vcfdiff(gp, tp, text_budget_bytes=4096, stats=st) == want
    assert st["num_batches"] >= 16 and st["pairs_heavy"] > 0 and len(want["events"]) == 1


def test_deferred_floats(gdb, tmp_path):
    """1.5e30 against 1.50e30: outside the device parser's exact range, decided by the host - equal; against 2.5e30: different"""
    g, t, _ = vi.make_pair(11, 3, 3, "float_noise", 60, exponent_floats=True)
    assert "e30" in g and "0e30" in t
    gp, tp = vi.write_as(str(tmp_path / "g.vcf"), g, "plain"), vi.write_as(str(tmp_path / "t.vcf"), t, "plain")
    st = {}
    assert gdb.vcfdiff(gp, tp, stats=st) == vm.model(gp, tp) and st["deferred"] > 0 and st["events"] == 0
    tp2 = vi.write_as(str(tmp_path / "t2.vcf"), g.replace("1.5e30", "2.5e30"), "plain")
    want = vm.model(gp, tp2)
    assert want["events"] and all(e["info"]["DIFFERS"] == ["BaseQRankSum"] for e in want["events"])
    assert gdb.vcfdiff(gp, tp2, stats=st) == want and st["deferred"] == len(want["events"])


@pytest.mark.parametrize("name", vcf_goldens())
def test_golden_against_itself(gdb, name):
    p = os.path.join(GOLDEN, name)
    st = {}
    got = gdb.vcfdiff(p, p, stats=st)
    with open(p) as f:
        n = sum(1 for line in f if line.strip() and not line.startswith("#"))
    assert got == {"compared": n, "events": []} and st["pairs_compared"] == n and st["pairs_heavy"] == 0


def test_t0_1_2_with_alts_swapped(gdb, tmp_path):
    p = os.path.join(GOLDEN, "t0_1_2_vcf_at_0")
    with open(p) as f:
        text = f.read()
    swapped = vi.swap_first_two_alts(text)
    assert swapped != text and "\tT,A,<NON_REF>\t" in swapped
    tp = str(tmp_path / "swapped.vcf")
    with open(tp, "w") as f:
        f.write(swapped)
    want = vm.model(p, tp)
    assert want["events"] == []
    st = {}
    assert gdb.vcfdiff(p, tp, stats=st) == want and st["pairs_heavy"] > 0
    # without the remap of the fields the same swap is found
    broken = text.replace("\tA,T,<NON_REF>\t", "\tT,A,<NON_REF>\t")
    with open(tp, "w") as f:
        f.write(broken)
    want = vm.model(p, tp)
    assert want["events"] and all("PL" in e["format"]["DIFFERS"] for e in want["events"])
    assert gdb.vcfdiff(p, tp) == want


def test_regions(gdb, tmp_path):
    g, t, _ = vi.make_pair(21, 3, 3, "delete_line", 60)
    gp, tp = vi.write_as(str(tmp_path / "g.vcf"), g, "plain"), vi.write_as(str(tmp_path / "t.vcf"), t, "plain")
    for regions in ("2", "1:100-150,2:120", "10:130-", "1,1:5"):
        want = vm.model(gp, tp, regions=regions)
        assert gdb.vcfdiff(gp, tp, regions=regions) == want, regions
    assert vm.model(gp, tp, regions="2")["events"] == [] and vm.model(gp, tp, regions="1")["events"]


def run_tool(gdb, *args):
    from genomicsdb_amd import build as b
    r = subprocess.run([b.TOOLS["vcfdiff"]] + [str(a) for a in args], capture_output=True, timeout=120)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_tool_messages(gdb, tmp_path):
    g, t, _ = vi.make_pair(31, 3, 3, "remove_info", 60)
    gp, tp = vi.write_as(str(tmp_path / "g.vcf"), g, "plain"), vi.write_as(str(tmp_path / "t.vcf"), t, "plain")
    ev = vm.model(gp, tp)["events"][0]
    bar = "=" * 69 + "\n"
    rc, out, err = run_tool(gdb, gp, tp)
    assert rc == 0 and out == ""
    body, timer = err.rsplit("GENOMICSDB_TIMER,vcfdiff,", 1)
    assert body == bar + ev["gold_text"] + "\n" + ev["test_text"] + "\n" + "ERROR: INFO field DP missing in test line\n" + bar
    assert ",compared,60," in timer and ",heavy,0," in timer
    g, t, _ = vi.make_pair(32, 3, 3, "cut_ref_block", 60)
    gp, tp = vi.write_as(str(tmp_path / "g2.vcf"), g, "plain"), vi.write_as(str(tmp_path / "t2.vcf"), t, "bgzf")
    evs = vm.model(gp, tp)["events"]
    rc, out, err = run_tool(gdb, "-t", "1e-4", gp, tp)
    assert rc == 0 and err.startswith("GENOMICSDB_TIMER,vcfdiff,")
    want = ""
    for e in evs:
        cols = e["gold_text"].split("\t")
        want += "WARNING: Gold and test REF blocks overlap, but do not match exactly at position %s,%s\n%s\n%s\n" % (cols[0], cols[1], e["gold_text"], e["test_text"])
    assert out == want and len(evs) == 2


def test_refusals(gdb, tmp_path):
    g, t, _ = vi.make_pair(41, 3, 3, "all_neutral", 30)
    gp = vi.write_as(str(tmp_path / "g.vcf"), g, "plain")
    renamed = vi.write_as(str(tmp_path / "renamed.vcf"), t.replace("\tS1", "\tT1", 1), "plain")
    with pytest.raises(gdb.GenomicsDBException, match="Sample names in the 2 file headers are different - cannot perform any further comparisons"):
        gdb.vcfdiff(gp, renamed)
    twice = vi.write_as(str(tmp_path / "twice.vcf"), g.replace("\tS1", "\tS0", 1), "plain")
    with pytest.raises(gdb.GenomicsDBException, match="duplicate sample name"):
        gdb.vcfdiff(twice, twice)
    bcf = str(tmp_path / "x.bcf")
    with open(bcf, "wb") as f:
        f.write(b"BCF\x02\x02" + b"\0" * 32)
    with pytest.raises(gdb.GenomicsDBException, match="is BCF2"):
        gdb.vcfdiff(gp, bcf)
    extra = "".join('##INFO=<ID=Z%d,Number=1,Type=Integer,Description="z">\n' % i for i in range(60))
    many = vi.write_as(str(tmp_path / "many.vcf"), t.replace("##contig", extra + "##contig", 1), "plain")
    with pytest.raises(gdb.GenomicsDBException, match="more than 64 distinct INFO names in the two headers"):
        gdb.vcfdiff(gp, many)
    for args, words in ((("-l", "x.json"), "--loader-config"), (("-p", "0"), "-p"), (("--test_to_gold_callset_map_file", "m"), "--test_to_gold_callset_map_file")):
        rc, out, err = run_tool(gdb, *(args + (gp, gp)))
        assert rc == 255 and words in err and "not in this build" in err
    rc, out, err = run_tool(gdb, gp)
    assert rc == 255 and "Needs 2 VCF files as input <gold> <test>" in err


def test_line_errors(gdb, tmp_path):
    g, t, _ = vi.make_pair(51, 3, 3, "all_neutral", 30)
    gp = vi.write_as(str(tmp_path / "g.vcf"), g, "plain")
    lines = t.split("\n")
    first = next(i for i, x in enumerate(lines) if x and not x.startswith("#"))
    def put(col, value):
        cols = lines[first + 1].split("\t")
        cols[col] = value(cols[col])
        return "\t".join(cols)
    cases = {"contig": put(0, lambda x: "chrZ"), "short": "\t".join(lines[first].split("\t")[:6]), "pos": put(1, lambda x: "1e2"),
             "info": put(7, lambda x: "NOPE=1;" + x), "format": put(8, lambda x: x + ":ZZ")}
    for what, bad in cases.items():
        mod = list(lines)
        mod[first + 1] = bad
        tp = vi.write_as(str(tmp_path / ("t_%s.vcf" % what)), "\n".join(mod), "plain")
        with pytest.raises(vm.VcfDiffError) as want:
            vm.model(gp, tp)
        assert "%s line %d" % (tp, first + 2) in str(want.value)
        with pytest.raises(gdb.GenomicsDBException) as got:
            gdb.vcfdiff(gp, tp)
        assert str(want.value) in str(got.value), what
    mod = list(lines)
    mod[first + 1], mod[first + 2] = mod[first + 2], mod[first + 1]
    tp = vi.write_as(str(tmp_path / "t_back.vcf"), "\n".join(mod), "plain")
    with pytest.raises(gdb.GenomicsDBException, match="POS goes back within contig 1 .*t_back.vcf line %d" % (first + 3)):
        gdb.vcfdiff(gp, tp)
