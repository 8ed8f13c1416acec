"""The bodies of the device vcfdiff (csrc/core/gdb_vcfdiff.hpp) and the host's share of it (csrc/host/vcfdiff_common.hpp) on the CPU,
through the stand-alone program tests/hostsim_vcfdiff (built with the address and undefined-behaviour sanitizers, run as a subprocess),
against the plain-Python model tests/tools/vcfdiff_model.py, which never calls the code under test.  The reports are equal, exactly:
on every generated pair of the device tests, on every VCF text golden against itself, with regions, and in the words of the errors.
Host code only - no device."""
import glob
import json
import os
import subprocess

import pytest

import helpers  # noqa: F401
import vcfdiff_inputs as vi
import vcfdiff_model as vm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outputs")


@pytest.fixture(scope="module")
def prog():
    from genomicsdb_amd import build as b
    return b.build_hostsim_vcfdiff()


def sim(prog, gold, test, *opts):
    r = subprocess.run([prog] + [str(o) for o in opts] + [gold, test], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.decode())


def vcf_goldens():
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "*"))):
        with open(p, "rb") as f:
            if f.read(16).startswith(b"##fileformat=VCF"):
                out.append(os.path.basename(p))
    return out


@pytest.mark.parametrize("ns,na,lines,transform", vi.pair_cases())
def test_generated_pair(prog, tmp_path, ns, na, lines, transform):
    g, t, expected = vi.make_pair(vi.seed_of(ns, na, transform), ns, na, transform, lines, exponent_floats=True)
    gp, tp = vi.write_as(str(tmp_path / "g.vcf"), g, "plain"), vi.write_as(str(tmp_path / "t.vcf.gz"), t, "gzip")
    want = vm.model(gp, tp)
    assert vi.summarize(want) == expected
    got = sim(prog, gp, tp)
    assert got["report"] == want
    assert got["pairs_light"] + got["pairs_heavy"] == want["compared"]
    assert (got["pairs_heavy"] > 0) == (na > 3 and transform in vi.PERMUTING)


def test_generator_holds_its_shapes():
    """ploidy 1, 2 and 3 in one file, G = 10, 28 and 84, the exponent-form floats"""
    g, t, _ = vi.make_pair(vi.seed_of(65, 7, "all_neutral"), 65, 7, "all_neutral", 24, exponent_floats=True)
    pl = set()
    for line in g.split("\n"):
        cols = line.split("\t")
        if not line.startswith("#") and len(cols) > 9 and cols[4].count(",") == 5:
            i = cols[8].split(":").index("PL")
            pl |= {len(c.split(":")[i].split(",")) for c in cols[9:]}
    assert {7, 28, 84} <= pl
    g4, _, _ = vi.make_pair(vi.seed_of(64, 4, "all_neutral"), 64, 4, "all_neutral", 30)
    assert any(len(c.split(":")[4].split(",")) == 10 for line in g4.split("\n") if "\tGT:AD:DP:GQ:PL:" in line for c in line.split("\t")[9:])
    assert g.count("\n") <= 300 and g != t


def test_deferred_floats(prog, tmp_path):
    g, t, _ = vi.make_pair(11, 3, 3, "float_noise", 60, exponent_floats=True)
    assert "e30" in g and "0e30" in t
    gp, tp = vi.write_as(str(tmp_path / "g.vcf"), g, "plain"), vi.write_as(str(tmp_path / "t.vcf"), t, "plain")
    got = sim(prog, gp, tp)
    assert got["report"] == vm.model(gp, tp) and got["deferred"] > 0 and got["report"]["events"] == []
    tp2 = vi.write_as(str(tmp_path / "t2.vcf"), g.replace("1.5e30", "2.5e30"), "plain")
    want = vm.model(gp, tp2)
    assert want["events"] and all(e["info"]["DIFFERS"] == ["BaseQRankSum"] for e in want["events"])
    assert sim(prog, gp, tp2)["report"] == want


@pytest.mark.parametrize("name", vcf_goldens())
def test_golden_against_itself(prog, name):
    p = os.path.join(GOLDEN, name)
    with open(p) as f:
        n = sum(1 for line in f if line.strip() and not line.startswith("#"))
    assert vm.model(p, p) == {"compared": n, "events": []}
    assert sim(prog, p, p)["report"] == {"compared": n, "events": []}


def test_t0_1_2_with_alts_swapped(prog, tmp_path):
    p = os.path.join(GOLDEN, "t0_1_2_vcf_at_0")
    with open(p) as f:
        text = f.read()
    tp = str(tmp_path / "swapped.vcf")
    with open(tp, "w") as f:
        f.write(vi.swap_first_two_alts(text))
    want = vm.model(p, tp)
    got = sim(prog, p, tp)
    assert want["events"] == [] and got["report"] == want and got["pairs_heavy"] > 0
    with open(tp, "w") as f:
        f.write(text.replace("\tA,T,<NON_REF>\t", "\tT,A,<NON_REF>\t"))
    want = vm.model(p, tp)
    assert want["events"] and all("PL" in e["format"]["DIFFERS"] for e in want["events"])
    assert sim(prog, p, tp)["report"] == want


def test_regions_and_threshold(prog, tmp_path):
    g, t, _ = vi.make_pair(21, 3, 3, "delete_line", 60)
    gp, tp = vi.write_as(str(tmp_path / "g.vcf"), g, "plain"), vi.write_as(str(tmp_path / "t.vcf"), t, "plain")
    for regions in ("2", "1:100-150,2:120", "10:130-", "1,1:5"):
        assert sim(prog, gp, tp, "-r", regions)["report"] == vm.model(gp, tp, regions=regions), regions
    g, t, _ = vi.make_pair(22, 3, 3, "float_beyond", 60)
    gp, tp = vi.write_as(str(tmp_path / "g2.vcf"), g, "plain"), vi.write_as(str(tmp_path / "t2.vcf"), t, "plain")
    for thr in (1e-5, 0.5, 10.0):
        want = vm.model(gp, tp, threshold=thr)
        assert sim(prog, gp, tp, "-t", thr)["report"] == want
    assert want["events"] == []


def test_errors_in_the_models_words(prog, tmp_path):
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
    texts = {}
    for what, bad in cases.items():
        mod = list(lines)
        mod[first + 1] = bad
        texts[what] = "\n".join(mod)
    mod = list(lines)
    mod[first + 1], mod[first + 2] = mod[first + 2], mod[first + 1]
    texts["back"] = "\n".join(mod)
    second_contig = next(i for i, x in enumerate(lines) if x.startswith("2\t"))
    mod = list(lines)
    mod.insert(second_contig + 1, lines[first])
    texts["not_contiguous"] = "\n".join(mod)
    texts["samples"] = t.replace("\tS1", "\tT1", 1)
    texts["duplicate"] = t.replace("\tS1", "\tS0", 1)
    texts["many"] = t.replace("##contig", "".join('##FORMAT=<ID=Z%d,Number=1,Type=Integer,Description="z">\n' % i for i in range(60)) + "##contig", 1)
    for what, text in texts.items():
        tp = vi.write_as(str(tmp_path / ("t_%s.vcf" % what)), text, "plain")
        with pytest.raises(vm.VcfDiffError) as want:
            vm.model(gp, tp)
        r = subprocess.run([prog, gp, tp], capture_output=True, timeout=120)
        assert r.returncode == 1 and r.stderr.decode().strip() == "VCFDiffException : " + str(want.value), what
