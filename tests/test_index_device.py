"""index_vcf: the .tbi of a bgzipped VCF built on the GPU (kernels/gdb_index.hip).  For every input of tests/index_inputs.py the file equals
what the host builder (gdbamd_build_output_index) writes for a copy of the same file, byte for byte, whatever the text budget; the counts
come from the statistics.  Each case is a file of a few hundred lines."""
import os
import random

import pytest

import helpers
import index_inputs
import tabix_reader

pytestmark = pytest.mark.gpu

CASES = index_inputs.cases()


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def host_tbi(tmp_path, data):
    from genomicsdb_amd import _lib
    p = _write(tmp_path / "host_copy.vcf.gz", data)
    assert _lib.lib().gdbamd_build_output_index(os.fsencode(p), 0) == 0, _lib.last_error()
    with open(p + ".tbi", "rb") as f:
        return f.read()


def device_tbi(tmp_path, data, budget=0, name="dev.vcf.gz"):
    import genomicsdb_amd
    p = _write(tmp_path / name, data)
    st = {}
    out = genomicsdb_amd.index_vcf(p, text_budget_bytes=budget, stats=st)
    assert out == p + ".tbi" and not os.path.exists(out + ".tmp")
    with open(out, "rb") as f:
        return f.read(), st


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_index_equals_the_host_builders_bytes(tmp_path, name):
    want = host_tbi(tmp_path, CASES[name])
    got, st = device_tbi(tmp_path, CASES[name])
    print(name, st)
    assert got == want
    assert st["batches"] <= 1 and st["members"] >= 1


def test_runs_of_one_bin_become_one_chunk_each(tmp_path):
    """runs of 1, 63, 64, 65 and 300: the run of 300 crosses a 256-thread block, the last wavefront is partial"""
    got, st = device_tbi(tmp_path, CASES["runs"])
    print(st)
    assert got == host_tbi(tmp_path, CASES["runs"])
    assert (st["records"], st["contigs"], st["bins"], st["chunks"]) == (493, 1, 5, 5)
    assert st["lines"] == 493 + 3 and st["linear_windows"] == 13


def test_a_contig_that_comes_back_keeps_its_id_and_its_chunk(tmp_path):
    got, st = device_tbi(tmp_path, CASES["contigs"])
    print(st)
    assert got == host_tbi(tmp_path, CASES["contigs"])
    assert (st["records"], st["contigs"], st["bins"], st["chunks"]) == (16, 3, 5, 5)
    idx = tabix_reader.Index(str(tmp_path / "dev.vcf.gz.tbi"))
    assert idx.names == ["a", "b", "c"]


def test_300_records_of_one_window_issue_few_atomics(tmp_path):
    got, st = device_tbi(tmp_path, CASES["windows"])
    print(st)
    assert got == host_tbi(tmp_path, CASES["windows"])
    # 305 records, the first one alone covers 70 windows: one atomic per (window, wavefront that touches it), not one per record
    assert st["records"] == 305 and 70 <= st["atomics"] < 100
    assert st["atomics"] * 100 < st["records"] * st["linear_windows"]


# (input, text budget, batches at least): the members of "batches" hold 1 500 bytes, so a budget of 2 000 makes every member a batch; the
# long line of "line_across_three_members" fills two members that are no batch of their own
@pytest.mark.parametrize("name,budget,at_least", [("batches", 2000, 5), ("batches", 4000, 3), ("runs", 4000, 3), ("windows", 3000, 3), ("info", 100, 3),
                                                  ("contigs", 1, 3), ("line_across_three_members", 1, 2)])
def test_bytes_do_not_depend_on_the_batch_cuts(tmp_path, name, budget, at_least):
    """the text budget cuts the file into batches; a bin run and a long reference block lie across the cuts"""
    one, st1 = device_tbi(tmp_path, CASES[name], 0, "one.vcf.gz")
    many, st = device_tbi(tmp_path, CASES[name], budget, "many.vcf.gz")
    print(st)
    assert st1["batches"] == 1 and st["batches"] >= at_least
    assert many == one == host_tbi(tmp_path, CASES[name])
    for k in ("lines", "records", "contigs", "bins", "chunks", "linear_windows", "text_bytes"):
        assert st[k] == st1[k], k


def test_batches_of_a_single_line(tmp_path):
    data = index_inputs.one_line_members()
    got, st = device_tbi(tmp_path, data, 1)
    print(st)
    assert got == host_tbi(tmp_path, data)
    assert st["batches"] == st["lines"] == 18 and st["members"] == 19


@pytest.mark.parametrize("name", sorted(index_inputs.refusals()))
def test_refusals_name_the_place_and_leave_nothing(tmp_path, name):
    import genomicsdb_amd
    data, words, line = index_inputs.refusals()[name]
    p = _write(tmp_path / "bad.vcf.gz", data)
    with pytest.raises(genomicsdb_amd.GenomicsDBException) as e:
        genomicsdb_amd.index_vcf(p)
    msg = str(e.value)
    assert words in msg, msg
    if line is not None:
        assert "(%s line %d)" % (p, line) in msg, msg
    assert sorted(os.listdir(tmp_path)) == ["bad.vcf.gz"]


def test_the_multi_contig_synthetic_gvcf(tmp_path):
    """the file of test_tbi_of_a_multi_contig_gvcf_finds_what_a_scan_finds through the device builder: the host builder's bytes, and the
    regions fetched through the index are what a scan finds"""
    from genomicsdb_amd import synth
    import test_vcf_index as tvi
    N = 40
    g = synth.Generator(N, 0, tvi.END, contigs=tvi.GENOME)
    cells, _ = g.chunk_bytes(tvi.END)
    q = helpers.synth_query(tmp_path, N, 0, tvi.END - 1, contigs=tvi.GENOME)
    text, nrec, _ = helpers.oracle_run_synth(q, cells, synth.SEED, with_header=True)
    data = tvi._bgzip(text)
    got, st = device_tbi(tmp_path, data, 8 << 20, "out.vcf.gz")
    print(st)
    assert got == host_tbi(tmp_path, data)
    assert st["records"] == nrec and st["contigs"] == len(tvi.GENOME) and st["batches"] >= 3
    rnd = random.Random(5)
    regions = [("1", 0, 1), ("1", 0, 60000), ("1", 16383, 16385), ("3", 49999, 50000), ("MT", 0, 4000), ("nope", 0, 10)]
    for _ in range(20):
        name, off, ln = tvi.GENOME[rnd.randrange(len(tvi.GENOME))]
        b = rnd.randrange(ln)
        regions.append((name, b, min(ln, b + rnd.choice([1, 10, 300, 5000, 40000]))))
    tvi._check_vcf(str(tmp_path / "out.vcf.gz"), text, regions)
