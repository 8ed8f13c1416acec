"""The index of the "z" / "b" query stream built on the device page by page (kernels/gdb_output_index.hip): GenomicsDBQueryStream(..., index=True)
is read to its end and written to a file, write_index writes the .tbi / .csi, and the file equals what the host builder
(gdbamd_build_output_index) writes when it re-reads that file, byte for byte.  The statistics say that the device path ran.  Every case is a
few hundred records."""
import gzip
import json
import os
import struct
import subprocess

import pytest

import helpers
import tabix_reader
from golden_cases import CASES

pytestmark = pytest.mark.gpu

FORMATS = ["z", "b"]


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    from genomicsdb_amd import _lib
    assert _lib.lib().gdb_mi355_device_count() > 0, "no HIP device"
    return genomicsdb_amd


def n_records(path, fmt):
    plain = gzip.decompress(open(path, "rb").read())
    if fmt == "z":
        return sum(1 for l in plain.split(b"\n") if l and not l.startswith(b"#"))
    at, n = 9 + struct.unpack_from("<I", plain, 5)[0], 0
    while at < len(plain):
        l_shared, l_indiv = struct.unpack_from("<II", plain, at)
        at += 8 + l_shared + l_indiv
        n += 1
    return n


def host_index(path, fmt):
    from genomicsdb_amd import _lib
    assert _lib.lib().gdbamd_build_output_index(os.fsencode(path), int(fmt == "b")) == 0, _lib.last_error()
    with open(path + (".csi" if fmt == "b" else ".tbi"), "rb") as f:
        return f.read()


def stream_and_index(gdb, tmp_path, q, cells, fmt, name="out", **kw):
    """-> (file, stats, index read back); asserts the device index against the host builder's and the statistics against the file"""
    s = gdb.GenomicsDBQueryStream(query_json=q, cells=cells, buffer_capacity=1 << 16, output_format=fmt, index=True, **kw)
    path = str(tmp_path / (name + "." + fmt))
    with open(path, "wb") as f:
        f.write(s.read())
    dev = path + ".dev"
    st = s.write_index(dev)
    s.close()
    print(fmt, name, st)
    with open(dev, "rb") as f:
        assert f.read() == host_index(path, fmt)
    idx = tabix_reader.Index(dev)
    assert st["records"] == n_records(path, fmt)
    assert st["bins"] == sum(len([b for b in r["bins"] if b != idx.meta_bin]) for r in idx.refs)
    assert st["chunks"] == sum(len(c) for r in idx.refs for b, c in r["bins"].items() if b != idx.meta_bin)
    assert st["contigs"] == len(idx.refs)
    return path, st, idx


def golden(name):
    """a case of golden_cases by its name, else the first one that produces the golden of that name"""
    _, callsets, vid, ov, _, mode = ([c for c in CASES if c[0] == name] + [c for c in CASES if c[4] == name])[0]
    q, _ = helpers.query_json(callsets, vid, ov, mode)
    return q, helpers.cells_for(callsets, vid)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("page", [700, None])
@pytest.mark.parametrize("name", ["t0_1_2_vcf_at_0", "t6_7_8_vcf_at_0", "t0_overlapping"])
def test_goldens_one_record_per_page_and_one_page(gdb, tmp_path, monkeypatch, name, page, fmt):
    """GDBAMD_DEVICE_PAGE_BYTES=700: every chunk merge crosses a page cut; the default page: a single page"""
    if page:
        monkeypatch.setenv("GDBAMD_DEVICE_PAGE_BYTES", str(page))
    q, cells = golden(name)
    _, st, _ = stream_and_index(gdb, tmp_path, q, cells, fmt)
    assert st["records"] > 0
    if page is None:
        assert st["pages"] == 1
    elif fmt == "z":
        assert 1 < st["pages"] <= st["records"]      # (BCF2 records are shorter: those of the smallest golden fit one page of 700 bytes)


def _synth_one_contig(tmp_path, n_samples, begin, end):
    from genomicsdb_amd import synth
    B, W = begin - 1000, end - begin + 2000
    fasta = tmp_path / "ref.fa"
    with open(fasta, "wb") as f:
        f.write(b">1\n" + b"N" * B + synth.reference(B, W + 4096) + b"\n")
    q = helpers.synth_query(tmp_path, n_samples, begin, end)
    q["reference_genome"] = str(fasta)
    g = synth.Generator(n_samples, B, W)
    cells, _ = g.chunk_bytes(B + W)
    g.close()
    return q, cells


@pytest.mark.parametrize("fmt", FORMATS)
def test_synthetic_one_contig_pages_of_several_blocks_and_pages_below_a_block(gdb, tmp_path, monkeypatch, fmt):
    """40 samples over [10 009 000, 10 012 000], which crosses the 16 kb window boundary at 10 010 624.  Pages of 40 000 bytes hold several
    8 192-byte blocks with records across block boundaries; pages of 3 000 bytes are smaller than a block.  The compressed bytes differ, so each
    index is compared with the host builder's through its own file; what does not depend on the cuts is equal"""
    q, cells = _synth_one_contig(tmp_path, 40, 10_009_000, 10_012_000)
    st = {}
    for page in (40000, 3000):
        monkeypatch.setenv("GDBAMD_DEVICE_PAGE_BYTES", str(page))
        _, st[page], idx = stream_and_index(gdb, tmp_path, q, cells, fmt, name="p%d" % page)
        assert st[page]["pages"] > 3
        assert st[page]["linear_windows"] == (10_012_000 >> 14) + 1
    assert st[40000]["pages"] < st[3000]["pages"]
    for k in ("records", "bins", "linear_windows", "contigs"):
        assert st[40000][k] == st[3000][k], k


GENOME = [("1", 0, 6000), ("2", 6000, 900), ("3", 6900, 5000)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_synthetic_three_contigs_out_of_contig_order(gdb, tmp_path, monkeypatch, fmt):
    """two query intervals per contig, the contigs out of order: text contig ids follow first appearance (and a contig comes back), BCF2 ids follow the header"""
    from genomicsdb_amd import synth
    END = 11900
    fasta = tmp_path / "genome.fa"
    with open(fasta, "wb") as f:
        for name, off, ln in GENOME:
            seq = synth.reference(off, ln)
            f.write(b">" + name.encode() + b"\n" + b"\n".join(seq[i:i + 60] for i in range(0, ln, 60)) + b"\n")
    g = synth.Generator(60, 0, END, contigs=GENOME)
    cells, _ = g.chunk_bytes(END)
    g.close()
    q = helpers.synth_query(tmp_path, 60, 0, END, contigs=GENOME)
    q["reference_genome"] = str(fasta)
    q["query_column_ranges"] = [[[7000, 7400], [6100, 6300], [1000, 1500], [9000, 9300], [6500, 6700], [3000, 3400]]]
    monkeypatch.setenv("GDBAMD_DEVICE_PAGE_BYTES", "20000")
    path, st, idx = stream_and_index(gdb, tmp_path, q, cells, fmt)
    assert st["pages"] >= 6
    if fmt == "z":
        plain = gzip.decompress(open(path, "rb").read())
        lines = [l for l in plain.split(b"\n") if l and not l.startswith(b"#")]
        first_seen = []
        for l in lines:
            c = l.split(b"\t", 1)[0].decode()
            if c not in first_seen:
                first_seen.append(c)
        assert idx.names == first_seen and sorted(first_seen) == ["1", "2", "3"]
        want = [l for l in lines if l.startswith(b"3\t") and tabix_reader.vcf_interval(l.split(b"\t"))[0] < 2400 and tabix_reader.vcf_interval(l.split(b"\t"))[1] > 2100]
        assert want and tabix_reader.fetch_vcf(path, idx, "3", 2100, 2400) == want
    else:
        with_records = [k for k, r in enumerate(idx.refs) if r["bins"]]
        assert len(with_records) == 3 and with_records == sorted(with_records)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_long_reference_block_issues_few_atomics(gdb, tmp_path, monkeypatch, fmt):
    """one sample with a block of 40 000 bp, a second one with short records inside its span: the block's pieces cover several 16 kb windows, and
    the hundred neighbours of one window issue one atomicMin per wavefront, not one each"""
    import hot_record_inputs as H
    block = [H.Call(100_000, "A", [], info={"END": 140_000})]
    short = [H.Call(100_010 + 10 * i, "C", ["T"]) for i in range(100)] + [H.Call(139_000 + 100 * i, "G", ["A"]) for i in range(5)]
    cells, q = H._import(tmp_path, [block, short], 7)
    q["query_column_ranges"] = [[[99_000, 141_000]]]
    for page, name in ((None, "one"), (5000, "cut")):
        if page:
            monkeypatch.setenv("GDBAMD_DEVICE_PAGE_BYTES", str(page))
        _, st, idx = stream_and_index(gdb, tmp_path, q, cells, fmt, name=name)
        assert st["records"] >= 105 and st["linear_windows"] >= 9
        assert st["atomics"] > 0 and st["atomics"] * 10 < st["records"] * st["linear_windows"]


@pytest.mark.parametrize("fmt", FORMATS)
def test_header_only_gives_the_index_of_zero_records(gdb, tmp_path, fmt):
    q, cells = golden("t0_1_2_vcf_at_0")
    _, st, idx = stream_and_index(gdb, tmp_path, q, cells, fmt, produce_header_only=True)
    assert (st["pages"], st["records"], st["chunks"]) == (0, 0, 0)


def test_misuse_is_refused_with_its_reason_and_the_stream_goes_on(gdb, tmp_path, monkeypatch):
    monkeypatch.setenv("GDBAMD_DEVICE_PAGE_BYTES", "700")
    q, cells = golden("t0_1_2_vcf_at_0")
    plain = gdb.GenomicsDBQueryStream(query_json=q, cells=cells, output_format="")
    want = plain.read()
    plain.close()
    # an unindexed format: at construction, and on a stream that then goes on
    for fmt in ("", "bu"):
        with pytest.raises(gdb.GenomicsDBException, match="not BGZF-compressed"):
            gdb.GenomicsDBQueryStream(query_json=q, cells=cells, output_format=fmt, index=True)
    s = gdb.GenomicsDBQueryStream(query_json=q, cells=cells, output_format="")
    with pytest.raises(gdb.GenomicsDBException, match="not BGZF-compressed"):
        s.enable_index()
    with pytest.raises(gdb.GenomicsDBException, match="was not enabled"):
        s.write_index(str(tmp_path / "no.tbi"))
    assert s.read() == want
    s.close()
    # write_index before the end; enable after the first body bytes
    s = gdb.GenomicsDBQueryStream(query_json=q, cells=cells, output_format="z", index=True, buffer_capacity=256)
    head = s.read(100)
    with pytest.raises(gdb.GenomicsDBException, match="has not been read to its end"):
        s.write_index(str(tmp_path / "early.tbi"))
    assert not os.path.exists(str(tmp_path / "early.tbi"))
    rest = s.read()
    assert gzip.decompress(head + rest) == want
    path = str(tmp_path / "late.z")
    with open(path, "wb") as f:
        f.write(head + rest)
    s.write_index(path + ".dev")
    s.close()
    assert open(path + ".dev", "rb").read() == host_index(path, "z")
    s = gdb.GenomicsDBQueryStream(query_json=q, cells=cells, output_format="z")
    got = s.read(1 << 15)      # beyond the header's block: body bytes
    with pytest.raises(gdb.GenomicsDBException, match="first body page has been produced"):
        s.enable_index()
    assert gzip.decompress(got + s.read()) == want
    s.close()


def test_gt_mpi_gather_index_on_device(gdb, tmp_path):
    """-O z / -O b with --index-on-device on the workspace of test_gt_mpi_gather_writes_tbi_and_csi: the index equals the one the same command
    writes without the flag, and regions fetched through it equal a scan; the flag with stdout or an unindexed format is an error"""
    q, cells = golden("t0_1_2_vcf_at_0")
    ws = tmp_path / "ws"
    (ws / "t0_1_2").mkdir(parents=True)
    (ws / "t0_1_2" / "cells.bin").write_bytes(cells)
    q.update(workspace=str(ws), array="t0_1_2", index_output_VCF=True)
    tool = os.path.join(helpers.ROOT, "genomicsdb_amd", "gt_mpi_gather")
    qj = str(tmp_path / "q.json")

    def run(fmt, out, *flags):
        q2 = dict(q)
        if out:
            q2["vcf_output_filename"] = out
        with open(qj, "w") as f:
            json.dump(q2, f)
        return subprocess.run([tool, "-j", qj, "-O", fmt, "-p", "300", "--produce-Broad-GVCF"] + list(flags), capture_output=True, timeout=300)

    for fmt, ext in (("z", ".tbi"), ("b", ".csi")):
        files = {}
        for flags in ((), ("--index-on-device",)):
            out = str(tmp_path / ("out_%s_%d" % (fmt, len(flags))))
            r = run(fmt, out, *flags)
            assert r.returncode == 0 and b"WARNING" not in r.stderr, r.stderr.decode()[-1500:]
            files[len(flags)] = (open(out, "rb").read(), open(out + ext, "rb").read())
        assert files[0] == files[1]
        out = str(tmp_path / ("out_%s_1" % fmt))
        idx = tabix_reader.Index(out + ext)
        plain = gzip.decompress(open(out, "rb").read())
        if fmt == "z":
            lines = [l for l in plain.split(b"\n") if l and not l.startswith(b"#")]
            for beg, end in [(0, 300_000_000)] + [(tabix_reader.vcf_interval(l.split(b"\t"))[0],) * 2 for l in lines[:6]]:
                end = end + 1 if end == beg else end
                want = [l for l in lines if tabix_reader.vcf_interval(l.split(b"\t"))[0] < end and tabix_reader.vcf_interval(l.split(b"\t"))[1] > beg]
                assert tabix_reader.fetch_vcf(out, idx, "1", beg, end) == want, (beg, end)
        else:
            assert len(tabix_reader.fetch_bcf(out, idx, 0, 0, 300_000_000)) == n_records(out, "b")
    r = run("z", None, "--index-on-device")
    assert r.returncode != 0 and b"needs an output file" in r.stderr
    r = run("", str(tmp_path / "plain.vcf"), "--index-on-device")
    assert r.returncode != 0 and b"needs -O z or -O b" in r.stderr
