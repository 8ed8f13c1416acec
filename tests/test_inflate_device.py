"""BGZF input inflated on the device (csrc/kernels/gdb_inflate.hip): bgzf_decompress against zlib on hand-made and zlib-made
members, on its own compressor's output and on corrupted buffers; import_cells(device=0) on bgzip'ed gVCFs - compressed bytes
cross the link, the device inflates, the cells are the host importer's byte for byte - with the fall-backs and refusals."""
import gzip
import json
import os
import shutil
import struct
import subprocess
import sys
import zlib

import pytest

import helpers
from golden_cases import CASES

pytestmark = pytest.mark.gpu

INPUTS = os.path.join(helpers.GOLDEN, "inputs")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bgzf_write  # noqa: E402
import test_inflate_bodies_cpu as bodies  # noqa: E402  (the hand-made streams)


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


def _hand_made_members():
    """(payload, member) of every member case of tests/test_inflate_bodies_cpu.py"""
    import random
    out = []

    def z(payload, **kw):
        out.append((payload, bgzf_write.member(payload, **kw)))

    def hand(payload, stream):
        assert zlib.decompress(stream, -15) == payload
        out.append((payload, bgzf_write.wrap(stream, payload)))
    z(b"")
    z(b"x")
    z(bodies.vcf_like(65536))
    z(bodies.vcf_like(65280, 2), level=1)
    for kw in (dict(level=0), dict(fixed=True), dict(level=6), dict(level=9)):
        z(bodies.vcf_like(30000, 3), **kw)
    hand(b"", bodies.Bits().put(1, 1).put(0, 2).bytes() + struct.pack("<HH", 0, 0xFFFF))       # stored block of length 0
    z(bodies.vcf_like(40000, 5), flush_at=13579)                                              # several blocks
    z(b"a" * 259, fixed=True)                                                                 # distance 1, length 258
    z(b"a" * 65536)
    z(b"abc" * 5000, level=9)                                                                 # distance < length
    first = random.Random(1).randbytes(32768)                                                 # distance 32 768
    b = bodies.Bits().put(1, 1).put(1, 2)
    bodies.fixed_lit(b, 257)
    b.code(29, 5).put(8191, 13)
    bodies.fixed_lit(b, 256)
    hand(first + first[:3], b"\x00" + struct.pack("<HH", 32768, 32768 ^ 0xFFFF) + first + b.bytes())
    lens = [0] * 257                                                                          # no distance code at all
    lens[65] = lens[66] = lens[67] = lens[256] = 2
    hand(b"ABCA", bodies.dynamic_block(lens, [0], [(65,), (66,), (67,), (65,), (256,)]).bytes())
    lens = [0] * 258                                                                          # a single distance code
    lens[97] = lens[98] = lens[256] = lens[257] = 2
    hand(b"abbbb", bodies.dynamic_block(lens, [1], [(97,), (98,), (257, 0, 0, 0, 0, 0), (256,)]).bytes())
    lens = [0] * 257                                                                          # 15-bit codes
    syms = list(range(65, 65 + 15)) + [256]
    for i, s in enumerate(syms):
        lens[s] = min(i + 1, 15)
    hand(bytes(syms[:-1]) + bytes([syms[-2], syms[-3]]), bodies.dynamic_block(lens, [0], [(s,) for s in syms[:-1]] + [(syms[-2],), (syms[-3],), (256,)]).bytes())
    z(b"")                                                                                    # an empty member in the middle
    z(random.Random(11).randbytes(20000))
    return out


def test_member_cases_in_one_buffer(gdb):
    cases = _hand_made_members()
    buf = b"".join(m for _, m in cases) + bgzf_write.EOF
    want = b"".join(p for p, _ in cases)
    got, ms = gdb.bgzf_decompress(buf)
    assert got == want and ms > 0
    assert gdb.bgzf_decompress(bgzf_write.EOF)[0] == b""


@pytest.fixture(scope="module")
def text3m():
    import synth_gvcf_text
    import random
    import tempfile
    d = tempfile.mkdtemp(prefix="inflate_text")
    try:
        synth_gvcf_text.write_vcf(os.path.join(d, "a.vcf"), ["S"], 30000, random.Random(99))
        t = open(os.path.join(d, "a.vcf"), "rb").read()
    finally:
        shutil.rmtree(d)
    while len(t) < 3 << 20:
        t += t
    return t[:3 << 20]


@pytest.mark.parametrize("member_size", [65280, 700])
@pytest.mark.parametrize("kw", [dict(level=1), dict(level=6), dict(level=9), dict(fixed=True), dict(level=0)], ids=["l1", "l6", "l9", "fixed", "stored"])
def test_three_mib_of_vcf_text(gdb, text3m, kw, member_size):
    buf = bgzf_write.bgzf(text3m, member_size=member_size, **kw)
    want = b"".join(zlib.decompress(s, -15) for _, s, _, _ in bgzf_write.split_members(buf))
    assert want == text3m
    got, _ = gdb.bgzf_decompress(buf)
    assert len(got) == len(want) and got == want


@pytest.mark.parametrize("vcf_text", [False, True], ids=["byte_level_kernel", "anchored_text_kernel"])
def test_inverts_the_projects_own_compressor(gdb, text3m, vcf_text):
    data = text3m[:1 << 20]
    z, _ = gdb.bgzf_compress(data, vcf_text=vcf_text)
    assert gdb.bgzf_decompress(z)[0] == data
    assert gdb.bgzf_decompress(z + gdb.BGZF_EOF)[0] == data


def test_corrupted_buffers_are_refused_with_the_offset(gdb, text3m):
    data = text3m[:200000]
    buf = bgzf_write.bgzf(data, member_size=65280)
    members = bgzf_write.split_members(buf)
    third = members[2][0]
    end_of_third = members[3][0]

    def refused(bad, offset):
        with pytest.raises(gdb.GenomicsDBException) as e:
            gdb.bgzf_decompress(bytes(bad))
        assert "offset %d" % offset in str(e.value), str(e.value)
    bad = bytearray(buf); bad[end_of_third - 8] ^= 1                 # CRC32
    refused(bad, third)
    bad = bytearray(buf); bad[end_of_third - 4:end_of_third] = struct.pack("<I", members[2][3] - 1)      # ISIZE too small
    refused(bad, third)
    bad = bytearray(buf); bad[end_of_third - 4:end_of_third] = struct.pack("<I", members[2][3] + 1)      # ISIZE too large
    refused(bad, third)
    bad = bytearray(buf); bad[third + 18 + 5000] ^= 0x10             # a payload bit
    refused(bad, third)
    last = members[-2][0]                                            # the last data member, truncated: in the file, and inside its BSIZE
    refused(buf[:len(buf) - 28 - 100], last)
    stream = members[-2][1]
    refused(buf[:last] + bgzf_write.wrap(stream[:len(stream) // 2], data[-members[-2][3]:]) + bgzf_write.EOF, last)
    assert gdb.bgzf_decompress(buf)[0] == data                       # the engine is still usable


# ---- import_cells

def _bgzf_copy(src_dir, dst_dir, rewrite):
    os.makedirs(dst_dir)
    sizes = 0
    for p in sorted(os.listdir(src_dir)):
        raw = open(os.path.join(src_dir, p), "rb").read()
        if p.endswith(".vcf"):
            raw = rewrite(raw)
            sizes += len(raw)
        with open(os.path.join(dst_dir, p), "wb") as f:
            f.write(raw)
    return os.path.join(dst_dir, "vid.json"), os.path.join(dst_dir, "callsets.json"), sizes


def _record_begin(text):
    at = 0
    while text[at:at + 1] in (b"#", b"\n"):
        at = text.index(b"\n", at) + 1
    return at


def _long_header(text):
    """more '##' lines, so that the header is longer than a small member"""
    first, rest = text.split(b"\n", 1)
    return first + b"\n" + b"".join(b"##padding=<ID=P%02d,Description=\"a header line that no importer reads\">\n" % k for k in range(30)) + rest


def _header_on_a_member_boundary(text):
    text = _long_header(text)
    rb = _record_begin(text)
    return bgzf_write.bgzf(text[:rb], member_size=700, level=1)[:-28] + bgzf_write.bgzf(text[rb:], member_size=700, level=1)


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    import synth_gvcf_text
    d = str(tmp_path_factory.mktemp("synth_inflate"))
    plain = os.path.join(d, "plain")
    v, c = synth_gvcf_text.write_inputs(plain, n_files=6, n_lines=2000, multi=3)
    out = {"plain": (plain, v, c, 0)}
    for name, rewrite in (("l6_65280", lambda t: bgzf_write.bgzf(t, member_size=65280, level=6)),
                          ("l1_700", lambda t: bgzf_write.bgzf(_long_header(t), member_size=700, level=1, empty_member_at=9)),      # and an empty member between two windows
                          ("boundary", _header_on_a_member_boundary)):
        dd = os.path.join(d, name)
        v2, c2, sizes = _bgzf_copy(plain, dd, rewrite)
        out[name] = (dd, v2, c2, sizes)
    # what the inputs are meant to be: header over several small members, first record inside one, lines that straddle members,
    # and in "boundary" a member that ends exactly where the header does
    text = _long_header(open(os.path.join(plain, "s0000.g.vcf"), "rb").read())
    rb = _record_begin(text)
    assert rb % 700 != 0 and rb > 700
    ends = [i + 1 for i in range(len(text)) if text[i] == 10]
    assert sum(1 for e in ends if e % 700 == 0) < len(ends) // 100
    small = bgzf_write.split_members(open(os.path.join(out["l1_700"][0], "s0000.g.vcf"), "rb").read())
    assert len(small) > 100 and small[9][3] == 0
    acc = [0]
    for m in bgzf_write.split_members(open(os.path.join(out["boundary"][0], "s0000.g.vcf"), "rb").read()):
        acc.append(acc[-1] + m[3])
    assert rb in acc
    return out


@pytest.fixture(scope="module")
def host_cells(gdb, synth):
    """the host importer's cells of the plain-text files, computed once: whole, and the two column partitions"""
    d, v, c, _ = synth["plain"]
    cut = 2500000
    return {(): gdb.import_cells(v, c, file_root=d), ("lo",): gdb.import_cells(v, c, file_root=d, column_begin=0, column_end=cut - 1),
            ("hi",): gdb.import_cells(v, c, file_root=d, column_begin=cut)}


PARTS = {(): {}, ("lo",): dict(column_begin=0, column_end=2500000 - 1), ("hi",): dict(column_begin=2500000)}


@pytest.mark.parametrize("part", list(PARTS), ids=["whole", "columns_below_the_cut", "columns_from_the_cut"])
@pytest.mark.parametrize("budget", [256, 0])
@pytest.mark.parametrize("variant", ["l6_65280", "l1_700", "boundary"])
def test_import_of_bgzf_files(gdb, synth, host_cells, variant, budget, part):
    d, v, c, sizes = synth[variant]
    n_files = 7
    st = {}
    got = gdb.import_cells(v, c, file_root=d, device=0, text_budget_bytes=budget, stats=st, **PARTS[part])
    want = host_cells[part]
    assert got[1] == want[1] and len(got[0]) == len(want[0])
    assert got[0] == want[0]
    assert st["num_device_members"] > 0 and st["num_host_inflated_files"] == 0 and st["compressed_bytes"] == sizes and st["num_files"] == n_files
    assert st["ms_inflate"] > 0 and sizes // 2 < st["bytes_h2d"] < st["text_bytes"]       # compressed bytes cross the link, not text
    if variant != "l6_65280":
        assert st["num_device_members"] > 100 * n_files
    if part == ("hi",):
        assert st["num_spanning_cells"] > 0


def test_inflate_on_the_host_gives_the_same_bytes(gdb, synth, host_cells):
    d, v, c, sizes = synth["l6_65280"]
    st = {}
    got = gdb.import_cells(v, c, file_root=d, device=0, stats=st, inflate="host")
    assert got == host_cells[()]
    assert st["num_device_members"] == 0 and st["num_host_inflated_files"] == 7 and st["ms_inflate"] == 0 and st["compressed_bytes"] == sizes
    assert st["bytes_h2d"] == st["text_bytes"]
    with pytest.raises(ValueError):
        gdb.import_cells(v, c, file_root=d, device=0, inflate="gpu")


@pytest.mark.parametrize("kernel", ["wave", "thread"])
def test_both_inflate_kernels_import_the_same_bytes(gdb, synth, host_cells, monkeypatch, kernel):
    monkeypatch.setenv("GDBAMD_INFLATE_KERNEL", kernel)      # the A/B of profiles/device_inflate.md
    d, v, c, _ = synth["l6_65280"]
    st = {}
    assert gdb.import_cells(v, c, file_root=d, device=0, stats=st, inflate="device") == host_cells[()]
    assert st["num_device_members"] > 0


def test_plain_gzip_falls_back_and_plain_text_is_unchanged(gdb, synth, host_cells, tmp_path):
    plain = synth["plain"][0]
    d = str(tmp_path / "mixed")
    shutil.copytree(synth["l6_65280"][0], d)
    text = open(os.path.join(plain, "s0001.g.vcf"), "rb").read()
    with open(os.path.join(d, "s0001.g.vcf"), "wb") as f:
        f.write(gzip.compress(text))
    shutil.copy(os.path.join(plain, "s0002.g.vcf"), os.path.join(d, "s0002.g.vcf"))
    v, c = os.path.join(d, "vid.json"), os.path.join(d, "callsets.json")
    st = {}
    assert gdb.import_cells(v, c, file_root=d, device=0, stats=st) == host_cells[()]
    assert st["num_host_inflated_files"] == 2 and st["num_device_members"] > 0
    with pytest.raises(gdb.GenomicsDBException, match="s0001.g.vcf is not a BGZF file"):
        gdb.import_cells(v, c, file_root=d, device=0, inflate="device")
    # every file as plain text: nothing is inflated anywhere, the bytes are today's
    st = {}
    p = synth["plain"]
    assert gdb.import_cells(p[1], p[2], file_root=p[0], device=0, stats=st) == host_cells[()]
    assert st["num_host_inflated_files"] == 7 and st["num_device_members"] == 0


def test_a_corrupted_member_refuses_the_import(gdb, synth, tmp_path):
    d = str(tmp_path / "bad")
    shutil.copytree(synth["l6_65280"][0], d)
    path = os.path.join(d, "s0003.g.vcf")
    raw = bytearray(open(path, "rb").read())
    members = bgzf_write.split_members(bytes(raw))
    assert len(members) > 3
    at = members[2][0]
    raw[at + 18 + 4000] ^= 0x04
    with open(path, "wb") as f:
        f.write(raw)
    v, c = os.path.join(d, "vid.json"), os.path.join(d, "callsets.json")
    for budget in (0, 256):
        with pytest.raises(gdb.GenomicsDBException) as e:
            gdb.import_cells(v, c, file_root=d, device=0, text_budget_bytes=budget)
        assert path in str(e.value) and "byte offset %d" % at in str(e.value) and "VCF2BinaryException" in str(e.value)
    # a bad member among those the host inflates for the header is refused in the same words
    raw = bytearray(open(os.path.join(synth["l6_65280"][0], "s0003.g.vcf"), "rb").read())
    raw[18 + 300] ^= 0x04
    with open(path, "wb") as f:
        f.write(raw)
    with pytest.raises(gdb.GenomicsDBException) as e:
        gdb.import_cells(v, c, file_root=d, device=0)
    assert path in str(e.value) and "byte offset 0 " in str(e.value)
    # and a later import still works
    good = synth["l6_65280"]
    assert gdb.import_cells(good[1], good[2], file_root=good[0], device=0)[1] > 0


def test_errors_still_name_file_and_line(gdb, tmp_path):
    import synth_gvcf_text
    v, c = synth_gvcf_text.write_inputs(str(tmp_path), n_files=1, n_lines=300, multi=0, seed=5)
    p = tmp_path / "s0000.g.vcf"
    text = p.read_text().split("\n")
    first = next(i for i, l in enumerate(text) if l and not l.startswith("#"))
    cols = text[first + 200].split("\t")
    cols[0] = "chrUn_7"
    text[first + 200] = "\t".join(cols)
    bgzf_write.write_file(str(p), "\n".join(text).encode(), member_size=700, level=1)
    for budget in (256, 0):
        with pytest.raises(gdb.GenomicsDBException) as e:
            gdb.import_cells(v, c, file_root=str(tmp_path), device=0, text_budget_bytes=budget)
        assert "contig chrUn_7 is not in the vid mapping" in str(e.value) and str(p) in str(e.value) and "line %d" % (first + 200 + 1) in str(e.value)


def test_final_line_without_newline(gdb, tmp_path):
    import synth_gvcf_text
    v, c = synth_gvcf_text.write_inputs(str(tmp_path), n_files=1, n_lines=200, multi=0, seed=6)
    p = tmp_path / "s0000.g.vcf"
    text = p.read_bytes().rstrip(b"\n")
    p.write_bytes(text)
    want = gdb.import_cells(v, c, file_root=str(tmp_path))
    bgzf_write.write_file(str(p), text, member_size=700, level=1)
    for budget in (256, 0):
        st = {}
        assert gdb.import_cells(v, c, file_root=str(tmp_path), device=0, text_budget_bytes=budget, stats=st) == want
        assert st["num_device_members"] > 0 and st["num_records"] == 200


@pytest.mark.parametrize("budget", [256, 0])
def test_reference_fixtures(gdb, budget):
    v, c = os.path.join(INPUTS, "vid.json"), os.path.join(INPUTS, "callsets", "t0_1_2.json")
    files = {cs["filename"] for cs in json.load(open(c))["callsets"].values()}
    sizes = sum(os.path.getsize(os.path.join(helpers.GOLDEN, f)) for f in files)
    want = gdb.import_cells(v, c, file_root=helpers.GOLDEN)
    for kw in ({}, dict(column_begin=0, column_end=12199), dict(column_begin=12200)):
        st = {}
        got = gdb.import_cells(v, c, file_root=helpers.GOLDEN, device=0, text_budget_bytes=budget, stats=st, inflate="device", **kw)
        assert got == gdb.import_cells(v, c, file_root=helpers.GOLDEN, **kw)
        assert st["num_device_members"] > 0 and st["num_host_inflated_files"] == 0 and st["compressed_bytes"] == sizes
    assert want[0] == helpers.cells_for("t0_1_2.json", "vid.json")


def test_vcf2tiledb_with_and_without_inflate_on_host(gdb, tmp_path):
    name, callsets, vid, ov, golden, mode = [c for c in CASES if c[0] == "t0_1_2_loading"][0]
    tool = os.path.join(os.path.dirname(gdb.__file__), "vcf2tiledb")
    outs = {}
    for flag in ("device", "host"):
        ws = tmp_path / flag
        ws.mkdir()
        loader = {"row_based_partitioning": False, "produce_combined_vcf": False, "produce_tiledb_array": True,
                  "column_partitions": [{"begin": ov.get("partition_begin", 0), "workspace": str(ws), "array": "arr"}],
                  "callset_mapping_file": os.path.join("inputs", "callsets", callsets), "vid_mapping_file": os.path.join("inputs", vid),
                  "treat_deletions_as_intervals": True}
        lj = ws / "loader.json"
        lj.write_text(json.dumps(loader))
        r = subprocess.run([tool, "--import-on-device"] + (["--inflate-on-host"] if flag == "host" else []) + [str(lj)], cwd=helpers.GOLDEN, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        line = [l for l in r.stderr.decode().splitlines() if ",vcf2binary_inflate," in l][0].split(",")
        members, host_files = int(line[line.index("device_members") + 1]), int(line[line.index("host_inflated_files") + 1])
        assert (members > 0 and host_files == 0) if flag == "device" else (members == 0 and host_files > 0)
        outs[flag] = (ws / "arr" / "cells.bin").read_bytes()
    assert outs["device"] == outs["host"] and len(outs["host"]) > 0
