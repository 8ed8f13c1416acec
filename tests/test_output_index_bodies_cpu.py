"""The bodies of the device builder of the output's index (csrc/core/gdb_output_index.hpp) on the CPU (tests/hostsim_output_index): the pages
of a "z" / "b" stream as the device sees them - uncompressed bytes, record offsets, compressed size of every block of B input bytes - give the
.tbi / .csi that the host builder (gdbamd_build_output_index) writes when it re-reads the finished file, byte for byte.  The files are assembled
here with zlib; B is tiny, so that block and page boundaries are cheap to hit.  No GPU."""
import ctypes
import os
import struct
import subprocess
import zlib

import pytest

import helpers  # noqa: F401  (puts tests/tools on the path)
import tabix_reader
from genomicsdb_amd import _lib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CONTIGS = ["chr1", "chr2", "chrX", "chrUn_1", "chrUn_2"]


_built = None


def _sim():
    """(library, sanitized program) of tests/hostsim_output_index, built when it is first asked for"""
    global _built
    if _built is None:
        from genomicsdb_amd import build
        lib_path, prog = build.build_hostsim_output_index()
        L = ctypes.CDLL(lib_path)
        L.hostsim_output_index_build.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p, ctypes.c_uint64]
        _built = (L, prog)
    return _built


def bgzf_block(data):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(data) + co.flush()
    bsize = 18 + len(body) + 8 - 1
    assert bsize < 65536
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize) + body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def header_bytes(bcf):
    text = "##fileformat=VCFv4.2\n" + "".join("##contig=<ID=%s,length=250000000>\n" % c for c in CONTIGS) + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\n"
    if not bcf:
        return text.encode()
    t = text.encode() + b"\x00"
    return b"BCF\x02\x02" + struct.pack("<I", len(t)) + t


def record(bcf, contig, pos, end, pad=0):
    """one record of contig (index into CONTIGS) covering the 1-based positions [pos, end], `pad` bytes longer than the shortest one"""
    if bcf:
        shared = struct.pack("<iii", contig, pos - 1, end - pos + 1) + b"\x00" * (12 + pad)
        return struct.pack("<II", len(shared), 0) + shared
    ref = "A"
    info = "END=%d" % end if end > pos else "."
    return ("%s\t%d\t%s\t%s\t<NON_REF>\t.\t.\t%s\tGT\t./.\n" % (CONTIGS[contig], pos, "." + "i" * pad if pad else ".", ref, info)).encode()


def padded(bcf, contig, pos, end, at, length=None, until=None):
    """a record that begins at page offset `at` and is `length` bytes long, or ends at page offset `until`"""
    base = len(record(bcf, contig, pos, end))
    want = length if length is not None else until - at
    assert want >= base, (want, base)
    r = record(bcf, contig, pos, end, want - base)
    assert len(r) == want
    return r


class Stream:
    """pages -> the finished file, the case file of the harness"""

    def __init__(self, bcf, B):
        self.bcf, self.B, self.pages = bcf, B, []

    def page(self, records):
        self.pages.append(list(records))
        return self

    def cut(self, records, every):
        for i in range(0, len(records), every):
            self.page(records[i:i + every])
        return self

    def write(self, tmp_path, name):
        head = bgzf_block(header_bytes(self.bcf))
        file_bytes = bytearray(head)
        case = bytearray(b"OIDX1\0\0\0" + struct.pack("<IIQQ", int(self.bcf), self.B, len(head), header_bytes(False).count(b"\n")))
        names = "".join(c + "\n" for c in CONTIGS).encode()
        case += struct.pack("<II", len(CONTIGS), len(names)) + names + struct.pack("<I", len(self.pages))
        for recs in self.pages:
            data = b"".join(recs)
            off = [0]
            for r in recs:
                off.append(off[-1] + len(r))
            blocks = [bgzf_block(data[i:i + self.B]) for i in range(0, len(data), self.B)]
            for b in blocks:
                file_bytes += b
            case += struct.pack("<QII", len(data), len(recs), len(blocks)) + data + struct.pack("<%dQ" % len(off), *off) + struct.pack("<%dI" % len(blocks), *[len(b) for b in blocks])
        file_bytes += EOF_BLOCK
        self.file_size = len(file_bytes)
        path = str(tmp_path / (name + (".bcf" if self.bcf else ".vcf.gz")))
        open(path, "wb").write(bytes(file_bytes))
        open(path + ".case", "wb").write(bytes(case))
        return path


def host_index(path, bcf):
    assert _lib.lib().gdbamd_build_output_index(os.fsencode(path), int(bcf)) == 0, _lib.last_error()
    return open(path + (".csi" if bcf else ".tbi"), "rb").read()


STAT_NAMES = ("pages", "records", "contigs", "bins", "chunks", "windows", "atomics")


def sim_index(path, bcf):
    out = path + ".sim" + (".csi" if bcf else ".tbi")
    st = (ctypes.c_uint64 * 7)()
    err = ctypes.create_string_buffer(1024)
    rc = _sim()[0].hostsim_output_index_build(os.fsencode(path + ".case"), os.fsencode(out), st, err, 1024)
    assert rc == 0, err.value.decode()
    return open(out, "rb").read(), dict(zip(STAT_NAMES, (int(x) for x in st))), out


def check(tmp_path, stream, name="s"):
    path = stream.write(tmp_path, name)
    want = host_index(path, stream.bcf)
    got, st, out = sim_index(path, stream.bcf)
    assert got == want
    idx = tabix_reader.Index(out)
    bins = sum(len([b for b in r["bins"] if b != idx.meta_bin]) for r in idx.refs)
    chunks = sum(len(c) for r in idx.refs for b, c in r["bins"].items() if b != idx.meta_bin)
    assert (st["bins"], st["chunks"]) == (bins, chunks)
    assert st["records"] == sum(len(p) for p in stream.pages)
    return path, st, idx


FORMATS = [pytest.param(False, id="text"), pytest.param(True, id="bcf")]


@pytest.mark.parametrize("B", [97, 256])
@pytest.mark.parametrize("bcf", FORMATS)
def test_records_at_block_and_page_boundaries(tmp_path, bcf, B):
    """a record across three blocks; one that ends exactly with a block (vend = the next block, offset 0); one that ends exactly with the last
    block of a page (vend = the first block of the next page); the stream's last record (vend = file size << 16, the EOF block counted)"""
    s = Stream(bcf, B)
    p, at = [], 0
    p.append(padded(bcf, 0, 100, 200, at, length=2 * B + 10)); at += len(p[-1])          # blocks 0, 1 and 2
    p.append(padded(bcf, 0, 300, 400, at, until=4 * B)); at = 4 * B                     # ends with block 3
    p.append(record(bcf, 0, 500, 600)); at += len(p[-1])
    p.append(padded(bcf, 0, 700, 800, at, until=6 * B))                                 # ends with the page's last block
    s.page(p)
    s.page([record(bcf, 0, 900, 1000), record(bcf, 0, 40000, 40010)])
    path, st, idx = check(tmp_path, s)
    assert st["pages"] == 2
    # the last chunk ends at the file's end
    ends = sorted(ce for r in idx.refs for b, c in r["bins"].items() if b != idx.meta_bin for _, ce in c)
    assert ends[-1] == s.file_size << 16 == os.path.getsize(path) << 16


@pytest.mark.parametrize("every", [1, 7])
@pytest.mark.parametrize("B", [97, 256])
@pytest.mark.parametrize("bcf", FORMATS)
def test_page_cuts_behind_every_record_and_every_7th(tmp_path, bcf, B, every):
    """42 records: chr1 until record 14 (a page cut when every = 7), chr2 until record 24 (no cut there), then chrX; the bins change inside and at cuts"""
    recs = []
    for i in range(42):
        contig = 0 if i < 14 else 1 if i < 24 else 2
        pos = 1000 + (i // 5) * 16384 + i * 7
        recs.append(record(bcf, contig, pos, pos + (3 if i % 4 else 0)))
    s = Stream(bcf, B).cut(recs, every)
    _, st, _ = check(tmp_path, s)
    assert st["pages"] == (42 + every - 1) // every and st["contigs"] == (len(CONTIGS) if bcf else 3)
    # the cuts do not show: one page gives the same bytes through the same file? (other compressed sizes: compared through its own file)
    check(tmp_path, Stream(bcf, B).page(recs), "one")


@pytest.mark.parametrize("bcf", FORMATS)
def test_a_run_of_one_bin_across_three_pages_is_one_chunk(tmp_path, bcf):
    recs = [record(bcf, 0, 2000 + 10 * i, 2005 + 10 * i) for i in range(9)]
    _, st, _ = check(tmp_path, Stream(bcf, 97).cut(recs, 3))
    assert (st["pages"], st["bins"], st["chunks"]) == (3, 1, 1)


@pytest.mark.parametrize("bcf", FORMATS)
def test_a_reference_block_across_70_windows(tmp_path, bcf):
    recs = [record(bcf, 0, 5000, 5000), record(bcf, 0, 6000, 6000 + 70 * 16384), record(bcf, 0, 7000, 7001), record(bcf, 0, 40 * 16384, 40 * 16384 + 5),
            record(bcf, 0, 80 * 16384, 80 * 16384 + 5)]
    for every in (1, 2, 5):
        _, st, _ = check(tmp_path, Stream(bcf, 256).cut(recs, every), "e%d" % every)
        assert st["windows"] == 81 or bcf      # (.csi has no linear index of its own: the windows are those the loffsets were derived from)


def test_text_contigs_follow_first_appearance_and_one_comes_back(tmp_path):
    order = [2, 2, 0, 0, 0, 2, 2, 1, 0]      # chrX first, chr1, chrX again, chr2, chr1 again
    recs = [record(False, c, 1000 + 100 * i, 1050 + 100 * i) for i, c in enumerate(order)]
    for every in (1, 2, 4, 9):
        _, st, idx = check(tmp_path, Stream(False, 97).cut(recs, every), "e%d" % every)
        assert idx.names == ["chrX", "chr1", "chr2"] and st["contigs"] == 3


def test_bcf_ids_follow_the_header_with_unused_contig_lines(tmp_path):
    recs = [record(True, c, 1000 + 100 * i, 1050 + 100 * i) for i, c in enumerate([0, 0, 2, 2, 3])]      # chr2 and chrUn_2 stay without records
    for every in (1, 2, 5):
        _, st, idx = check(tmp_path, Stream(True, 97).cut(recs, every), "e%d" % every)
        assert len(idx.refs) == len(CONTIGS) and st["contigs"] == len(CONTIGS)
        assert [bool(r["bins"]) for r in idx.refs] == [True, False, True, True, False]


@pytest.mark.parametrize("bcf", FORMATS)
def test_a_header_only_stream(tmp_path, bcf):
    _, st, idx = check(tmp_path, Stream(bcf, 256))
    assert st["records"] == 0 and st["chunks"] == 0
    assert len(idx.refs) == (len(CONTIGS) if bcf else 0)


@pytest.mark.parametrize("bcf", FORMATS)
def test_runs_of_1_63_64_65_and_300_records_of_one_bin(tmp_path, bcf):
    """runs of one bin, each closed by a record of another bin: the window rule works in lanes of 64 neighbours"""
    recs, pos = [], 1000
    for k, n in enumerate((1, 63, 64, 65, 300)):
        base = (2 * k) * 16384
        for i in range(n):
            recs.append(record(bcf, 0, base + 100 + i, base + 100 + i))
        recs.append(record(bcf, 0, base + 16384 + 5, base + 16384 + 6))
    assert pos
    for every, name in ((len(recs), "one"), (64, "e64"), (7, "e7")):
        _, st, _ = check(tmp_path, Stream(bcf, 256).cut(recs, every), name)
        assert st["chunks"] == 10 and st["bins"] == 10
    # one page: far fewer atomics than records
    _, st, _ = check(tmp_path, Stream(bcf, 256).page(recs), "again")
    assert st["atomics"] <= 10 + len(recs) // 64 + 10


@pytest.mark.parametrize("bcf", FORMATS)
def test_the_sanitized_program_writes_the_same_index(tmp_path, bcf):
    """the same source as a stand-alone program under the address and undefined-behaviour sanitizers"""
    recs = []
    for i in range(120):
        contig = [0, 2, 3][i // 40]
        pos = 500 + (i % 40) * 3000
        recs.append(record(bcf, contig, pos, pos + (20000 if i % 13 == 0 else 2), pad=i % 5))
    s = Stream(bcf, 97).cut(recs, 7)
    path = s.write(tmp_path, "san")
    want = host_index(path, bcf)
    out = path + ".san" + (".csi" if bcf else ".tbi")
    r = subprocess.run([_sim()[1], path + ".case", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("stats pages 18 records 120 "), r.stdout + r.stderr
    assert open(out, "rb").read() == want
