"""Inputs of the tabix-builder tests (tests/test_index_bodies_cpu.py, tests/test_index_device.py): VCF text and BGZF with chosen member
boundaries - the smallest files at which each piece of the device builder can go wrong.  CASES: name -> bytes of a .vcf.gz file."""
import gzip
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEADER = b"##fileformat=VCFv4.2\n##contig=<ID=1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\n"
W = 1 << 14      # a window of the linear index


def member(chunk):
    """one BGZF member of `chunk` (empty: ISIZE 0)"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(chunk) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp
            + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))


def bgzf(chunks, eof=True):
    return b"".join(member(c) for c in chunks) + (EOF_BLOCK if eof else b"")


def cut(data, at):
    """data cut at the ascending offsets `at`; an offset named twice gives an empty chunk between"""
    out, prev = [], 0
    for a in at:
        out.append(data[prev:a])
        prev = a
    out.append(data[prev:])
    return out


def even(data, n):
    return [data[i:i + n] for i in range(0, len(data), n)] or [b""]


def rec(chrom, pos, ref="A", info=".", tail=b"\tGT\t0/0"):
    return b"%s\t%d\t.\t%s\t<NON_REF>\t.\t.\t%s" % (chrom.encode(), pos, ref.encode(), info.encode()) + tail + b"\n"


def block(chrom, pos, end):
    return rec(chrom, pos, info="END=%d" % end)


def _lines(n, chrom="1", start=100, step=7):
    return b"".join(rec(chrom, start + i * step) for i in range(n))


def runs_text():
    """runs of 1, 63, 64, 65 and 300 records of one (contig, bin) each: 493 records, so the run of 300 crosses a 256-thread block and the
    last wavefront is partial; every run lies in a 16 kb window of its own -> 5 bins, 5 chunks"""
    out = HEADER
    for k, n in enumerate((1, 63, 64, 65, 300)):
        out += b"".join(rec("1", 3 * k * W + 10 + i) for i in range(n))
    return out


def contigs_text():
    """three contigs; "a" is interrupted by "b" and comes back with the bin of its last record: per contig that is one chunk, and "a" keeps id 0"""
    out = HEADER
    out += b"".join(rec("a", 100 + i) for i in range(5))
    out += b"".join(rec("b", 50 + i) for i in range(3))
    out += b"".join(rec("a", 200 + i) for i in range(4))
    out += b"".join(rec("c", 5 * W + i) for i in range(3))      # a contig whose first record is not in window 0
    out += rec("b", 9 * W)                                       # "b" again, another bin
    return out


def windows_text():
    out = HEADER
    out += block("1", 5 * W + 7, 5 * W + 70 * W)                 # a reference block over more than 64 windows; nothing in windows 0 .. 4
    out += b"".join(rec("1", 80 * W + i) for i in range(300))    # 300 records in one window
    out += rec("1", 90 * W)                                      # a gap of several empty windows
    out += block("1", (1 << 26) - 100, (1 << 26) + 100)          # across a 2^26 boundary: a bin of a higher level
    out += rec("1", (1 << 26) + 500)
    out += rec("2", 3 * W + 1, ref="ACGT")
    return out


def info_text():
    out = HEADER
    out += rec("1", 1000, info="END=5000;DP=3")
    out += rec("1", 1001, info="DP=3;END=40000;X=1")
    out += rec("1", 1002, info="DP=3;END=5000")
    out += rec("1", 1003, info="END=")
    out += rec("1", 1004, info="XEND=5")
    out += rec("1", 1005, info="END=abc")
    out += rec("1", 1006, info="END=17")                          # END below POS
    out += rec("1", 1007, info=".")
    out += b"#a comment between records\n\n"
    out += rec("1", 1008, info="DP=1;END=70000", tail=b"")        # 8 columns (7 tabs): INFO runs to the end of the line
    out += rec("1", 1009, info="END=  +33000x", tail=b"\tGT")     # blanks, a sign, digits up to the first non-digit
    out += b"1\t1010\t.\tA\n"                                     # 3 tabs: skipped
    out += b"1\t1011\t.\tACG\t.\n"                                # 4 tabs: a record, end from REF
    out += rec("1", 1012, info="END=1500\r", tail=b"")            # a carriage return belongs to the line
    out += rec("1", 1013, ref="ACGTACGT")
    return out


def batches_text():
    """a few hundred lines with a bin run and a long reference block in the middle: whatever the cuts, the same file"""
    out = HEADER
    out += _lines(120, "1", 100, 50)
    out += block("1", 8000, 8000 + 40 * W)
    out += b"".join(rec("1", 2 * W + 5 + i) for i in range(150))
    out += _lines(60, "2", 10, 900)
    out += _lines(40, "1", 60 * W, 11)
    return out


def _boundary(kind):
    a, b, c = rec("1", 100), rec("1", 200, info="END=900"), rec("1", 300)
    text = HEADER + a + b + c
    e1 = len(HEADER) + len(a)                 # behind the first record's newline
    if kind == "line_ends_with_member":
        return bgzf(cut(text, [len(HEADER), e1]))
    if kind == "line_ends_with_member_then_empty":
        return bgzf(cut(text, [len(HEADER), e1, e1]))
    if kind == "empty_member_inside_line":
        return bgzf(cut(text, [e1 + 9, e1 + 9]))
    if kind == "line_across_three_members":
        long_line = rec("1", 150, ref="ACGT" * 20, info="DP=7;END=2000")      # > 80 bytes
        t = HEADER + a + long_line + c
        at = len(HEADER) + len(a) + 5
        return bgzf(cut(t, [at, at + 40, at + 80]))
    if kind == "last_line_without_newline":
        return bgzf(even(text[:-1], 61))
    if kind == "last_line_ends_last_member":
        return bgzf(cut(text, [len(HEADER) + 3, e1 + 4]))
    if kind == "last_line_ends_last_member_no_eof":
        return bgzf(cut(text, [len(HEADER) + 3, e1 + 4]), eof=False)
    if kind == "header_only":
        return bgzf(even(HEADER, 37))
    if kind == "eof_only":
        return EOF_BLOCK
    if kind == "no_header":
        return bgzf(even(a + b + c, 50))      # the first record at virtual offset 0
    raise KeyError(kind)


BOUNDARY_KINDS = ("line_ends_with_member", "line_ends_with_member_then_empty", "empty_member_inside_line", "line_across_three_members",
                  "last_line_without_newline", "last_line_ends_last_member", "last_line_ends_last_member_no_eof", "header_only", "eof_only", "no_header")


def cases():
    out = {k: _boundary(k) for k in BOUNDARY_KINDS}
    out["runs"] = bgzf(even(runs_text(), 3000))
    out["contigs"] = bgzf(even(contigs_text(), 100))
    out["windows"] = bgzf(even(windows_text(), 2500))
    out["info"] = bgzf(even(info_text(), 90))
    out["batches"] = bgzf(even(batches_text(), 1500))
    return out


def one_line_members():
    """every line a member of its own: with a text budget of 1 byte every batch is a single line"""
    text = HEADER + _lines(9) + block("1", 500, 3 * W) + _lines(5, "2")
    return bgzf([l + b"\n" for l in text.split(b"\n")[:-1]])


def refusals():
    """name -> (bytes, what the error must say, has the error a line)"""
    good = batches_text()
    chunks = even(good, 1500)
    members = [member(c) for c in chunks]
    bad = bytearray(members[2])
    for i in range(30, 40):
        bad[i] ^= 0x5A                       # inside the DEFLATE stream: header, BSIZE and trailer stay
    damaged = b"".join(members[:2]) + bytes(bad) + b"".join(members[3:]) + EOF_BLOCK
    at = len(members[0]) + len(members[1])
    return {
        "plain_text": (good, "not a BGZF file", None),
        "plain_gzip": (gzip.compress(good), "not a BGZF file", None),
        "broken_chain": (bgzf(chunks)[:-28] + b"garbage", "byte offset %d" % len(bgzf(chunks, eof=False)), None),
        "damaged_member": (damaged, "corrupt BGZF member at byte offset %d" % at, None),
        "pos_zero": (bgzf(even(HEADER + rec("1", 5) + rec("1", 0) + rec("1", 9), 70)), "POS below 1", 5),
        "pos_2_31": (bgzf(even(HEADER + rec("1", 5) + b"\n" + rec("1", 1 << 31), 70)), "at or above 2^31", 6),
        "end_2_31": (bgzf(even(HEADER + rec("1", 5, info="END=%d" % (1 << 31)), 70)), "at or above 2^31", 4),
    }
