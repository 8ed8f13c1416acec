"""The bodies of the BGZF inflater (csrc/core/gdb_inflate.hpp) on the CPU, through the harness tests/hostsim_inflate: 64
emulated lanes run the very phases a wavefront runs (table build, serial decode, match copies, CRC32 per lane and its
combination).  Every result is compared with zlib; every malformed stream must end in an error code, never in a crash or in
bytes that are not zlib's.  Host code only - no device."""
import ctypes
import glob
import os
import random
import struct
import sys
import zlib

import pytest

import helpers

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bgzf_write  # noqa: E402

LANES = 64
# InfErr of csrc/core/gdb_inflate.hpp
(OK, E_BLOCK_TYPE, E_CODE, E_NO_EOB, E_SYMBOL, E_DISTANCE, E_OUTPUT, E_INPUT, E_STORED_LEN, E_ISIZE, E_CRC) = range(11)


@pytest.fixture(scope="module")
def sim():
    from genomicsdb_amd import build as b
    L = ctypes.CDLL(b.build_hostsim_inflate())
    c = ctypes
    L.hostsim_inflate_member.argtypes = [c.c_char_p, c.c_uint32, c.c_char_p, c.c_uint32, c.c_uint32, c.c_uint32, c.POINTER(c.c_uint32), c.POINTER(c.c_uint32)]
    L.hostsim_inflate_bgzf.argtypes = [c.c_char_p, c.c_uint64, c.c_char_p, c.c_uint64, c.POINTER(c.c_uint64), c.c_uint32, c.POINTER(c.c_uint32), c.POINTER(c.c_uint64)]
    L.hostsim_inflate_state_bytes.restype = c.c_uint32
    return L


def inflate(L, stream, isize, crc, lanes=LANES):
    """-> (err, bytes decoded, crc computed)"""
    out = ctypes.create_string_buffer(max(isize, 1))
    n, got = ctypes.c_uint32(), ctypes.c_uint32()
    err = L.hostsim_inflate_member(bytes(stream), len(stream), out, isize, crc & 0xFFFFFFFF, lanes, ctypes.byref(n), ctypes.byref(got))
    return err, out.raw[:min(n.value, isize)], got.value


def check(L, payload, stream=None, **kw):
    payload = bytes(payload)
    stream = bgzf_write.raw_deflate(payload, **kw) if stream is None else stream
    assert zlib.decompress(stream, -15) == payload
    for lanes in (LANES, 1, 7):
        err, got, crc = inflate(L, stream, len(payload), zlib.crc32(payload), lanes)
        assert err == OK, "error %d with %d lanes" % (err, lanes)
        assert got == payload and crc == zlib.crc32(payload)
    return stream


def vcf_like(n, seed=1):
    r = random.Random(seed)
    lines = []
    pos = 1000
    while sum(map(len, lines)) < n:
        pos += r.randrange(1, 300)
        lines.append("1\t%d\t.\t%s\t<NON_REF>\t.\t.\tEND=%d\tGT:DP:GQ:MIN_DP:PL\t0/0:%d:%d:%d:0,%d,%d\n"
                     % (pos, r.choice("ACGT"), pos + r.randrange(1, 200), r.randrange(60), r.randrange(99), r.randrange(60), r.randrange(120), r.randrange(1800)))
    return "".join(lines).encode()[:n]


class Bits:
    """a DEFLATE stream written by hand: bits LSB first, Huffman codes MSB first"""
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        self.v |= value << self.n
        self.n += nbits
        return self

    def code(self, code, nbits):
        for i in range(nbits - 1, -1, -1):
            self.put((code >> i) & 1, 1)
        return self

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def fixed_lit(b, sym):
    if sym < 144:
        return b.code(0x30 + sym, 8)
    if sym < 256:
        return b.code(0x190 + sym - 144, 9)
    if sym < 280:
        return b.code(sym - 256, 7)
    return b.code(0xC0 + sym - 280, 8)


def canonical(lens):
    """symbol -> (code, len) of the canonical code of RFC 1951 3.2.2"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def dynamic_block(lit_lens, dist_lens, symbols, final=True):
    """a dynamic block with the given code lengths (sent plainly, each through a 5-bit code-length code... of 19 equal
    codes that is: HCLEN = 19 with every code-length symbol at 5 bits is over-subscribed, so symbols 0..15 get 4 bits) and the
    symbols [(lit/len symbol, extra, nextra) | (.., dist symbol, extra, nextra)]"""
    b = Bits().put(1 if final else 0, 1).put(2, 2)
    b.put(len(lit_lens) - 257, 5).put(len(dist_lens) - 1, 5).put(19 - 4, 4)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = [4] * 16 + [0, 0, 0]          # 16 codes of 4 bits: complete
    for s in order:
        b.put(cl[s], 3)
    cc = canonical(cl)
    for l in list(lit_lens) + list(dist_lens):
        b.code(*cc[l])
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    for t in symbols:
        b.code(*lc[t[0]])
        if len(t) > 1:
            b.put(t[1], t[2])
        if len(t) > 3:
            b.code(*dc[t[3]])
            b.put(t[4], t[5])
    return b


# ---- well-formed members

def test_state_fits_next_to_a_member_twice_in_lds(sim):
    assert 2 * (sim.hostsim_inflate_state_bytes() + 65536 + 32) <= 160 * 1024


def test_empty_and_one_byte(sim):
    check(sim, b"")
    check(sim, b"", level=0)
    check(sim, b"x")
    check(sim, b"x", fixed=True)
    check(sim, b"x", level=0)


@pytest.mark.parametrize("size", [65536, 65280])
def test_full_members(sim, size):
    check(sim, vcf_like(size))
    check(sim, vcf_like(size, 2), level=1)


@pytest.mark.parametrize("kw", [dict(level=0), dict(fixed=True), dict(level=1), dict(level=6), dict(level=9)], ids=["stored", "fixed", "l1", "l6", "l9"])
def test_block_kinds(sim, kw):
    check(sim, vcf_like(30000, 3), **kw)
    check(sim, vcf_like(777, 4), **kw)


def test_stored_block_of_length_zero(sim):
    # Z_FULL_FLUSH ends with an empty stored block; one more by hand: final stored block, LEN 0
    stream = Bits().put(1, 1).put(0, 2).bytes() + struct.pack("<HH", 0, 0xFFFF)
    check(sim, b"", stream=stream)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    stream = c.compress(b"abc" * 100) + c.flush(zlib.Z_FULL_FLUSH) + c.flush(zlib.Z_FULL_FLUSH) + c.flush()
    check(sim, b"abc" * 100, stream=stream)


def test_several_blocks_in_one_member(sim):
    data = vcf_like(40000, 5)
    check(sim, data, flush_at=13579)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    stream = b"".join(c.compress(data[i:i + 5000]) + c.flush(zlib.Z_FULL_FLUSH if i % 10000 else zlib.Z_SYNC_FLUSH) for i in range(0, 40000, 5000)) + c.flush()
    check(sim, data, stream=stream)
    # stored, dynamic and fixed blocks in one member
    a, b_, c_ = os.urandom(300), vcf_like(9000, 6), b"tail tail tail"
    z1 = zlib.compressobj(0, zlib.DEFLATED, -15)
    z = z1.compress(a) + z1.flush(zlib.Z_FULL_FLUSH)
    z2 = zlib.compressobj(9, zlib.DEFLATED, -15)
    z += z2.compress(b_) + z2.flush(zlib.Z_FULL_FLUSH)
    z3 = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    z += z3.compress(c_) + z3.flush()
    check(sim, a + b_ + c_, stream=z)


def test_run_distance_one_length_258(sim):
    s = check(sim, b"a" * 259, fixed=True)
    assert len(s) < 10
    check(sim, b"a" * 65536)
    check(sim, b"q" + b"\0" * 60000, level=9)


def test_distance_smaller_than_length(sim):
    check(sim, b"abc" * 5000, level=9)
    check(sim, b"0123456" * 37 + b"xy" * 129, fixed=True)
    # by hand: "ab", then length 11 at distance 2, in a fixed block
    b = Bits().put(1, 1).put(1, 2)
    fixed_lit(b, ord("a")); fixed_lit(b, ord("b"))
    fixed_lit(b, 265).put(0, 1)        # length 11
    b.code(1, 5)                       # distance 2
    fixed_lit(b, 256)
    check(sim, b"ab" + b"ab" * 5 + b"a", stream=b.bytes())


def test_distance_32768(sim):
    # (zlib itself never looks further back than 32 768 - 262 bytes, so the longest distance is written by hand)
    head = vcf_like(300, 12)
    check(sim, head + random.Random(5).randbytes(32768 - 262 - 300) + head + b"end", level=9)
    # 32 768 stored bytes, then length 3 at distance 32 768 (symbol 29, 13 extra bits all ones) in a fixed block
    first = os.urandom(32768)
    b = Bits().put(1, 1).put(1, 2)
    fixed_lit(b, 257)
    b.code(29, 5).put(8191, 13)
    fixed_lit(b, 256)
    stream = b"\x00" + struct.pack("<HH", 32768, 32768 ^ 0xFFFF) + first + b.bytes()
    check(sim, first + first[:3], stream=stream)


def test_no_matches_one_zero_length_distance_code(sim):
    # distinct bytes, shuffled: zlib finds no match and sends HDIST = 1 with a code of length 0
    # from zlib: every 3 letters of this de Bruijn sequence occur once, so there is nothing to match (zlib still declares two
    # distance codes; the single zero-length one is written by hand below)
    seq, k, n = [], 4, 3
    a = [0] * (k * n)

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    data = bytes(b"ACGT"[x] for x in seq + seq[:2])
    stream = bgzf_write.raw_deflate(data, level=9)
    assert stream[0] & 6 == 4 and len(data) == 66           # a dynamic block
    check(sim, data, stream=stream)
    lens = [0] * 257
    lens[65] = lens[66] = 2; lens[67] = 2; lens[256] = 2
    b = dynamic_block(lens, [0], [(65,), (66,), (67,), (65,), (256,)])
    check(sim, b"ABCA", stream=b.bytes())


def test_single_distance_code(sim):
    # one distance code of one bit: the incomplete code RFC 1951 permits
    lens = [0] * 258
    lens[97] = 2; lens[98] = 2; lens[256] = 2; lens[257] = 2
    b = dynamic_block(lens, [1], [(97,), (98,), (257, 0, 0, 0, 0, 0), (256,)])       # length 3 at distance 1
    check(sim, b"abbbb", stream=b.bytes())
    # the unused half of that code is no code: an error, not a symbol
    b = dynamic_block(lens, [1], [(97,), (98,), (257,)])
    b.put(1, 1)
    b.code(*canonical(lens)[256]).put(0, 16)
    err, _, _ = inflate(sim, b.bytes(), 5, 0)
    assert err == E_SYMBOL
    # zlib writes one for a run
    check(sim, b"z" * 1000, level=9)


def test_fifteen_bit_codes(sim):
    # Fibonacci-like frequencies make the Huffman tree as deep as zlib lets it be
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    data = bytearray()
    for s, f in enumerate(fib):
        data += bytes([s + 40]) * min(f, 20000)
    random.Random(3).shuffle(data)
    data = bytes(data[:65000])
    stream = bgzf_write.raw_deflate(data, level=6)
    check(sim, data, stream=stream)
    # and by hand, whatever zlib chose: lengths 1, 2, .., 14, 15, 15
    lens = [0] * 257
    syms = list(range(65, 65 + 15)) + [256]
    for i, s in enumerate(syms):
        lens[s] = min(i + 1, 15)
    b = dynamic_block(lens, [0], [(s,) for s in syms[:-1]] + [(syms[-2],), (syms[-3],), (256,)])
    check(sim, bytes(syms[:-1]) + bytes([syms[-2], syms[-3]]), stream=b.bytes())


def test_random_bytes(sim):
    data = random.Random(11).randbytes(20000)
    for level in (1, 6, 9):
        check(sim, data, level=level)
    check(sim, data, fixed=True)


FIXTURES = sorted(glob.glob(os.path.join(helpers.GOLDEN, "inputs", "vcfs", "*.vcf.gz")))


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_fixture_files(sim, path):
    raw = open(path, "rb").read()
    want = b"".join(zlib.decompress(s, -15) for _, s, _, _ in bgzf_write.split_members(raw))
    dst = ctypes.create_string_buffer(len(want) + 1)
    n, err, off = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint64()
    assert sim.hostsim_inflate_bgzf(raw, len(raw), dst, len(want), ctypes.byref(n), LANES, ctypes.byref(err), ctypes.byref(off)) == 0
    assert n.value == len(want) and dst.raw[:n.value] == want and want.startswith(b"##fileformat=VCF")


def test_walk_refuses_what_is_not_bgzf(sim):
    import gzip
    dst = ctypes.create_string_buffer(1 << 16)
    n = ctypes.c_uint64()
    good = bgzf_write.bgzf(b"hello\n" * 100, member_size=50)

    def walk(buf):
        return sim.hostsim_inflate_bgzf(bytes(buf), len(buf), dst, 1 << 16, ctypes.byref(n), LANES, None, None)
    assert walk(good) == 0 and dst.raw[:n.value] == b"hello\n" * 100
    holed = bgzf_write.bgzf(b"hello\n" * 100, member_size=50, empty_member_at=5)          # an empty member in the middle
    assert len(holed) == len(good) + 28 and walk(holed) == 0 and dst.raw[:n.value] == b"hello\n" * 100
    assert walk(gzip.compress(b"hello\n" * 100)) == -1
    assert walk(b"##fileformat=VCFv4.2\n") == -1
    assert walk(b"") == -1
    assert walk(good[:-5]) == -1 and walk(good + b"\n") == -1 and walk(good[:100] + b"\0" + good[101:]) in (-1, 2, 3)
    big = bytearray(bgzf_write.member(b"x" * 10))
    big[-4:] = struct.pack("<I", 65537)
    assert walk(big) == -1


# ---- malformed members

def test_reserved_block_type(sim):
    assert inflate(sim, Bits().put(1, 1).put(3, 2).put(0, 13).bytes(), 10, 0)[0] == E_BLOCK_TYPE


def test_oversubscribed_and_incomplete_codes(sim):
    lens = [0] * 257
    lens[65] = lens[66] = lens[256] = 1                   # three codes of one bit
    assert inflate(sim, dynamic_block(lens, [0], []).bytes() + b"\0" * 8, 10, 0)[0] == E_CODE
    lens = [0] * 257
    lens[65] = 2; lens[256] = 2                           # half of the code space unused, and not the one-code case
    assert inflate(sim, dynamic_block(lens, [0], []).bytes() + b"\0" * 8, 10, 0)[0] == E_CODE
    lens = [0] * 257
    lens[65] = lens[66] = lens[67] = lens[256] = 2
    assert inflate(sim, dynamic_block(lens, [2, 2, 2], []).bytes() + b"\0" * 8, 10, 0)[0] == E_CODE       # incomplete distance code
    assert inflate(sim, dynamic_block(lens, [1, 1, 1], []).bytes() + b"\0" * 8, 10, 0)[0] == E_CODE       # over-subscribed
    # the code-length code itself: HCLEN = 4, one code of 1 bit
    b = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(1, 3).put(0, 3).put(0, 3).put(0, 3)
    assert inflate(sim, b.bytes() + b"\0" * 8, 10, 0)[0] == E_CODE
    # a repeat with nothing to repeat, and one that runs past the last length
    b = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
    for s in range(19):
        b.put(2 if s < 4 else 0, 3)                       # symbols 16, 17, 18, 0 at 2 bits
    cc = canonical([2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2])
    first = Bits(); first.v, first.n = b.v, b.n
    first.code(*cc[16]).put(0, 2)
    assert inflate(sim, first.bytes() + b"\0" * 8, 10, 0)[0] == E_CODE
    for _ in range(3):
        b.code(*cc[18]).put(127, 7)                       # 3 x 138 zeros > 258 lengths
    assert inflate(sim, b.bytes() + b"\0" * 8, 10, 0)[0] == E_CODE
    # HLIT = 30: 287 literal/length codes
    assert inflate(sim, Bits().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(0, 4).bytes() + b"\0" * 40, 10, 0)[0] == E_CODE


def test_missing_end_of_block_code(sim):
    lens = [0] * 257
    lens[65] = 1; lens[66] = 1
    assert inflate(sim, dynamic_block(lens, [0], [(65,)]).bytes() + b"\0" * 8, 10, 0)[0] == E_NO_EOB


def test_symbols_out_of_range(sim):
    for sym in (286, 287):                                # fixed code: length symbols that do not exist
        b = Bits().put(1, 1).put(1, 2)
        fixed_lit(b, ord("a")); fixed_lit(b, sym); b.put(0, 16)
        assert inflate(sim, b.bytes(), 300, 0)[0] == E_SYMBOL
    for d in (30, 31):                                    # fixed code: distance symbols that do not exist
        b = Bits().put(1, 1).put(1, 2)
        fixed_lit(b, ord("a")); fixed_lit(b, 257); b.code(d, 5).put(0, 16)
        assert inflate(sim, b.bytes(), 300, 0)[0] == E_SYMBOL


def test_distance_before_the_start(sim):
    b = Bits().put(1, 1).put(1, 2)
    fixed_lit(b, ord("a")); fixed_lit(b, 257); b.code(1, 5)      # distance 2 with one byte written
    fixed_lit(b, 256)
    assert inflate(sim, b.bytes(), 300, 0)[0] == E_DISTANCE
    b = Bits().put(1, 1).put(1, 2)
    fixed_lit(b, 257); b.code(0, 5); fixed_lit(b, 256)           # a match as the first symbol
    assert inflate(sim, b.bytes(), 300, 0)[0] == E_DISTANCE


def test_output_longer_than_isize(sim):
    data = vcf_like(5000, 8)
    for kw in (dict(level=6), dict(level=0), dict(fixed=True)):
        s = bgzf_write.raw_deflate(data, **kw)
        assert inflate(sim, s, 4999, zlib.crc32(data))[0] == E_OUTPUT
        assert inflate(sim, s, 0, 0)[0] == E_OUTPUT
        assert inflate(sim, s, 5001, zlib.crc32(data))[0] == E_ISIZE
    s = bgzf_write.raw_deflate(b"a" * 300, fixed=True)         # a match that crosses ISIZE
    assert inflate(sim, s, 200, 0)[0] == E_OUTPUT


def test_input_exhausted(sim):
    data = vcf_like(5000, 9)
    for kw in (dict(level=6), dict(level=0), dict(fixed=True)):
        s = bgzf_write.raw_deflate(data, **kw)
        for cut in (0, 1, 2, 3, 5, 40, len(s) // 2, len(s) - 1):
            assert inflate(sim, s[:cut], 5000, zlib.crc32(data))[0] == E_INPUT, (kw, cut)


def test_len_nlen_mismatch(sim):
    s = bytearray(bgzf_write.raw_deflate(b"stored bytes", level=0))
    s[3] ^= 0x10
    assert inflate(sim, bytes(s), 12, zlib.crc32(b"stored bytes"))[0] == E_STORED_LEN


def test_crc_and_isize_are_verified(sim):
    data = vcf_like(3000, 10)
    s = bgzf_write.raw_deflate(data)
    assert inflate(sim, s, 3000, zlib.crc32(data) ^ 1)[0] == E_CRC
    assert inflate(sim, s, 3000, zlib.crc32(data))[0] == OK


def _zlib(stream):
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream)
        return out if d.eof else None
    except zlib.error:
        return None


def test_two_thousand_mutations(sim):
    r = random.Random(2024)
    bases = []
    for kw, n in ((dict(level=6), 6000), (dict(level=1), 3000), (dict(fixed=True), 800), (dict(level=0), 500), (dict(level=9, flush_at=700), 2500)):
        data = vcf_like(n, n)
        bases.append((data, bgzf_write.raw_deflate(data, **kw)))
    ok = errors = 0
    for k in range(2000):
        data, s = bases[k % len(bases)]
        s = bytearray(s)
        at = r.randrange(len(s)) if k % 3 else r.randrange(min(len(s), 120))      # a third of them in the block header
        if k % 2:
            s[at] ^= 1 << r.randrange(8)
        else:
            s[at] = (s[at] + 1 + r.randrange(255)) & 0xFF
        err, got, crc = inflate(sim, bytes(s), len(data), zlib.crc32(data))
        if err == OK:
            assert got == data and crc == zlib.crc32(data)          # zlib's bytes of the unmutated stream, with their CRC
            ok += 1
        else:
            assert 1 <= err <= E_CRC
            want = _zlib(bytes(s))
            assert want is None or want != data, "zlib inflates this to the original, the bodies say error %d" % err
            errors += 1
    assert ok + errors == 2000 and errors > 1500
