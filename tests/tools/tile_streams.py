"""DEFLATE streams for the tile inflater of compressed fragment files (csrc/core/gdb_tile_inflate.hpp): the hand-made case list, a
small grid of zlib-made streams and seeded mutations of them - shared by tests/test_tile_inflate_bodies_cpu.py (the body on the CPU)
and tests/test_tile_inflate_device.py (the kernel).  The bit writer and the code builders are those of test_inflate_bodies_cpu.py.

A token list is what a block decodes to: an int is a literal, (length, distance) a match written with the symbols a compressor would
choose, ("sym", length symbol, extra, distance symbol or None, extra) a match by explicit symbols, ("raw", value, nbits) bits as
they are."""
import collections
import random
import struct
import zlib

from test_inflate_bodies_cpu import Bits, fixed_lit, canonical, dynamic_block, vcf_like  # noqa: F401

TILE = 8192
# TileErr of csrc/core/gdb_tile_inflate.hpp
(OK, E_BLOCK_TYPE, E_CODE, E_NO_EOB, E_SYMBOL, E_DISTANCE, E_OUTPUT, E_INPUT, E_STORED_LEN, E_SIZE) = range(10)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

Case = collections.namedtuple("Case", "name stream want expect payload")      # expect: the TileErr; OK = zlib accepts it as `want` bytes, which are `payload`


def zlib_verdict(stream, want):
    """zlib's bytes when it takes `stream` as a complete raw DEFLATE stream of exactly `want` bytes (bytes behind the final block are
    ignored, as inflate with Z_FINISH does), else None"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(stream), want + 1)
    except zlib.error:
        return None
    return out if d.eof and len(out) == want else None


def len_code(length):
    if length == 258:
        return 285, 0, 0
    i = max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + i, length - LEN_BASE[i], LEN_EXTRA[i]


def dist_code(dist):
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, dist - DIST_BASE[i], DIST_EXTRA[i]


def _match(t):
    """-> (length symbol, extra, nextra, distance symbol or None, extra, nextra)"""
    if t[0] == "sym":
        _, ls, le, ds, de = t
        return ls, le, (LEN_EXTRA[ls - 257] if 257 <= ls <= 285 else 0), ds, de, (DIST_EXTRA[ds] if ds is not None and ds < 30 else 0)
    return len_code(t[0]) + dist_code(t[1])


def model(tokens, before=b""):
    """the bytes a token list decodes to behind `before` (well-formed tokens only)"""
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif t[0] != "raw":
            ls, le, _, ds, de, _ = _match(t)
            length, dist = LEN_BASE[ls - 257] + le, DIST_BASE[ds] + de
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(before):])


def _put_tokens(b, tokens, lit, dist):
    for t in tokens:
        if isinstance(t, int):
            lit(t)
        elif t[0] == "raw":
            b.put(t[1], t[2])
        else:
            ls, le, lne, ds, de, dne = _match(t)
            lit(ls)
            b.put(le, lne)
            if ds is not None:
                dist(ds)
                b.put(de, dne)


def fixed_block(tokens, final=True, b=None, eob=True):
    b = Bits() if b is None else b
    b.put(1 if final else 0, 1).put(1, 2)
    _put_tokens(b, tokens, lambda s: fixed_lit(b, s), lambda s: b.code(s, 5))
    if eob:
        fixed_lit(b, 256)
    return b


def stored_block(data, final=True, b=None, length=None, nlen=None):
    b = Bits() if b is None else b
    b.put(1 if final else 0, 1).put(0, 2)
    b.put(0, (-b.n) % 8)
    length = len(data) if length is None else length
    b.put(length, 16).put((length ^ 0xFFFF) if nlen is None else nlen, 16)
    b.put(int.from_bytes(bytes(data), "little"), 8 * len(data))
    return b


def dyn_block(tokens, lit_lens, dist_lens, final=True, b=None, cl_lens=None, ops=None, eob=True):
    """a dynamic block: the header with the code-length code `cl_lens` (19 lengths; default: 0..15 at 4 bits) and the code-length
    symbols `ops` [(symbol,) or (16 | 17 | 18, extra)] (default: every length sent plainly), then the tokens and the end-of-block code"""
    b = Bits() if b is None else b
    b.put(1 if final else 0, 1).put(2, 2)
    b.put(len(lit_lens) - 257, 5).put(len(dist_lens) - 1, 5).put(19 - 4, 4)
    cl_lens = [4] * 16 + [0, 0, 0] if cl_lens is None else cl_lens
    for s in ORDER:
        b.put(cl_lens[s], 3)
    ops = [(l,) for l in list(lit_lens) + list(dist_lens)] if ops is None else ops
    if ops:
        cc = canonical(cl_lens)
        for op in ops:
            b.code(*cc[op[0]])
            if op[0] >= 16:
                b.put(op[1], {16: 2, 17: 3, 18: 7}[op[0]])
    if tokens or eob:
        lc, dc = canonical(lit_lens), canonical(dist_lens)
        _put_tokens(b, tokens, lambda s: b.code(*lc[s]), lambda s: b.code(*dc[s]))
        if eob:
            b.code(*lc[256])
    return b


def pad(b, nbytes=12):
    """zero bytes behind a stream that is refused before its end: the refusal must not be for want of input"""
    return b.put(0, (-b.n) % 8 + 8 * nbytes)


def lens_of(n, d):
    out = [0] * n
    for s, l in d.items():
        out[s] = l
    return out


def hand_made_cases():
    """the streams chosen for this decoder: [Case]"""
    r = random.Random(1951)
    rb = lambda n: bytes(r.randrange(256) for _ in range(n))
    C = []

    def ok(name, b, payload):
        C.append(Case(name, b.bytes() if isinstance(b, Bits) else bytes(b), len(payload), OK, bytes(payload)))
        return payload

    def bad(name, b, want, err):
        C.append(Case(name, b.bytes() if isinstance(b, Bits) else bytes(b), want, err, None))

    # ---- stream ends and refill(): the byte loop of the last 8 bytes
    long_fixed = fixed_block(list(rb(40))).bytes()
    for k in range(18):
        if k >= 2:
            data = rb(k - 2)
            data = bytes(x & 0x7F for x in data)                   # (8-bit codes: 3 + 8 m + 7 bits = m + 2 bytes)
            b = fixed_block(list(data))
            assert len(b.bytes()) == k
            ok("fixed block of %d bytes" % k, b, data)
        if k >= 5:
            data = rb(k - 5)
            b = stored_block(data)
            assert len(b.bytes()) == k
            ok("stored block of %d bytes" % k, b, data)
        bad("first %d bytes of a fixed block" % k, long_fixed[:k], 40, E_INPUT)
    data = bytes([200, 201, 202, 203, 204, 205, 1, 2, 3])          # six 9-bit codes: the end-of-block code is the last 7 bits of the last byte
    b = fixed_block(list(data))
    assert b.n % 8 == 0
    ok("end-of-block code in the last 7 bits", b, data)
    text = vcf_like(3000, 11)
    co = zlib.compressobj(9, zlib.DEFLATED, -15)
    dyn = co.compress(text) + co.flush()
    assert (dyn[0] >> 1) & 3 == 2
    ok("dynamic stream of zlib", dyn, text)
    for cut in sorted(set([0, 1, 2, 3, 5, len(dyn) // 2] + list(range(len(dyn) - 16, len(dyn))))):
        bad("dynamic stream cut at byte %d" % cut, dyn[:cut], len(text), E_INPUT)
    for extra in (1, 7, 8, 9, 40):
        ok("%d bytes behind the final block" % extra, dyn + rb(extra), text)
        ok("%d bytes behind a final fixed block" % extra, fixed_block(list(b"tail")).bytes() + b"\xff" * extra, b"tail")

    # ---- stored blocks
    for j in range(8):                                             # j 9-bit literals in front: the stored header begins at bit (2 + j) % 8
        front = bytes([150 + i for i in range(j)]) + b"AB"
        b = fixed_block(list(front), final=False)
        assert b.n % 8 == (2 + j) % 8
        body = rb(33)
        ok("stored header at bit offset %d" % (b.n % 8), stored_block(body, b=b), front + body)
    ok("stored block of LEN 0, final", stored_block(b""), b"")
    ok("stored block of LEN 0, not final", fixed_block([], b=stored_block(b"", final=False)), b"")
    ok("stored block of LEN 0 between literals", fixed_block([66], b=stored_block(b"", final=False, b=fixed_block([65], final=False))), b"AB")
    body = rb(100)
    ok("stored LEN equal to what is left of the tile", stored_block(body, b=fixed_block([1, 2, 3], final=False)), b"\x01\x02\x03" + body)
    body = rb(TILE)
    ok("one stored block of 8192", stored_block(body), body)
    bad("stored LEN one more than what is left", stored_block(rb(101), b=fixed_block([1, 2, 3], final=False)), 103, E_OUTPUT)
    bad("one stored block of 8192 into 8191", stored_block(body), TILE - 1, E_OUTPUT)
    bad("stored NLEN wrong", stored_block(rb(20), nlen=0xFFFF ^ 21), 20, E_STORED_LEN)
    bad("stored NLEN equal to LEN", stored_block(rb(20), nlen=20), 20, E_STORED_LEN)
    bad("stored block cut inside its bytes", stored_block(rb(20)).bytes()[:-1], 20, E_INPUT)
    bad("stored block cut inside NLEN", stored_block(rb(20)).bytes()[:4], 20, E_INPUT)

    # ---- matches
    for ls in range(257, 286):
        for extra in sorted({0, (1 << LEN_EXTRA[ls - 257]) - 1}):
            toks = [97, 98, 99, ("sym", ls, extra, 2, 0)]
            ok("length symbol %d extra %d" % (ls, extra), fixed_block(toks), model(toks))
    for ds in range(26):
        dist = min(DIST_BASE[ds] + (1 << DIST_EXTRA[ds]) - 1, TILE - 3)
        front = rb(dist)
        toks = [("sym", 257, 0, ds, dist - DIST_BASE[ds])]
        ok("distance symbol %d, distance %d" % (ds, dist), fixed_block(toks, b=stored_block(front, final=False)), front + model(toks, front))
        toks = [("sym", 257, 0, ds, 0)]
        front = rb(DIST_BASE[ds])
        ok("distance symbol %d extra 0" % ds, fixed_block(toks, b=stored_block(front, final=False)), front + model(toks, front))
    front = rb(TILE - 3)
    for ds in range(26, 30):
        bad("distance symbol %d reaches before the start" % ds, fixed_block([("sym", 257, 0, ds, 0)], b=stored_block(front, final=False)), TILE, E_DISTANCE)
    for ds in (30, 31):
        bad("distance symbol %d in a fixed block" % ds, pad(fixed_block([97, 98, 99, ("sym", 257, 0, ds, 0)])), 6, E_SYMBOL)
    front = rb(17)
    for dist in (1, 2, 3, 7, 8, 9, 15, 16, 17):
        for length in (3, 7, 8, 9, 16, 17, 258):
            toks = list(front) + [(length, dist), 0x21]
            ok("distance %d length %d" % (dist, length), fixed_block(toks), model(toks))
    toks = list(front) + [(30, 17)]
    ok("distance equal to the bytes written", fixed_block(toks), model(toks))
    bad("distance one more than the bytes written", pad(fixed_block(list(front) + [(30, 18)])), 47, E_DISTANCE)
    bad("a match as the first symbol", pad(fixed_block([(3, 1)])), 3, E_DISTANCE)
    toks = [1, 2, 3, 4, 5, 6, 7, 8, 9, (100, 9)]
    ok("a match that ends at the end of the tile", fixed_block(toks), model(toks))
    bad("a match that passes the end of the tile by one", pad(fixed_block(toks)), 108, E_OUTPUT)
    full = rb(TILE - 258)
    ok("a match that ends at byte 8192", fixed_block([(258, 300)], b=stored_block(full, final=False)), full + model([(258, 300)], full))
    bad("a match that would end at byte 8193", pad(fixed_block([7, (258, 300)], b=stored_block(full, final=False))), TILE, E_OUTPUT)
    bad("a literal at the end of the tile", pad(fixed_block([65, 66, 67, 68])), 3, E_OUTPUT)
    bad("a literal behind a full tile", pad(fixed_block([65], b=stored_block(body, final=False))), TILE, E_OUTPUT)
    for s in (286, 287):
        bad("length symbol %d through the fixed codes" % s, pad(fixed_block([97, 98, 99, ("sym", s, 0, None, 0)])), 3, E_SYMBOL)

    # ---- dynamic headers
    lits = list(range(65, 79))                                     # 14 literals at lengths 1..14, end-of-block and length 3 at 15 bits; 16 distance codes likewise
    ll = lens_of(258, dict(list(zip(lits, range(1, 15))) + [(256, 15), (257, 15)]))
    dl = list(range(1, 15)) + [15, 15]
    toks = lits * 14 + [(3, DIST_BASE[i]) for i in range(16)] + [78]
    ok("codes of 1 to 15 bits, literals and distances", dyn_block(toks, ll, dl), model(toks))
    bad("a 15-bit distance code that reaches before the start", pad(dyn_block(lits + [("sym", 257, 0, 15, 5)], ll, dl)), 17, E_DISTANCE)
    ll4 = lens_of(257, {97: 1, 98: 2, 99: 3, 256: 3})
    cl7 = lens_of(19, {18: 1, 0: 2, 1: 3, 2: 4, 17: 5, 16: 6, 3: 7, 4: 7})
    toks = [97, 98, 99, 99, 98, 97]
    ok("a code-length code with codes of 7 bits", dyn_block(toks, ll4, [1, 1], cl_lens=cl7), model(toks))
    ll286 = [9] * 256 + [6] * 28 + [5] * 2
    dl30 = [5] * 28 + [4] * 2
    toks = list(rb(50)) + [(258, 50), (3, 1), ("sym", 284, 31, 0, 0)]
    ok("HLIT 29 and HDIST 29", dyn_block(toks, ll286, dl30), model(toks))
    for n in (287, 288):
        bad("HLIT %d" % (n - 257), pad(dyn_block([], [8] * n, [5] * 30, ops=[], eob=False), 40), 0, E_CODE)
    cl_rep = lens_of(19, {0: 2, 1: 3, 2: 3, 16: 3, 17: 3, 18: 3, 3: 4, 4: 4})

    def zeros(n):                                                  # n lengths of zero as repeat symbols
        out = []
        while n > 138:
            out.append((18, 127))
            n -= 138
        return out + ([(18, n - 11)] if n >= 11 else [(17, n - 3)] if n >= 3 else [(0,)] * n)
    assert sum(2.0 ** -l for l in cl_rep if l) == 1.0
    bad("repeat 16 as the first code-length symbol", pad(dyn_block([], ll4, [1, 1], cl_lens=cl_rep, ops=[(16, 0)], eob=False), 40), 0, E_CODE)
    # lengths: 97 -> 2, 98 -> 2, 256 -> 2, 257 -> 2, then four distance codes of 2 bits: "2, repeat 16 x 4" runs from symbol 257 into the distance lengths
    ll_r = lens_of(258, {97: 2, 98: 2, 256: 2, 257: 2})
    ops16 = zeros(97) + [(2,), (2,)] + zeros(256 - 99) + [(2,), (2,), (16, 1)]
    toks = [97, 98, 98, 97, (3, 4), (3, 1), (3, 2), (3, 3)]
    ok("repeat 16 across the literal / distance boundary, filling the last length exactly", dyn_block(toks, ll_r, [2, 2, 2, 2], cl_lens=cl_rep, ops=ops16), model(toks))
    bad("repeat 16 one past the last length", pad(dyn_block([], ll_r, [2, 2, 2, 2], cl_lens=cl_rep, ops=ops16[:-1] + [(16, 2)], eob=False), 40), 0, E_CODE)
    # 7 unused length symbols and 4 unused distance symbols as ONE repeat 18 of 11 zeros
    ll_z = lens_of(265, {97: 1, 256: 2, 257: 2})
    dl_z = [0, 0, 0, 0, 1, 1]
    ops18 = zeros(97) + [(1,)] + zeros(256 - 98) + [(2,), (2,), (18, 0), (1,), (1,)]
    toks = [97] * 8 + [(3, 5), (3, 8)]
    ok("repeat 18 across the literal / distance boundary", dyn_block(toks, ll_z, dl_z, cl_lens=cl_rep, ops=ops18), model(toks))
    bad("repeat 18 one past the last length", pad(dyn_block([], ll_z, dl_z, cl_lens=cl_rep, ops=ops18[:-3] + [(18, 3)], eob=False), 40), 0, E_CODE)
    bad("repeat 17 past the last length", pad(dyn_block([], ll_z, dl_z, cl_lens=cl_rep, ops=ops18[:-1] + [(17, 0)], eob=False), 40), 0, E_CODE)
    toks = [97, 98, 98, 97]
    ok("no distance code at all", dyn_block(toks, ll4, [0]), model(toks))
    bad("a match without a distance code", pad(dyn_block([97, ("sym", 257, 0, None, 0)], lens_of(258, {97: 1, 256: 2, 257: 2}), [0], eob=False)), 4, E_SYMBOL)
    ll_m = lens_of(258, {97: 1, 256: 2, 257: 2})
    toks = [97, (3, 1), 97]
    ok("a single distance code of one bit, used", dyn_block(toks, ll_m, [1]), model(toks))
    bad("the unused half of a single distance code", pad(dyn_block([97, ("sym", 257, 0, None, 0), ("raw", 1, 1)], ll_m, [1], eob=False)), 4, E_SYMBOL)
    ok("a single literal / length code of one bit (end-of-block only)", dyn_block([], lens_of(257, {256: 1}), [0]), b"")
    bad("the unused half of a single literal / length code", pad(dyn_block([("raw", 1, 1)], lens_of(257, {256: 1}), [0], eob=False)), 0, E_SYMBOL)
    hdr = lambda ll, dl, **kw: pad(dyn_block([], ll, dl, eob=False, **kw), 40)
    bad("over-subscribed code-length code", hdr(ll4, [1, 1], cl_lens=lens_of(19, {0: 1, 1: 1, 2: 1}), ops=[]), 0, E_CODE)
    bad("incomplete code-length code", hdr(ll4, [1, 1], cl_lens=lens_of(19, {0: 1, 1: 2}), ops=[]), 0, E_CODE)
    bad("a single code-length code of one bit", hdr(ll4, [1, 1], cl_lens=lens_of(19, {0: 1}), ops=[]), 0, E_CODE)
    bad("over-subscribed literal / length code", hdr(lens_of(257, {97: 1, 98: 1, 256: 1}), [1, 1]), 0, E_CODE)
    bad("incomplete literal / length code", hdr(lens_of(257, {97: 2, 256: 2}), [1, 1]), 0, E_CODE)
    bad("over-subscribed distance code", hdr(ll4, [1, 1, 1]), 0, E_CODE)
    bad("incomplete distance code", hdr(ll4, [2, 2]), 0, E_CODE)
    bad("no end-of-block code", hdr(lens_of(257, {97: 1, 98: 1}), [1, 1]), 0, E_NO_EOB)
    # the strictness cases: one code of TWO bits is not the incomplete code RFC 1951 permits (zlib refuses it)
    bad("a single literal / length code of two bits", pad(dyn_block([], lens_of(257, {256: 2}), [0]), 40), 0, E_CODE)
    bad("a single distance code of two bits", pad(dyn_block([97], ll_m, [2]), 40), 1, E_CODE)

    # ---- block sequences in one tile
    data = rb(600)
    b = Bits()
    for i, x in enumerate(data):
        fixed_block([x], final=i == 599, b=b)
    ok("600 fixed blocks of one literal each", b, data)
    p1, p2, p3, p4 = rb(30), rb(70), [97, 98, 99, 99, 98, 97], [1, 2, (9, 100)]
    b = fixed_block(list(p1), final=False)
    stored_block(p2, final=False, b=b)
    dyn_block(p3, ll4, [1, 1], final=False, b=b, cl_lens=cl7)
    fixed_block(p4, b=b)
    whole = p1 + p2 + model(p3, p1 + p2)
    ok("fixed, stored, dynamic, fixed in one stream", b, whole + model(p4, whole))
    b = Bits()
    for _ in range(3):
        fixed_block([], final=False, b=b)
        stored_block(b"", final=False, b=b)
        dyn_block([], ll4, [1, 1], final=False, b=b)
    ok("empty blocks of every kind in front of the data", fixed_block(list(b"data"), b=b), b"data")
    b = fixed_block(list(b"data"), final=False)
    dyn_block([], ll4, [1, 1], final=False, b=b)
    ok("empty blocks of every kind behind the data", stored_block(b"", b=fixed_block([], final=False, b=b)), b"data")
    bad("the reserved block type", pad(Bits().put(1, 1).put(3, 2)), 0, E_BLOCK_TYPE)
    bad("the reserved block type behind a block", pad(fixed_block([65], final=False).put(0, 1).put(3, 2)), 1, E_BLOCK_TYPE)
    bad("no final block", fixed_block(list(b"data"), final=False), 4, E_INPUT)
    bad("fewer bytes than the tile's size", fixed_block(list(b"data")), 5, E_SIZE)
    bad("an empty stream for an empty tile", b"", 0, E_INPUT)
    return C


def payload(r, kind, n):
    if kind == 0:
        return bytes(r.randrange(256) for _ in range(n))
    if kind == 1:
        return bytes(r.choice(b"ACGT") for _ in range(n))
    if kind == 2:                                                  # runs
        out = bytearray()
        while len(out) < n:
            out += bytes([r.choice(b"abc")]) * r.randrange(1, 40)
        return bytes(out[:n])
    if kind == 3:
        return bytes(n)
    if kind == 4:                                                  # a geometric alphabet
        return bytes(min(int(r.expovariate(0.7)), 255) for _ in range(n))
    return vcf_like(n, r.randrange(1 << 30))


def zlib_grid(count=300, seed=8192):
    """[(stream, payload)]: zlib-made raw streams of 0..8192 bytes - levels 0 / 1 / 6 / 9, every strategy, memLevel 1..9, and flushes
    of every kind every 1..3000 bytes"""
    r = random.Random(seed)
    sizes = list(range(41)) + [TILE - 1, TILE]
    out = []
    for i in range(count):
        n = sizes[i] if i < len(sizes) else r.randrange(41, TILE + 1)
        data = payload(r, i % 6, n)
        co = zlib.compressobj(r.choice((0, 1, 6, 9)), zlib.DEFLATED, -15, r.randrange(1, 10),
                              r.choice((zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED)))
        if r.randrange(3) == 0 and n > 1:
            step, how = r.randrange(1, 3001), r.choice((zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, zlib.Z_PARTIAL_FLUSH, zlib.Z_BLOCK))
            z = b"".join(co.compress(data[a:a + step]) + co.flush(how) for a in range(0, n, step)) + co.flush()
        else:
            z = co.compress(data) + co.flush()
        out.append((z, data))
    return out


def mutations(grid, count=4000, nbases=200, seed=4000):
    """[(stream, want, kind, the payload of the unchanged stream)]: seeded mutations of the first `nbases` streams of the grid that have at least 8 bytes of payload;
    kind 'flip' = one bit flipped, 'byte' = one byte replaced, 'cut' = truncated"""
    r = random.Random(seed)
    bases = [(z, d) for z, d in grid if len(d) >= 8][:nbases]
    out = []
    for k in range(count):
        z, d = bases[k % len(bases)]
        s = bytearray(z)
        kind = ("flip", "flip", "flip", "byte", "cut")[k % 5]
        if kind == "cut":
            s = s[:r.randrange(len(s))]
        else:
            at = r.randrange(len(s)) if k % 3 else r.randrange(min(len(s), 40))      # (a third of them in the first block's header)
            if kind == "flip":
                s[at] ^= 1 << r.randrange(8)
            else:
                s[at] = (s[at] + 1 + r.randrange(255)) & 0xFF
        out.append((bytes(s), len(d), kind, d))
    return out


def write_case_file(path, cases):
    """the cases as the stand-alone program tile_inflate_fuzz reads them"""
    with open(path, "wb") as f:
        f.write(b"TILECASE" + struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<III", len(c.stream), c.want, c.expect) + c.stream)
