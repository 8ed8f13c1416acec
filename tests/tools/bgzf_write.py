"""BGZF written with Python's zlib (raw streams, wbits=-15): the test inputs of the device inflater.

member(payload, ...) is one gzip member with the "BC" subfield; bgzf(data, ...) cuts `data` into members of `member_size`
payload bytes and always ends with the EOF member.  level 0 gives stored blocks; fixed=True gives fixed-Huffman blocks
(Z_FIXED); flush_at puts a Z_FULL_FLUSH into each member behind that many payload bytes (several DEFLATE blocks in one
member); empty_member_at inserts an empty member in front of the member of that index.
"""
import struct
import zlib

EOF = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0])
MAX_MEMBER = 65536


def raw_deflate(payload, level=6, fixed=False, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, zlib.Z_FIXED if fixed else zlib.Z_DEFAULT_STRATEGY)
    if flush_at is not None and 0 < flush_at < len(payload):
        return c.compress(payload[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(payload[flush_at:]) + c.flush()
    return c.compress(payload) + c.flush()


def wrap(stream, payload=None, crc=None, isize=None):
    """a BGZF member around a raw DEFLATE stream; crc / isize override the trailer (for malformed inputs)"""
    total = 18 + len(stream) + 8
    if total > MAX_MEMBER:
        raise ValueError("member of %d bytes: BSIZE holds at most %d" % (total, MAX_MEMBER))
    crc = zlib.crc32(payload) if crc is None else crc
    isize = len(payload) if isize is None else isize
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", total - 1) + stream
            + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF))


def member(payload, level=6, fixed=False, flush_at=None):
    payload = bytes(payload)
    return wrap(raw_deflate(payload, level, fixed, flush_at), payload)


def bgzf(data, member_size=65280, level=6, fixed=False, flush_at=None, empty_member_at=None):
    data = bytes(data)
    out = []
    for k, at in enumerate(range(0, len(data), member_size)):
        if empty_member_at == k:
            out.append(member(b"", level))
        out.append(member(data[at:at + member_size], level, fixed, flush_at))
    out.append(EOF)
    return b"".join(out)


def split_members(buf):
    """[(offset, raw stream, crc, isize)] of a BGZF buffer (the test's own walk over the headers)"""
    out = []
    at = 0
    while at < len(buf):
        assert buf[at:at + 4] == b"\x1f\x8b\x08\x04" and buf[at + 12:at + 16] == b"BC\x02\x00", "not BGZF at %d" % at
        xlen, = struct.unpack_from("<H", buf, at + 10)
        bsize = struct.unpack_from("<H", buf, at + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", buf, at + bsize - 8)
        out.append((at, buf[at + 12 + xlen:at + bsize - 8], crc, isize))
        at += bsize
    return out


def write_file(path, data, **kw):
    with open(path, "wb") as f:
        f.write(bgzf(data, **kw))
