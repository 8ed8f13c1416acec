"""Reader and writer of the columnar fragment file (versions 2 and 3; format: csrc/kernels/gdb_pipeline.hip, 'columnar fragment
file') for the tests: parse() cuts a file into its sections, write_v3() writes a version-3 file from the raw bytes of the sections
with a tile writer of the caller's choice, so that a test decides what DEFLATE stream every 8 KiB tile is.

Layout, little endian: "GDBAMDF2", u32 version, u32 nfields, i64 ncells, i64 nmarkers, i32 num_rows, i32 pad, six 8-byte meta
fields (88 bytes); per field u8 var, u8 elem_size, u16 name_len, i32 fixed_num, u64 data_bytes, name; version 3 only: u64 stored
bytes of every column section (row, begin, end, then offsets and data per field); then, each 64-byte aligned: row[], begin[],
end[], marker_begin[] (never compressed), per field off[] (variable-length fields only) and data[].  A version-3 column section is
[tile streams][u64 tile offset x (ntiles + 1)][u64 ntiles]."""
import struct
import zlib

TILE = 8192


class Field:
    def __init__(self, var, elem_size, fixed_num, data_bytes, name, header):
        self.var, self.elem_size, self.fixed_num, self.data_bytes, self.name, self.header = var, elem_size, fixed_num, data_bytes, name, header


class Section:
    """name: "row" / "begin" / "end" / "markers" / "<field> offsets" / "<field> data"; nbytes: its size as inflated; stored_index: its
    slot in the version-3 table of stored sizes (None: the markers); at: file offset of its first byte; tiles: the DEFLATE stream
    of every tile as found in the file (None: the section is raw in the file), tile_offs: their offsets from `at`"""
    def __init__(self, name, nbytes, stored_index, field=None):
        self.name, self.nbytes, self.stored_index, self.field = name, nbytes, stored_index, field
        self.at, self.tiles, self.tile_offs, self._raw = None, None, None, None

    @property
    def ntiles(self):
        return (self.nbytes + TILE - 1) // TILE

    @property
    def raw(self):
        """the section's bytes as they lie in device memory (tiles inflated with zlib)"""
        if self._raw is None:
            self._raw = b"".join(zlib.decompressobj(-15).decompress(z) for z in self.tiles)
            assert len(self._raw) == self.nbytes
        return self._raw


class Fragment:
    def __init__(self):
        self.version = self.C = self.M = self.nfields = None
        self.head = None            # the 88 header bytes
        self.fields = []
        self.sections = []
        self.first_section_at = None

    def section(self, name):
        return [s for s in self.sections if s.name == name][0]


def _align(x):
    return (x + 63) & ~63


def parse(blob):
    blob = bytes(blob)
    f = Fragment()
    assert blob[:8] == b"GDBAMDF2"
    f.version, f.nfields, f.C, f.M = struct.unpack_from("<IIqq", blob, 8)
    assert f.version in (2, 3)
    f.head = blob[:88]
    at = 88
    for _ in range(f.nfields):
        var, es, name_len, fixed_num, data_bytes = struct.unpack_from("<BBHiQ", blob, at)
        f.fields.append(Field(var, es, fixed_num, data_bytes, blob[at + 16:at + 16 + name_len].decode(), blob[at:at + 16 + name_len]))
        at += 16 + name_len
    nsec = 3 + 2 * f.nfields
    stored = None
    if f.version == 3:
        stored = struct.unpack_from("<%dQ" % nsec, blob, at)
        at += 8 * nsec
    f.sections = [Section("row", f.C * 4, 0), Section("begin", f.C * 8, 1), Section("end", f.C * 8, 2), Section("markers", f.M * 8, None)]
    for i, fd in enumerate(f.fields):
        if fd.var:
            f.sections.append(Section(fd.name + " offsets", (f.C + 1) * 4, 3 + 2 * i, fd))
        f.sections.append(Section(fd.name + " data", fd.data_bytes, 4 + 2 * i, fd))
    for s in f.sections:
        at = _align(at)
        if f.first_section_at is None:
            f.first_section_at = at
        s.at = at
        if f.version == 2 or s.stored_index is None:
            s._raw = blob[at:at + s.nbytes]
            assert len(s._raw) == s.nbytes
            at += s.nbytes
            continue
        st = stored[s.stored_index]
        nt = struct.unpack_from("<Q", blob, at + st - 8)[0]
        assert nt == s.ntiles
        s.tile_offs = struct.unpack_from("<%dQ" % (nt + 1), blob, at + st - 8 - 8 * (nt + 1))
        assert s.tile_offs[0] == 0 and s.tile_offs[nt] + 8 * (nt + 1) + 8 == st
        s.tiles = [blob[at + s.tile_offs[i]:at + s.tile_offs[i + 1]] for i in range(nt)]
        at += st
    assert at == len(blob)
    return f


def write_v3(frag, tile_writer):
    """a version-3 file of the fragment's sections; tile_writer(raw tile bytes, section, tile index) -> the tile's raw DEFLATE
    stream.  The tile index of every section is written from the streams' real sizes, so whatever the writer returns (a stream cut
    short, say) is exactly what the reader hands to the inflater for that tile."""
    out = bytearray(frag.head)
    struct.pack_into("<I", out, 8, 3)
    for fd in frag.fields:
        out += fd.header
    nsec = 3 + 2 * frag.nfields
    stored_pos = len(out)
    out += bytes(8 * nsec)
    stored = [0] * nsec
    for s in frag.sections:
        out += bytes((64 - len(out) % 64) % 64)
        raw = s.raw
        if s.stored_index is None:
            out += raw
            continue
        offs = [0]
        for i in range(s.ntiles):
            z = bytes(tile_writer(raw[i * TILE:(i + 1) * TILE], s, i))
            out += z
            offs.append(offs[-1] + len(z))
        out += struct.pack("<%dQ" % (s.ntiles + 1), *offs) + struct.pack("<Q", s.ntiles)
        stored[s.stored_index] = offs[-1] + 8 * (s.ntiles + 1) + 8
    struct.pack_into("<%dQ" % nsec, out, stored_pos, *stored)
    return bytes(out)
