"""Shared by the incremental-import tests: begin-cell streams taken apart and put together in Python - the yardstick the
bounded imports and the device merge (genomicsdb_amd.merge_cells) are held against - and crafted opaque streams."""
import random
import struct

HEADER = struct.Struct("<qqQ")      # row, column, cell_size


def split_cells(data):
    """[(row, col, cell bytes)] of a stream, by its size chain"""
    out = []
    at = 0
    while at < len(data):
        row, col, size = HEADER.unpack_from(data, at)
        assert size >= HEADER.size and at + size <= len(data)
        out.append((row, col, data[at:at + size]))
        at += size
    return out


def rows_between(data, lo, hi):
    """the cells of `data` whose row lies in [lo, hi], in their order"""
    return b"".join(c for r, _, c in split_cells(data) if lo <= r <= hi)


def sorted_merge(streams):
    """the streams' cells in (column, row) order; Python's sort is stable, so equal keys keep stream order, then in-stream order"""
    cells = [c for s in streams for c in split_cells(s)]
    return b"".join(c for _, _, c in sorted(cells, key=lambda c: (c[1], c[0])))


def cell(row, col, payload):
    return HEADER.pack(row, col, HEADER.size + len(payload)) + payload


def crafted_stream(rng, n, rows, col_range, sizes=(0, 1, 15, 16, 17, 63, 64, 65)):
    """n cells with rows drawn from `rows`, columns below col_range and seeded random payloads, sorted by (column, row)"""
    keys = sorted(((rng.randrange(col_range), rng.choice(rows)) for _ in range(n)))
    return b"".join(cell(r, c, rng.randbytes(rng.choice(sizes))) for c, r in keys)


def rng(seed):
    return random.Random(seed)
