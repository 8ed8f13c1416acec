#!/usr/bin/env python3
"""Binary cells + vid mapping -> the lines of a CSV cell file (the reference loader's CSV input, CSV2TileDBBinary).

An independent printer for the tests of the device importer's CSV path: it walks the cell layout of vcf2cells.py / vcf_importer.h
    [row i64][col i64][cell_size u64][END i64][REF][ALT][QUAL f32][FILTER][INFO attributes][FORMAT attributes]
and prints one line per cell, tokens separated by ',' in that order: a fixed-length attribute as its elements, a variable-length
numeric attribute as its count and its elements, REF / ALT / a variable-length char attribute as one token.  Floats are printed
with %.9g (which names every float uniquely), a TileDB null (int 0x7fffffff, float bits 0x7f7fffff, END 2^63-1) as an empty token.

    cells2csv.py <cells.bin> <vid.json> > out.csv
"""
import os
import random
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vcf2cells  # noqa: E402

NULL_INT, NULL_FLOAT_BITS, NULL_INT64 = 0x7FFFFFFF, 0x7F7FFFFF, 2**63 - 1


def attributes(vid_path):
    """-> [(name, kind 'int'|'float'|'str', fixed length or None)] for QUAL.. in schema order; refuses what CSV lines cannot carry"""
    fields, _ = vcf2cells.load_vid(vid_path)
    names, info, fmt = vcf2cells.schema_attributes(fields)
    if "ID" in names:
        raise NotImplementedError("a vid that declares ID has no CSV form")
    out = []
    for f in info + fmt:
        if f.ndim != 1 or f.tuple_idx is not None or f.kind not in ("int", "float", "str") or (f.kind == "str" and f.fixed):
            raise NotImplementedError("field %s has no CSV form" % f.name)
        out.append((f.name, f.kind, f.length if f.fixed else None))
    return out


def _int(v):
    return "" if v == NULL_INT else str(v)


def _float(bits):
    return "" if bits == NULL_FLOAT_BITS else "%.9g" % struct.unpack("<f", struct.pack("<I", bits))[0]


def cells_to_lines(cells, vid_path):
    attrs = attributes(vid_path)
    lines, at = [], 0
    while at < len(cells):
        row, col, size = struct.unpack_from("<qqQ", cells, at)
        p = at + 24
        (end,) = struct.unpack_from("<q", cells, p)
        p += 8
        tok = [str(row), str(col), "" if end == NULL_INT64 else str(end)]
        for _ in range(2):      # REF, ALT
            (n,) = struct.unpack_from("<i", cells, p)
            tok.append(cells[p + 4:p + 4 + n].decode("latin-1"))
            p += 4 + n
        tok.append(_float(struct.unpack_from("<I", cells, p)[0]))
        p += 4
        for name, kind, fixed in [("FILTER", "int", None)] + attrs:
            if kind == "str":
                (n,) = struct.unpack_from("<i", cells, p)
                tok.append(cells[p + 4:p + 4 + n].decode("latin-1"))
                p += 4 + n
                continue
            n = fixed
            if n is None:
                (n,) = struct.unpack_from("<i", cells, p)
                p += 4
                tok.append(str(n))
            for _ in range(n):
                tok.append(_int(struct.unpack_from("<i", cells, p)[0]) if kind == "int" else _float(struct.unpack_from("<I", cells, p)[0]))
                p += 4
        if p != at + size:
            raise ValueError("cell at byte %d: walked %d bytes, cell_size is %d" % (at, p - at, size))
        for t in tok:
            if "," in t or '"' in t or "\n" in t:
                raise ValueError("cell at byte %d: a token with a separator or a quote has no CSV form" % at)
        lines.append(",".join(tok))
        at += size
    return lines


def csv_text(cells, vid_path, seed=None):
    """the CSV file of the cells; seed: shuffle the lines, keeping the order of lines with equal (column, row)"""
    lines = cells_to_lines(cells, vid_path)
    if seed is not None:
        keyed = {}
        for ln in lines:
            r, c = ln.split(",", 2)[:2]
            keyed.setdefault((c, r), []).append(ln)
        groups = list(keyed.values())
        random.Random(seed).shuffle(groups)
        lines = [ln for g in groups for ln in g]
    return "".join(ln + "\n" for ln in lines)


if __name__ == "__main__":
    sys.stdout.write(csv_text(open(sys.argv[1], "rb").read(), sys.argv[2]))
