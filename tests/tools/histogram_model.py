"""Model of vcf_histogram ("Histogram of the input files") in plain Python: how many records of the input files of a
callset mapping begin in each bin of a uniform histogram over the columns.  It shares nothing with the code under test: files are
read with gzip / open, lines are split with bytes.split, numbers are parsed with int().

The rule: column = contig offset + POS - 1 of a record line (a line that is neither empty nor a '#' line).  The record counts iff
column_begin <= column <= column_end, and it counts once per callset of its file whose row lies in [lb, ub] (the weight); a file
without such a callset is not read.  UniformHistogram(0, max_histogram_range, num_bins) of the reference:
    size_of_bin = (max_histogram_range - 0 + 1 + (num_bins - 1)) // num_bins,   bin = column // size_of_bin
A counted column above max_histogram_range raises HistogramRange(path, 1-based physical line)."""
import gzip
import json

LAST = 2 ** 63 - 2


class HistogramRange(Exception):
    def __init__(self, path, line, column):
        Exception.__init__(self, "%s line %d: column %d" % (path, line, column))
        self.path, self.line, self.column = path, line, column


def contig_offsets(vid_path):
    contigs = json.load(open(vid_path))["contigs"]
    if isinstance(contigs, dict):
        return {k: int(v["tiledb_column_offset"]) for k, v in contigs.items()}
    return {c["name"]: int(c["tiledb_column_offset"]) for c in contigs}


def read_text(path):
    with open(path, "rb") as f:
        magic = f.read(2)
    if magic == b"\x1f\x8b":
        with gzip.open(path, "rb") as f:
            return f.read()
    with open(path, "rb") as f:
        return f.read()


def callset_entries(callsets_path):
    c = json.load(open(callsets_path))["callsets"]
    return list(c.values()) if isinstance(c, dict) else list(c)


def weights(callsets_path, lb=0, ub=LAST):
    """-> [(filename, weight)] in mapping order: the files with a callset whose row lies in the bounds, which are clamped as the
    loader clamps them (negative -> 0, swapped when reversed)"""
    lb, ub = max(lb, 0), max(ub, 0)
    if ub < lb:
        lb, ub = ub, lb
    out = {}
    for e in callset_entries(callsets_path):
        if lb <= int(e["row_idx"]) <= ub:
            out[e["filename"]] = out.get(e["filename"], 0) + 1
    return list(out.items())


def record_columns(text, offsets):
    """-> [(1-based physical line, column)] of the record lines, in file order"""
    out = []
    pieces = text.split(b"\n")
    if pieces and pieces[-1] == b"":
        pieces.pop()
    for i, body in enumerate(pieces):
        if body.endswith(b"\r"):
            body = body[:-1]
        if not body or body.startswith(b"#"):
            continue
        cols = body.split(b"\t")
        out.append((i + 1, offsets[cols[0].decode()] + int(cols[1]) - 1))
    return out


def size_of_bin(max_histogram_range, num_bins):
    return (max_histogram_range + 1 + (num_bins - 1)) // num_bins


def bin_sequence(text, offsets, max_histogram_range, num_bins, column_begin=0, column_end=LAST, path="<text>"):
    """-> per record line, in file order: its bin, or None when the record lies outside the column bounds"""
    size = size_of_bin(max_histogram_range, num_bins)
    seq = []
    for line, col in record_columns(text, offsets):
        if col < column_begin or col > column_end:
            seq.append(None)
            continue
        if col > max_histogram_range:
            raise HistogramRange(path, line, col)
        seq.append(col // size)
    return seq


def histogram(vid_path, callsets_path, root, max_histogram_range, num_bins, column_begin=0, column_end=LAST, lb=0, ub=LAST, info=None):
    """-> [count per bin]; info, a dict, receives files / records (record lines seen) / counted (those inside the column bounds)"""
    import os
    offsets = contig_offsets(vid_path)
    counts = [0] * num_bins
    files = records = counted = 0
    for name, weight in weights(callsets_path, lb, ub):
        path = name if os.path.isabs(name) or not root else os.path.join(root, name)
        files += 1
        for b in bin_sequence(read_text(path), offsets, max_histogram_range, num_bins, column_begin, column_end, path):
            records += 1
            if b is not None:
                counted += 1
                counts[b] += weight
    if info is not None:
        info.update({"files": files, "records": records, "counted": counted})
    return counts


def text(counts, max_histogram_range):
    """Histogram::print of the reference"""
    size = size_of_bin(max_histogram_range, len(counts))
    out = "Histogram: [\n"
    for b, n in enumerate(counts):
        if n:
            out += "%d,%d,%d\n" % (b * size, (b + 1) * size - 1, n)
    return out + "]\n"


def runs(seq):
    """-> [(first index, length, value)] of the runs of equal values of a sequence"""
    out = []
    for i, v in enumerate(seq):
        if out and out[-1][2] == v:
            out[-1] = (out[-1][0], out[-1][1] + 1, v)
        else:
            out.append((i, 1, v))
    return out
