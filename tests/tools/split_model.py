"""Model of vcf2tiledb --split-files ("Splitting input files by column partition") in plain Python: which lines of a (g)VCF
text file go to which column partition.  It shares nothing with the code under test: files are read with gzip / open, lines are
split with bytes.split, numbers are parsed with int().

The rule: partition p = [begin_p, end_p].  A '#' line goes to every partition, an empty line to none, a record line - verbatim, in
file order, '\\r' kept - to every partition that its interval [col, tend] overlaps:
    col  = contig offset + POS - 1
    tend = contig offset + END - 1 when INFO carries END (the last END counts), else col + len(REF) - 1
A last line without a newline gets one."""
import gzip
import json


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


def derive_partitions(begins, last_end=2 ** 63 - 2):
    """[(begin, end)] in the order given, ends derived from the sorted begins like the loader JSON's column_partitions"""
    order = sorted(begins)
    return [(b, order[order.index(b) + 1] - 1 if order.index(b) + 1 < len(order) else last_end) for b in begins]


def lines_of(text):
    """-> the physical lines, each with its newline (the last one gets one)"""
    pieces = text.split(b"\n")
    if pieces and pieces[-1] == b"":
        pieces.pop()
    return [p + b"\n" for p in pieces]


def interval(raw, offsets):
    body = raw[:-1]
    if body.endswith(b"\r"):
        body = body[:-1]
    cols = body.split(b"\t")
    off = offsets[cols[0].decode()]
    col = off + int(cols[1]) - 1
    tend = col + len(cols[3]) - 1
    if cols[7] != b".":
        for kv in cols[7].split(b";"):
            if kv.split(b"=")[0] == b"END":
                tend = off + int(kv.split(b"=", 1)[1]) - 1
    return col, tend


def classify(text, offsets):
    """-> [(raw, None | (col, tend))]: the lines of the output in file order, None for a '#' line"""
    out = []
    for raw in lines_of(text):
        body = raw[:-1]
        if body.endswith(b"\r"):
            body = body[:-1]
        if not body:
            continue
        out.append((raw, None if body.startswith(b"#") else interval(raw, offsets)))
    return out


def overlaps(iv, part):
    return iv[0] <= part[1] and iv[1] >= part[0]


def split_text(text, offsets, partitions):
    """-> [bytes per partition]"""
    lines = classify(text, offsets)
    return [b"".join(raw for raw, iv in lines if iv is None or overlaps(iv, part)) for part in partitions]


def split_file(path, offsets, partitions):
    return split_text(read_text(path), offsets, partitions)


def round_trip_precondition(text, offsets, part):
    """Among the record lines with col < begin, none that misses the partition has a col >= that of one that overlaps it: then the
    importer's partition-begin rule sees the same latest record in the split file as in the original."""
    before = [iv for _, iv in classify(text, offsets) if iv is not None and iv[0] < part[0]]
    inside = [iv[0] for iv in before if overlaps(iv, part)]
    return not inside or all(iv[0] < min(inside) for iv in before if not overlaps(iv, part))


def replay_differs(text, offsets, part):
    """The sharper statement for one file: the importer replays, per row, the latest record at or before the partition begin if
    it reaches the begin.  The split file differs from the original exactly when the original's latest record misses the partition
    (nothing is replayed) while the split file still holds an earlier one that reaches it (which then is)."""
    ivs = [iv for _, iv in classify(text, offsets) if iv is not None and iv[0] <= part[0]]
    if not ivs:
        return False
    best = None
    for iv in ivs:                      # the largest col; of equals the later line
        if best is None or iv[0] >= best[0]:
            best = iv
    return not overlaps(best, part) and any(overlaps(iv, part) and iv[0] < part[0] for iv in ivs)
