"""Shared by the streaming-import tests (CPU harness and device): a callset mapping of VCF files -> per stream its header bytes and
its records, as text lines and as BCF2 records, cut into writes; the same writes as the input of tests/tools/stream_import_model.py
(columns from the text, END and size of every cell from the HOST importer's cells of the same records); and the caller's loop that
the model assumes, run against anything with the StreamImporter interface.  Not a test module."""
import gzip
import json
import os
import struct
import sys

import helpers

sys.path.insert(0, os.path.join(helpers.ROOT, "tests", "tools"))
import stream_import_model as model  # noqa: E402
import vcf2bcf  # noqa: E402

INPUTS = os.path.join(helpers.GOLDEN, "inputs")


def read_text(path):
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def split_text(text):
    """VCF text -> (header through the #CHROM line, [record line with its newline])"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    k = max(i for i, l in enumerate(lines) if l.startswith(b"#")) + 1
    return b"".join(l + b"\n" for l in lines[:k]), [l + b"\n" for l in lines[k:] if l]


def split_bcf(data):
    """plain BCF2 stream -> (header: 9 + l_text bytes, [record])"""
    l_text = struct.unpack_from("<I", data, 5)[0]
    at, recs = 9 + l_text, []
    while at < len(data):
        l_shared, l_indiv = struct.unpack_from("<II", data, at)
        recs.append(data[at:at + 8 + l_shared + l_indiv])
        at += 8 + l_shared + l_indiv
    return data[:9 + l_text], recs


def contig_offsets(vid_path):
    c = json.load(open(vid_path))["contigs"]
    items = c.items() if isinstance(c, dict) else [(x["name"], x) for x in c]
    return {k: v["tiledb_column_offset"] for k, v in items}


def column_of(line, offsets):
    chrom, pos = line.split(b"\t", 2)[:2]
    return offsets[chrom.decode()] + int(pos) - 1


def parse_cells(cells):
    """begin-cells -> [(row, column, size, END)]"""
    out, at = [], 0
    while at < len(cells):
        row, col, size, end = struct.unpack_from("<qqQq", cells, at)
        out.append((row, col, size, end))
        at += size
    assert at == len(cells)
    return out


class Streams:
    """the sources of a callset mapping as buffer streams.  sources: [(stream name, VCF text)] in mapping order; rows_of: name -> rows in
    sample order of the callsets that use it; host_cells: the host importer's cells of the same records over the whole column range"""

    def __init__(self, vid_path, sources, rows_of, host_cells, bcf=False):
        self.names = [n for n, _ in sources]
        self.bcf = bcf
        offsets = contig_offsets(vid_path)
        vid = json.load(open(vid_path))
        self.headers, self.records, self.columns, self.cells = [], [], [], []
        # (row, column) -> its cells in the host importer's order: equal keys come from one stream, in record order
        by_key = {}
        for row, col, size, end in parse_cells(host_cells):
            by_key.setdefault((row, col), []).append((end, size))
        for name, text in sources:
            head, lines = split_text(text)
            cols = [column_of(l, offsets) for l in lines]
            if bcf:
                head, recs = split_bcf(vcf2bcf.encode(text, vid=vid)[0])
                assert len(recs) == len(lines)
            else:
                recs = lines
            self.headers.append(head)
            self.records.append(recs)
            self.columns.append(cols)
            per_record = []
            for col in cols:
                one = []
                for row in rows_of.get(name, []):
                    end, size = by_key[(row, col)].pop(0)
                    one.append((row, end, size))
                per_record.append(one)
            self.cells.append(per_record)
        self.used = [bool(rows_of.get(n)) for n in self.names]

    def writes(self, capacity):
        """per stream the list of writes: [[record index]]; whole records up to `capacity` bytes per write, a larger record goes alone"""
        out = []
        for s, recs in enumerate(self.records):
            room = capacity[s] if isinstance(capacity, (list, tuple)) else capacity      # (one capacity per stream, or one for all)
            ws, cur, n = [], [], 0
            for i, r in enumerate(recs):
                if cur and n + len(r) > room:
                    ws.append(cur)
                    cur, n = [], 0
                cur.append(i)
                n += len(r)
            if cur:
                ws.append(cur)
            out.append(ws)
        return out

    def model_input(self, writes):
        return [[[(self.columns[s][i], self.cells[s][i]) for i in w] for w in ws] if self.used[s] else None for s, ws in enumerate(writes)]

    def bytes_of(self, s, write):
        return b"".join(self.records[s][i] for i in write)


MAX_COLUMN = 2**63 - 2


def mapping_sources(callsets_path, files=None, root=helpers.GOLDEN):
    """a callset mapping -> ([(source name, VCF text)] in order of first appearance, {source name: rows in sample order}); a source is a
    "filename" or a "stream_name"; files: {stream name: file} where the names are not the files themselves"""
    cs = json.load(open(callsets_path))["callsets"]
    entries = list(cs.values()) if isinstance(cs, dict) else cs
    names = []
    for e in entries:
        n = e.get("filename", e.get("stream_name"))
        if n not in names:
            names.append(n)
    rows_of = {n: [r for _, r in sorted((e.get("idx_in_file", 0), e["row_idx"]) for e in entries if e.get("filename", e.get("stream_name")) == n)] for n in names}
    sources = []
    for n in names:
        f = (files or {}).get(n, n)
        sources.append((n, read_text(f if os.path.isabs(f) else os.path.join(root, f))))
    return sources, rows_of


def host_reference(gdb, vid_path, sources, rows_of, tmpdir, bcf, treat=True):
    """-> f(column_begin, column_end): the HOST importer's cells of the sources as files.  For BCF2 streams the files hold the text that
    the independent decoder tests/tools/bcf2text.py makes of the encoded records (floats as %.9g), as tests/test_import_bcf_device.py does"""
    os.makedirs(tmpdir, exist_ok=True)
    vid = json.load(open(vid_path))
    callsets = {}
    for k, (name, text) in enumerate(sources):
        if bcf:
            text = helpers.bcf_stream_to_text(vcf2bcf.encode(text, vid=vid)[0])
        with open(os.path.join(tmpdir, "src%d.vcf" % k), "wb") as f:
            f.write(text)
        for i, row in enumerate(rows_of.get(name, [])):
            callsets["cs%d" % row] = {"row_idx": row, "idx_in_file": i, "filename": "src%d.vcf" % k}
    c = os.path.join(tmpdir, "files.json")
    with open(c, "w") as f:
        json.dump({"callsets": callsets}, f)
    cache = {}

    def cells(column_begin=0, column_end=MAX_COLUMN):
        key = (column_begin, column_end)
        if key not in cache:
            cache[key] = gdb.import_cells(vid_path, c, file_root=tmpdir, treat_deletions_as_intervals=treat, column_begin=column_begin, column_end=column_end)[0]
        return cache[key]
    return cells


def loader_json(vid_path, callsets_path=None, column_begin=0, column_end=None, treat=True, **more):
    parts = [{"begin": column_begin, "workspace": more.pop("workspace", "/nonexistent"), "array": "arr"}]
    if column_end is not None:
        parts.append({"begin": column_end + 1, "workspace": parts[0]["workspace"], "array": "arr_next"})
    d = {"row_based_partitioning": False, "column_partitions": parts, "vid_mapping_file": vid_path, "treat_deletions_as_intervals": treat,
         "produce_tiledb_array": False, "produce_combined_vcf": False}
    if callsets_path:
        d["callset_mapping_file"] = callsets_path
    d.update(more)
    return d


def run_streams(imp_factory, S, capacity, column_begin=0, column_end=MAX_COLUMN, callsets_json="", host=None, end_with_empty_write=True):
    """the whole check of one case: batches against the model, the concatenation against the host importer, the pending figures against
    the model and its bound -> (batches, stats)"""
    writes = S.writes(capacity)
    expected = model.run(S.model_input(writes), column_begin, column_end)
    imp = imp_factory()
    try:
        for k, (name, head) in enumerate(zip(S.names, S.headers)):
            imp.add_buffer_stream(name, S.bcf, capacity[k] if isinstance(capacity, (list, tuple)) else capacity, head)
        file_idx = imp.setup(callsets_json)
        assert [i >= 0 for i in file_idx] == S.used
        assert imp.max_identifiers == sum(S.used)
        batches = drive(imp, S, writes, end_with_empty_write)
        st = imp.stats()
        imp.finish()
    finally:
        imp.close()
    check_against_model(batches, expected)
    if host is not None:
        assert b"".join(c for c, _ in batches) == host(column_begin, column_end)
    bound_cells, bound_bytes = model.pending_bound(S.model_input(writes), column_begin, column_end)
    want_cells, want_bytes = max(b["pending_cells"] for b in expected), max(b["pending_bytes"] for b in expected)
    print("pending cells %d (model %d, bound %d), bytes %d (model %d, bound %d), batches %d" %
          (st["max_pending_cells"], want_cells, bound_cells, st["max_pending_bytes"], want_bytes, bound_bytes, len(batches)))
    assert st["max_pending_cells"] == want_cells <= bound_cells
    assert st["max_pending_bytes"] == want_bytes <= bound_bytes
    assert st["num_batches"] == len(expected) and st["num_cells"] == sum(len(b["cells"]) for b in expected)
    assert st["num_spanning_cells"] == sum(b["spanning"] for b in expected)
    return batches, st


def drive(imp, streams, writes, end_with_empty_write=True):
    """the caller's loop of the model: the first write of every used stream, then after every batch the next write of every reported
    stream (none, or an empty one, when it has no more) -> [(cells, exhausted)]"""
    nxt = [0] * len(writes)
    out = []

    def refill(s):
        if nxt[s] < len(writes[s]):
            imp.write(s, streams.bytes_of(s, writes[s][nxt[s]]))
        elif end_with_empty_write and s % 2 == 0:
            imp.write(s, b"")
        nxt[s] += 1

    for s in range(len(writes)):
        if streams.used[s]:
            refill(s)
    for _ in range(100000):
        cells, exhausted = imp.import_batch()
        out.append((cells, exhausted))
        if imp.done:
            return out
        assert exhausted, "a batch that is not the last reports at least one stream"
        for s, part in exhausted:
            assert part == 0
            refill(s)
    raise AssertionError("the import does not end")


def check_against_model(batches, expected):
    """device batches [(cells, exhausted)] against the model's"""
    assert len(batches) == len(expected)
    for k, ((cells, exhausted), want) in enumerate(zip(batches, expected)):
        got = [(col, row, size) for row, col, size, _ in parse_cells(cells)]
        assert got == want["cells"], "batch %d" % k
        assert [s for s, _ in exhausted] == want["exhausted"], "batch %d" % k


def fixture_case(gdb, tmpdir, callsets, vid="vid.json", files=None, bcf=False, treat=True, extra_unused=None):
    """a fixture callset mapping as buffer streams -> (Streams, host reference, vid path, callsets path); extra_unused: the name of one
    more stream, with the first source's text, that no callset uses"""
    v, c = os.path.join(INPUTS, vid), os.path.join(INPUTS, "callsets", callsets)
    sources, rows_of = mapping_sources(c, files)
    host = host_reference(gdb, v, sources, rows_of, str(tmpdir), bcf, treat)
    if extra_unused:
        sources = sources + [(extra_unused, sources[0][1])]
    return Streams(v, sources, rows_of, host(), bcf), host, v, c


def buffer_files():
    """t0_1_2_buffer_mapping.json: stream name -> file of the fixture tree"""
    return json.load(open(os.path.join(INPUTS, "callsets", "t0_1_2_buffer_mapping.json")))


SYNTH_HEADER = (b"##fileformat=VCFv4.1\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n##ALT=<ID=NON_REF,Description=\"any\">\n"
                b"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"depth\">\n"
                b"##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"quality\">\n##FORMAT=<ID=MIN_DP,Number=1,Type=Integer,Description=\"min depth\">\n"
                b"##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"likelihoods\">\n##INFO=<ID=END,Number=1,Type=Integer,Description=\"end\">\n"
                b"##contig=<ID=1,length=249250621>\n")


def synthetic_sources(seed=20240611, dense=300, sparse=12, span=60000):
    """two seeded single-sample gVCF streams over the same columns of contig 1: `dense` records against `sparse` records; every 7th record
    of the dense stream is followed by a second record at the same POS (a block and a site), so that with small writes such a pair
    falls on either side of a write boundary -> ([(name, text)], {name: [row]})"""
    import random
    rng = random.Random(seed)
    out = []
    for k, n in enumerate((dense, sparse)):
        pos = sorted(rng.sample(range(1000, 1000 + span), n))
        lines = [SYNTH_HEADER + b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS%d\n" % k]
        for i, p in enumerate(pos):
            end = min(p + rng.randrange(1, 40), (pos[i + 1] - 1) if i + 1 < n else p + 5)
            dp = rng.randrange(1, 90)
            lines.append(b"1\t%d\t.\t%s\t<NON_REF>\t.\t.\tEND=%d\tGT:DP:GQ:MIN_DP:PL\t0/0:%d:%d:%d:0,%d,%d\n" %
                         (p, rng.choice([b"A", b"C", b"G", b"T"]), max(end, p), dp, rng.randrange(0, 99), max(dp - 3, 0), rng.randrange(1, 60), rng.randrange(60, 900)))
            if k == 0 and i % 7 == 3:
                lines.append(b"1\t%d\t.\tG\tA,<NON_REF>\t%d.5\tPASS\t.\tGT:DP:GQ:PL\t0/1:%d:%d:%d,0,%d,%d,%d,%d\n" %
                             (p, rng.randrange(30, 900), dp, rng.randrange(0, 99), rng.randrange(1, 900), rng.randrange(1, 900), rng.randrange(1, 900),
                              rng.randrange(1, 900), rng.randrange(1, 900)))
        out.append(("synth_stream_%d" % k, b"".join(lines)))
    return out, {"synth_stream_0": [0], "synth_stream_1": [1]}


def stream_callsets(rows_of):
    """a callset mapping that names every source by its stream name"""
    return {"callsets": {"cs%d" % r: {"row_idx": r, "idx_in_file": i, "stream_name": n} for n, rows in rows_of.items() for i, r in enumerate(rows)}}


def hostsim_case_text(S, writes, column_begin, column_end):
    """the model's input as tests/hostsim_import_stream reads it"""
    max_row = max([r for cells in S.cells for rec in cells for r, _, _ in rec] or [0])
    bits = 1
    while max_row >> bits:
        bits += 1
    out = ["%d %d %d %d %d" % (bits, max_row, column_begin, column_end, len(writes))]
    for s, ws in enumerate(writes):
        out.append("%d %d" % (1 if S.used[s] else 0, len(ws) if S.used[s] else 0))
        for w in ws if S.used[s] else []:
            out.append("%d" % len(w))
            for i in w:
                out.append("%d %d " % (S.columns[s][i], len(S.cells[s][i])) + " ".join("%d %d %d" % c for c in S.cells[s][i]))
    return "\n".join(out) + "\n"


def hostsim_report(batches):
    """the model's batches as tests/hostsim_import_stream prints them"""
    lines = []
    for b in batches:
        w = "inf" if b["W"] == model.POS_INF else "-inf" if b["W"] == model.NEG_INF else "%d" % b["W"]
        lines.append("W %s |%s |%s | %d %d" % (w, "".join(" %d %d %d" % c for c in b["cells"]), "".join(" %d" % s for s in b["exhausted"]), b["pending_cells"], b["pending_bytes"]))
    return "\n".join(lines) + "\n"
