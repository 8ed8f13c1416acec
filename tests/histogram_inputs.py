"""Inputs shared by the input histogram's tests (test_histogram_bodies_cpu.py, test_histogram_device.py): the fixture callset
mappings that list only VCF files, and a hand-made generator whose sequence of bins holds the run lengths at which the aggregation
inside a wavefront can go wrong.  What a histogram must be always comes from tests/tools/histogram_model.py."""
import glob
import gzip
import json
import os
import sys

import helpers

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bgzf_write  # noqa: E402
import histogram_model  # noqa: E402

INPUTS = os.path.join(helpers.GOLDEN, "inputs")
VID = os.path.join(INPUTS, "vid.json")
CONTIG2 = 249250621          # column offset of contig "2" in vid.json
LAST_COLUMN = 3101976561     # the last column of vid.json's last contig (NC_007605: offset 3101804739, length 171823)


def fixture_mappings():
    """-> [file name] of the mappings under tests/golden/inputs/callsets that list only VCF files which exist"""
    out = []
    for path in sorted(glob.glob(os.path.join(INPUTS, "callsets", "*.json"))):
        doc = json.load(open(path))
        if "callsets" not in doc or any(k.endswith("csv_files") and doc[k] for k in doc):
            continue
        entries = histogram_model.callset_entries(path)
        if entries and all(e.get("filename") and os.path.exists(os.path.join(helpers.GOLDEN, e["filename"])) for e in entries):
            out.append(os.path.basename(path))
    return out


def fixture(name):
    """-> (vid, callsets, file root)"""
    return VID, os.path.join(INPUTS, "callsets", name), helpers.GOLDEN


# ---- the generator: bins of 1000 columns; per run (contig, bin within the contig, records)
GEN_BIN = 1000
GEN_RUNS = [("1", 0, 1), ("1", 1, 63), ("1", 2, 64), ("1", 3, 65), ("1", 4, 300), ("1", 5, 1), ("1", 7, 2), ("2", 0, 100), ("2", 1, 107)]
GEN_NUM_BINS = (CONTIG2 + 2 * GEN_BIN) // GEN_BIN + 1
GEN_RANGE = GEN_NUM_BINS * GEN_BIN - 1       # size_of_bin = (GEN_RANGE + 1 + GEN_NUM_BINS - 1) // GEN_NUM_BINS = GEN_BIN
GEN_HEADER = ["##fileformat=VCFv4.2", "##contig=<ID=1,length=249250621>", "##contig=<ID=2,length=243199373>",
              "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tGA\tGB"]
GEN_ENCODINGS = ("plain", "gzip", "bgzf")


def gen_lines():
    """the record lines: within contig c, the j-th record of the run in bin k begins at column offset(c) + first + j, where first is
    the first column of the contig that falls into the bin"""
    lines = []
    for contig, k, n in GEN_RUNS:
        off = 0 if contig == "1" else CONTIG2
        first_bin = off // GEN_BIN + k
        first_col = max(first_bin * GEN_BIN, off)
        for j in range(n):
            pos = first_col + j - off + 1
            lines.append("\t".join([contig, str(pos), ".", "ACGT"[j % 4], "<NON_REF>", ".", ".", "END=%d" % (pos + 5), "GT:DP", "0/0:%d" % (j % 50), "0/0:7"]))
    return lines


def gen_text():
    return ("\n".join(GEN_HEADER + gen_lines()) + "\n").encode()


def write_generated(dirname):
    """-> {encoding: (vid, callsets, file root)}: the same text as plain, gzip and BGZF (members of 4000 bytes), two callsets each"""
    os.makedirs(dirname, exist_ok=True)
    text = gen_text()
    names = {"plain": "hist_gen.vcf", "gzip": "hist_gen.vcf.gz", "bgzf": "hist_gen_bgzf.vcf.gz"}
    with open(os.path.join(dirname, names["plain"]), "wb") as f:
        f.write(text)
    with gzip.open(os.path.join(dirname, names["gzip"]), "wb") as f:
        f.write(text)
    bgzf_write.write_file(os.path.join(dirname, names["bgzf"]), text, member_size=4000)
    out = {}
    for enc, fn in names.items():
        cp = os.path.join(dirname, "callsets_%s.json" % enc)
        with open(cp, "w") as f:
            json.dump({"callsets": {"GA": {"row_idx": 0, "idx_in_file": 0, "filename": fn}, "GB": {"row_idx": 1, "idx_in_file": 1, "filename": fn}}}, f)
        out[enc] = (VID, cp, dirname)
    return out


def write_one_line(dirname, contig, pos, name="edge.vcf"):
    """a one-sample file with two records in front and one record at contig:pos -> (vid, callsets, root, path, 1-based line of that record)"""
    os.makedirs(dirname, exist_ok=True)
    rec = lambda c, p: "\t".join([c, str(p), ".", "A", "<NON_REF>", ".", ".", "END=%d" % p, "GT:DP", "0/0:3"])      # noqa: E731
    lines = GEN_HEADER[:3] + ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tEA", rec("1", 1), rec("1", 2), rec(contig, pos)]
    path = os.path.join(dirname, name)
    with open(path, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode())
    cp = os.path.join(dirname, name + ".callsets.json")
    with open(cp, "w") as f:
        json.dump({"callsets": {"EA": {"row_idx": 0, "idx_in_file": 0, "filename": name}}}, f)
    return VID, cp, dirname, path, len(lines)
