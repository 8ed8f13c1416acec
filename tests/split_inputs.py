"""Inputs shared by the splitter's tests (test_split_bodies_cpu.py, test_split_device.py): the three input sets, the hand-made file,
a walker of BGZF members.  What a split must give always comes from tests/tools/split_model.py."""
import json
import os
import struct
import sys

import helpers

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import split_model  # noqa: E402

INPUTS = os.path.join(helpers.GOLDEN, "inputs")
VID = os.path.join(INPUTS, "vid.json")
LAST_END = 2 ** 63 - 2
CONTIG2 = 249250621          # column offset of contig "2" in vid.json

# the hand-made partitions: [0, 999] [1000, 1999] [2000, 9999] [10000, contig 2 - 1] (no record) [contig 2, ..]
HAND_BEGINS = [0, 1000, 2000, 10000, CONTIG2]
_FMT = "GT:DP:GQ:MIN_DP:PL"


def _rec(chrom, pos, ref, alt, info, samples=("0/0:3:9:3:0,9,90", "0/0:5:12:4:0,12,120")):
    return "\t".join([chrom, str(pos), ".", ref, alt, ".", ".", info, _FMT] + list(samples))


HAND_LINES = [
    "##fileformat=VCFv4.2",
    "##contig=<ID=1,length=249250621>",
    "##contig=<ID=2,length=243199373>",
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tHA\tHB",
    _rec("2", 100, "A", "<NON_REF>", "END=200"),                      # contig 2 in front of contig 1: partition 4
    _rec("1", 500, "C", "<NON_REF>", "END=2500"),                     # spans all three partitions
    _rec("1", 901, "G", "<NON_REF>", "END=1000"),                     # tend 999 = begin_1 - 1: out of partition 1
    _rec("1", 950, "T", "<NON_REF>", "END=1001"),                     # tend 1000 = begin_1: in
    _rec("1", 995, "ACGTACGT", "A,<NON_REF>", "."),                   # no END: col 994, tend 994 + 8 - 1 = 1001, by the length of REF
    _rec("1", 1100, "A", "<NON_REF>", "DP=3;END=1500"),               # END is not the first key
    _rec("1", 1600, "C", "<NON_REF>", "END=1700;DP=2;END=2500"),      # END twice: the last one counts, so partitions 1 and 2
    _rec("1", 1800, "G", "T,<NON_REF>", "DP=7") + "\r",               # a CRLF line
    _rec("1", 2000, "T", "<NON_REF>", "END=2000"),                    # col 1999 = end_1: in partition 1
    _rec("1", 2001, "A", "<NON_REF>", "END=2100"),                    # col 2000 = end_1 + 1: out of partition 1
    _rec("1", 3000, "C", "G,<NON_REF>", "DP=11"),                     # the last line, without a newline
]


def hand_text():
    return ("\n".join(HAND_LINES)).encode()


def write_hand(dirname, text=None):
    """-> (vid, callsets, file root, [file names]) of the hand-made two-sample file in dirname"""
    os.makedirs(dirname, exist_ok=True)
    with open(os.path.join(dirname, "hand_split.vcf"), "wb") as f:
        f.write(hand_text() if text is None else text)
    cs = {"callsets": {"HA": {"row_idx": 0, "idx_in_file": 0, "filename": "hand_split.vcf"}, "HB": {"row_idx": 1, "idx_in_file": 1, "filename": "hand_split.vcf"}}}
    cp = os.path.join(dirname, "hand_split_callsets.json")
    with open(cp, "w") as f:
        json.dump(cs, f)
    return VID, cp, dirname, ["hand_split.vcf"]


def golden_set(callsets):
    cp = os.path.join(INPUTS, "callsets", callsets)
    names = []
    for v in json.load(open(cp))["callsets"].values():
        if v["filename"] not in names:
            names.append(v["filename"])
    return VID, cp, helpers.GOLDEN, names


def input_sets(tmpdir):
    """-> {set name: (vid, callsets, file root, [file names], [partition begins])}"""
    return {"a": golden_set("t0_1_2.json") + ([0, 12200, 17385],),
            "b": golden_set("t6_7_8.json") + ([0, 8029500, 8029501],),
            "c": write_hand(os.path.join(str(tmpdir), "hand")) + (HAND_BEGINS,)}


def model_of(vid, root, names, begins):
    """-> ({(name, p): bytes}, [(begin, end)])"""
    parts = split_model.derive_partitions(begins, LAST_END)
    offsets = split_model.contig_offsets(vid)
    out = {}
    for name in names:
        for p, text in enumerate(split_model.split_file(os.path.join(root, name), offsets, parts)):
            out[(name, p)] = text
    return out, parts


def is_header_only(text):
    return all(line.startswith(b"#") for line in text.splitlines())


def assert_model_is_interesting(model, names, n_parts):
    """some (file, partition) is header-only, and some line lands in two or more partitions"""
    assert any(is_header_only(t) for t in model.values())
    shared = False
    for name in names:
        seen = {}
        for p in range(n_parts):
            for line in model[(name, p)].splitlines():
                if not line.startswith(b"#"):
                    seen[line] = seen.get(line, 0) + 1
        shared = shared or any(n >= 2 for n in seen.values())
    assert shared


def bgzf_members(buf):
    """-> [(offset, size)] of a buffer that is BGZF from its first byte to its last and ends with the 28-byte EOF block; asserts both"""
    out, at = [], 0
    while at < len(buf):
        assert buf[at:at + 4] == b"\x1f\x8b\x08\x04", at
        xlen = struct.unpack_from("<H", buf, at + 10)[0]
        assert buf[at + 12:at + 14] == b"BC" and struct.unpack_from("<H", buf, at + 14)[0] == 2 and xlen == 6, at
        size = struct.unpack_from("<H", buf, at + 16)[0] + 1
        assert at + size <= len(buf), at
        out.append((at, size))
        at += size
    assert at == len(buf) and out and out[-1][1] == 28
    assert buf[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    return out


def contigs_in(text):
    names = []
    for line in text.splitlines():
        if line and not line.startswith(b"#"):
            c = line.split(b"\t")[0].decode()
            if c not in names:
                names.append(c)
    return names
