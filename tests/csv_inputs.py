"""Inputs and known answers shared by the CPU and the GPU tests of the device importer's CSV path (test_import_csv_bodies_cpu.py,
test_import_csv_device.py).  Nothing here comes from the code under test: CSV text is printed by tests/tools/cells2csv.py from the
host TEXT importer's cells, the hand fixture's cells are written out with struct.pack, and every error case names the words and the
line the format's rules give it."""
import json
import os
import struct
import sys

import helpers
from golden_cases import CASES

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import cells2csv  # noqa: E402

INPUTS = os.path.join(helpers.GOLDEN, "inputs")
COLUMN_END = 2**63 - 2


def paths(callsets, vid):
    return os.path.join(INPUTS, vid), os.path.join(INPUTS, "callsets", callsets)


def _fields(vid):
    fields = json.load(open(os.path.join(INPUTS, vid)))["fields"]
    return fields if isinstance(fields, dict) else {f.get("name", f.get("field_name")): f for f in fields}


def is_2d(vid):
    return any(isinstance(f.get("length"), list) or isinstance(f.get("type"), list) for f in _fields(vid).values())


def declares_id(vid):
    return "ID" in _fields(vid)


ALL_PAIRS = sorted({(c[1], c[2]) for c in CASES if not is_2d(c[2])})
PAIRS = [p for p in ALL_PAIRS if not declares_id(p[1])]
ID_PAIRS = [p for p in ALL_PAIRS if declares_id(p[1])]


def csv_mapping(callsets_json, directory, name="cells.csv", rows=None, key="unsorted_csv_files"):
    """a copy of the mapping whose callsets (those of `rows`, default all) read the CSV file `name`; -> path of the new mapping"""
    m = json.load(open(callsets_json))
    cs = m["callsets"]
    for c in (cs.values() if isinstance(cs, dict) else cs):
        if rows is None or c["row_idx"] in rows:
            c["filename"] = name
    m[key] = [name]
    os.makedirs(directory, exist_ok=True)
    out = os.path.join(directory, "callsets_csv.json")
    with open(out, "w") as f:
        json.dump(m, f)
    return out


def split_cells(cells):
    out, at = [], 0
    while at < len(cells):
        size = struct.unpack_from("<Q", cells, at + 16)[0]
        out.append(cells[at:at + size])
        at += size
    return out


def after_csv(cells, vid_path):
    """the cells a CSV reader makes of the %.9g text of `cells`: the same bytes, except that a float element that is a NaN (the
    importer's 'missing inside a vector', bits 0x7f800001) is printed as "nan" and read back by strtof as the default quiet NaN
    0x7fc00000 - no decimal text names a NaN's payload.  -> (expected bytes, number of such elements)"""
    out = bytearray(cells)
    attrs = cells2csv.attributes(vid_path)
    at, nans = 0, 0
    while at < len(cells):
        size = struct.unpack_from("<Q", cells, at + 16)[0]
        p = at + 32
        for _ in range(2):
            p += 4 + struct.unpack_from("<i", cells, p)[0]
        p += 4
        for _, kind, fixed in [("FILTER", "int", None)] + attrs:
            n = fixed
            if n is None:
                n = struct.unpack_from("<i", cells, p)[0]
                p += 4
            if kind == "str":
                p += n
                continue
            for _ in range(n):
                if kind == "float":
                    (x,) = struct.unpack_from("<f", cells, p)
                    if x != x:
                        out[p:p + 4] = struct.pack("<I", 0x7FC00000)
                        nans += 1
                p += 4
        assert p == at + size
        at += size
    return bytes(out), nans


# ---- the hand fixture inputs/callsets/csv_hand.csv (vid_csv_hand.json: INFO DP int, MQ float, AF float A, NM char; FORMAT GT, PL, SB int x 4)
HAND = ("csv_hand.json", "vid_csv_hand.json")
HAND_PARTITION = (100, 5000)        # line 1 (column 50) lies in front of it, line 7 (column 6000) behind it
HAND_RECORDS = 6                    # non-empty lines: 8 physical lines, lines 3 and 6 are empty ("" and "\r")
NULL_I, NULL_F, NULL_I64 = 0x7FFFFFFF, 0x7F7FFFFF, 2**63 - 1
# tokens outside the device's fast path, counted by hand: line 2 "1e30" "0x1f"; line 5 " 7" " 5"; line 8 "+1" "010" "12abc"
HAND_DEFERRED = 7


def _cell(row, col, body):
    return struct.pack("<qqQ", row, col, 24 + len(body)) + body


def _s(b):
    return struct.pack("<i", len(b)) + b


def _f(x):
    return struct.pack("<f", x)


def _i(*v):
    return struct.pack("<%di" % len(v), *v)


def hand_cells(begin=0, end=COLUMN_END):
    """the cells of csv_hand.csv in (column, row) order, lines with equal (column, row) in file order"""
    nf, ni = struct.pack("<I", NULL_F), _i(NULL_I)
    line1 = _cell(0, 50, struct.pack("<q", 400) + _s(b"A") + _s(b"&") + nf + _i(0) + ni + nf + _i(0) + _s(b"") + _i(0) + _i(0) + _i(1, 2, 3, 4))
    line2 = _cell(2, 300, struct.pack("<q", 310) + _s(b"AT") + _s(b"A|&") + _f(50.5) + _i(1, 0) + _i(12) + _f(60.0) + _i(3) + _f(0.25) + _f(1e-3) + _f(1e30) + _s(b"abc")
                  + _i(2, 0, 1) + _i(3, 0, 30, 31) + _i(1, 2, 3, 4))
    line5 = _cell(2, 300, struct.pack("<q", 300) + _s(b"AT") + _s(b"&") + _f(7.0) + _i(0) + _i(5) + _f(-0.5) + _i(1) + _f(5.0) + _s(b"z") + _i(1, 0) + _i(0) + ni * 4)
    line7 = _cell(2, 6000, struct.pack("<q", 6000) + _s(b"A") + _s(b"&") + nf + _i(0) + ni + nf + _i(0) + _s(b"") + _i(0) + _i(0) + _i(1, 2, 3, 4))
    line8 = _cell(0, 200, struct.pack("<q", NULL_I64) + _s(b"G") + _s(b"&") + nf + _i(0) + ni + nf + _i(0) + _s(b"") + _i(2, -1, 1) + _i(1, 8) + _i(-7, 12, 5) + ni)
    ordered = [(50, line1), (200, line8), (300, line2), (300, line5), (6000, line7)]
    kept = [c for col, c in ordered if begin <= col <= end]
    return b"".join(kept), len(kept)


# ---- errors: (id, lines of a.csv over vid_csv_hand.json with rows 0 and 2, words of the message, line number) ----------------------
GOOD = "0,100,100,A,&,,0,,,0,,0,0,1,2,3,4"
LINE_ERRORS = [
    ("quote", [GOOD, '0,101,101,A,&,,0,,,0,"x",0,0,1,2,3,4', '0,102,"'], r"a '\"' in a CSV line", 2),
    ("quote_in_a_skipped_row", [GOOD, '1,101,101,"A"'], r"a '\"' in a CSV line", 2),
    ("row", [GOOD, GOOD, "x,100,100,A,&"], "row, column or END of a CSV line cannot be parsed", 3),
    ("row_of_no_callset_is_still_parsed", ["*,100"], "row, column or END of a CSV line cannot be parsed", 1),
    ("column", [GOOD, "0,,100,A,&"], "row, column or END of a CSV line cannot be parsed", 2),
    ("column_missing", [GOOD, "", "0"], "row, column or END of a CSV line cannot be parsed", 3),
    ("end", [GOOD, "0,100,e,A,&,,0,,,0,,0,0,1,2,3,4"], "row, column or END of a CSV line cannot be parsed", 2),
    ("count_null", [GOOD, "0,100,100,A,&,,*,,,0,,0,0,1,2,3,4"], "a count token of a CSV line is null, negative", 2),
    ("count_empty", [GOOD, "0,100,100,A,&,,0,,,,,0,0,1,2,3,4"], "a count token of a CSV line is null, negative", 2),
    ("count_negative", [GOOD, "0,100,100,A,&,,0,,,-1,,0,0,1,2,3,4"], "a count token of a CSV line is null, negative", 2),
    ("count_past_the_line", ["", GOOD, "0,100,100,A,&,,0,,,0,,0,9,1,2,3,4"], "a count token of a CSV line is null, negative", 3),
    ("left_over", [GOOD, GOOD + ",5"], "tokens left over after the last attribute", 2),
    ("left_over_empty", [GOOD + ","], "tokens left over after the last attribute", 1),
    ("open", [GOOD, "0,100,100,A,&,,0,,,0,,0,0,1,2"], "a CSV line ends before its last attribute", 2),
    ("open_after_alt", [GOOD, "2,100,100,A"], "a CSV line ends before its last attribute", 2),
    ("value_int", [GOOD, "0,100,100,A,&,,0,x7,,0,,0,0,1,2,3,4"], r"field DP: cannot convert 'x7' to an integer", 2),
    ("value_float", [GOOD, "0,100,100,A,&,,0,,.,0,,0,0,1,2,3,4"], r"field MQ: cannot convert '\.' to a float", 2),
    ("the_smaller_line_speaks", [GOOD, "0,100,100,A,&,,0,,,0,,0,0,1,2", "x,1"], "a CSV line ends before its last attribute", 2),
]


def write_case(directory, lines, vid_fields=None, name="a.csv", raw=None):
    """-> (vid, callsets, root): a.csv with the lines, rows 0 and 2 mapped to it"""
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, name), "wb") as f:
        f.write(raw if raw is not None else "".join(ln + "\n" for ln in lines).encode())
    vid = json.load(open(os.path.join(INPUTS, "vid_csv_hand.json")))
    if vid_fields:
        vid["fields"].update(vid_fields)
    with open(os.path.join(directory, "vid.json"), "w") as f:
        json.dump(vid, f)
    with open(os.path.join(directory, "callsets.json"), "w") as f:
        json.dump({"callsets": {"A": {"row_idx": 0, "idx_in_file": 0, "filename": name}, "B": {"row_idx": 2, "idx_in_file": 0, "filename": name}},
                   "sorted_csv_files": [name]}, f)
    return os.path.join(directory, "vid.json"), os.path.join(directory, "callsets.json"), directory


# refused by name before any line is read: (id, extra vid fields, words)
VID_REFUSALS = [
    ("id", {"ID": {"type": "char", "length": "VAR"}}, "field ID: a vid that declares ID is not imported from CSV cell files"),
    ("fixed_char", {"TAG": {"vcf_field_class": ["FORMAT"], "type": "char", "length": 3}}, "field TAG: fixed-length char attributes are not imported from CSV cell files"),
    ("flag", {"DB": {"vcf_field_class": ["INFO"], "type": "flag"}}, "field DB: only int, float and char attributes are imported from CSV cell files"),
    ("two_dimensional", {"AS_X": {"vcf_field_class": ["INFO"], "type": "float", "length": ["R", "var"], "vcf_delimiter": ["|", ","]}},
     "field AS_X: .*not imported by the device importer"),
]
