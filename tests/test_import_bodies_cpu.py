"""The bodies of the device importer (csrc/core/gdb_import.hpp) on the CPU, through the harness tests/hostsim_import (measure,
scan, write, deferred tokens, partition-begin rule, sort, gather as plain loops around the same functions): the cells must be
the host importer's (csrc/host/vcf_importer.cc) byte for byte, and the number fast paths must give the bits of strtoll /
(float)strtod wherever they accept - and accept everything they promise to.  Host code only - no device."""
import ctypes
import json
import os
import random
import re
import struct

import pytest

import helpers
from golden_cases import CASES

INPUTS = os.path.join(helpers.GOLDEN, "inputs")


def _is_2d(vid):
    fields = json.load(open(os.path.join(INPUTS, vid)))["fields"]
    fields = fields.values() if isinstance(fields, dict) else fields        # (vid_as_array.json lists its fields)
    return any(isinstance(f.get("length"), list) or isinstance(f.get("type"), list) for f in fields)


PAIRS = sorted({(c[1], c[2]) for c in CASES if not _is_2d(c[2])})
PAIRS_2D = sorted({(c[1], c[2]) for c in CASES if _is_2d(c[2])})
HAND = ("import_hand.json", "vid_import_hand.json")
HAND_DEFERRED = 8       # QUAL 1234.5678901234567, MQ=1e-30, FS=nan (x 2 samples) and QUAL Inf (x 2 samples)


@pytest.fixture(scope="module")
def gdb():
    from genomicsdb_amd import build as b
    b.build_native()
    import genomicsdb_amd
    return genomicsdb_amd


@pytest.fixture(scope="module")
def sim():
    from genomicsdb_amd import build as b
    L = ctypes.CDLL(b.build_hostsim_import())
    c = ctypes
    L.hsi_last_error.restype = c.c_char_p
    L.hsi_import.argtypes = [c.c_char_p, c.c_char_p, c.c_char_p, c.c_int, c.c_int64, c.c_int64, c.POINTER(c.c_void_p), c.POINTER(c.c_uint64), c.POINTER(c.c_int64)]
    L.hsi_free.argtypes = [c.c_void_p]
    L.hsi_check_floats.argtypes = [c.c_char_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    L.hsi_check_ints.argtypes = [c.c_char_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    return L


def _paths(callsets, vid):
    return os.path.join(INPUTS, vid), os.path.join(INPUTS, "callsets", callsets)


def sim_import(L, vid, callsets, treat=True, begin=0, end=2**63 - 2, root=None):
    """-> (bytes, {files, records, cells, spanning, deferred}); raises RuntimeError with the harness's message"""
    p, n = ctypes.c_void_p(), ctypes.c_uint64()
    st = (ctypes.c_int64 * 5)()
    rc = L.hsi_import(os.fsencode(vid), os.fsencode(callsets), os.fsencode(root or helpers.GOLDEN), 1 if treat else 0, begin, end, ctypes.byref(p), ctypes.byref(n), st)
    if rc != 0:
        raise RuntimeError(L.hsi_last_error().decode())
    try:
        return ctypes.string_at(p.value, n.value), dict(zip(("files", "records", "cells", "spanning", "deferred"), st))
    finally:
        L.hsi_free(p)


@pytest.mark.parametrize("treat", [True, False], ids=["deletions_as_intervals", "deletions_as_points"])
@pytest.mark.parametrize("callsets,vid", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_bodies_match_host_importer_on_fixtures(gdb, sim, callsets, vid, treat):
    v, c = _paths(callsets, vid)
    want, ncells = gdb.import_cells(v, c, file_root=helpers.GOLDEN, treat_deletions_as_intervals=treat, device=None)
    got, st = sim_import(sim, v, c, treat)
    assert ncells > 0 and st["cells"] == ncells
    assert got == want
    if treat:
        assert got == helpers.cells_for(callsets, vid)
    assert st["deferred"] == 0, "every numeric token of the fixtures is inside the fast path"


def test_fixture_census(sim):
    files = set()
    for callsets, vid in PAIRS:
        cs = json.load(open(_paths(callsets, vid)[1]))["callsets"]
        files.update(x["filename"] for x in (cs.values() if isinstance(cs, dict) else cs))
    assert "inputs/vcfs/t0_1_2_combined.vcf.gz" in files       # the multi-sample file: INFO sums divided among 3 samples


@pytest.mark.parametrize("treat", [True, False])
def test_bodies_partition_cut(gdb, sim, treat):
    v, c = _paths("t0_1_2.json", "vid.json")
    cut = 12200
    for begin, end in ((0, cut - 1), (cut, 2**63 - 2)):
        want, ncells = gdb.import_cells(v, c, file_root=helpers.GOLDEN, treat_deletions_as_intervals=treat, column_begin=begin, column_end=end)
        got, st = sim_import(sim, v, c, treat, begin, end)
        assert got == want and st["cells"] == ncells and st["deferred"] == 0
        if begin:
            assert st["spanning"] > 0, "the fixture has reference blocks across column %d" % cut
    v, c = _paths("t0_overlapping.json", "vid.json")
    want, _ = gdb.import_cells(v, c, file_root=helpers.GOLDEN, treat_deletions_as_intervals=treat, column_begin=12202)
    assert sim_import(sim, v, c, treat, 12202)[0] == want


def test_device_argument_none_is_the_host_path(gdb):
    v, c = _paths("t0_1_2.json", "vid.json")
    assert gdb.import_cells(v, c, file_root=helpers.GOLDEN, device=None, text_budget_bytes=0, stats=None) == gdb.import_cells(v, c, file_root=helpers.GOLDEN)
    from genomicsdb_amd import _lib
    assert "gdbamd_import_cells_device" in _lib.SYMBOLS and hasattr(_lib.lib(), "gdbamd_import_cells_device")


@pytest.mark.parametrize("callsets,vid", PAIRS_2D, ids=["%s-%s" % p for p in PAIRS_2D])
def test_two_dimensional_fields_are_refused_by_name(gdb, sim, callsets, vid):
    v, c = _paths(callsets, vid)
    assert gdb.import_cells(v, c, file_root=helpers.GOLDEN)[1] > 0       # the host importer keeps serving the vid
    with pytest.raises(RuntimeError, match=r"field \w+: .*not imported by the device importer"):
        sim_import(sim, v, c)


# ---- numbers ---------------------------------------------------------------------------------------------------------------
def _blob(strings):
    offs, at = [], 0
    for s in strings:
        offs.append(at)
        at += len(s) + 1
    return b"".join(s.encode() + b"\0" for s in strings), (ctypes.c_uint32 * len(strings))(*offs)


def _significant(digits):
    return len(digits.strip("0"))


def _random_decimal(rng, promised):
    """a decimal string and whether the fast path promises to take it: at most 15 digits after stripping leading and trailing zeros
    of the digit string, and the decimal exponent over that stripped digit string read as an integer within +-22"""
    while True:
        nd = rng.randrange(1, 16) if promised else rng.randrange(1, 21)
        digits = "".join(rng.choice("0123456789") for _ in range(nd))
        point = rng.randrange(0, nd + 1)              # digits in front of the point: 0 = leading '.', nd = none or a trailing '.'
        ex = rng.randrange(-45, 41)
        stripped = digits.strip("0")
        trailing = len(digits) - len(digits.rstrip("0")) if stripped else 0
        e10 = ex - (nd - point) + trailing            # exponent of `stripped` read as an integer
        ok = not stripped or (len(stripped) <= 15 and -22 <= e10 <= 22)
        if promised and not ok:
            continue
        s = rng.choice(["", "", "-", "+"]) + digits[:point] + ("." if point < nd or rng.random() < 0.2 else "") + digits[point:]
        if ex or rng.random() < 0.3:
            s += rng.choice("eE") + rng.choice(["", "+"] if ex >= 0 else ["-"]) + str(abs(ex))
        return s, ok


def test_float_fast_path_has_the_bits_of_strtod(sim):
    rng = random.Random(77)
    cases = [_random_decimal(rng, i % 2 == 0) for i in range(200000)]
    cases += [(s, True) for s in ("0", "-0", "+0.0", "0e99", "1", "-1.5", "1e22", "1e-22", "123456789012345", "1234567890123450000000", ".5", "5.", "-.5e-3",
                                  "100.000", "0.000000000000000000001", "9007199254740993e0"[:15], "475.77", "1E5")]
    cases += [(s, False) for s in ("1234.5678901234567", "1e-30", "1e23", "nan", "NaN", "inf", "Inf", "-inf", "infinity", "0x1p3", " 1", "1 ", "1%", "", ".", "+", "-.",
                                   "1e", "1e+", "1.2.3", "abc", "1,2", "1_0", "1234567890123456", "1e-23")]
    strings = [s for s, _ in cases]
    n = len(strings)
    blob, offs = _blob(strings)
    acc, rok = (ctypes.c_uint8 * n)(), (ctypes.c_uint8 * n)()
    bits, rbits = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    sim.hsi_check_floats(blob, offs, n, acc, bits, rok, rbits)
    promised = sum(1 for _, ok in cases if ok)
    assert promised * 2 >= n
    wrong = [(strings[i], hex(bits[i]), hex(rbits[i])) for i in range(n) if acc[i] and (not rok[i] or bits[i] != rbits[i])]
    assert not wrong, wrong[:10]
    refused = [strings[i] for i in range(n) if cases[i][1] and not acc[i]]
    assert not refused, refused[:10]
    parsed_outside = [s for s in ("1234.5678901234567", "1e-30", "1e23", "nan", "Inf", "inf", "0x1p3", " 1", "1%", "", ".", "1e", "abc") if acc[strings.index(s)]]
    assert not parsed_outside
    # hand-checked bits
    want = {"475.77": struct.unpack("<I", struct.pack("<f", 475.77))[0], "-0": 0x80000000, "1E5": 0x47C35000, ".5": 0x3F000000, "1e22": 0x64078678}
    for s, w in want.items():
        assert acc[strings.index(s)] and bits[strings.index(s)] == w, s


def test_int_fast_path_has_the_value_of_strtoll(sim):
    rng = random.Random(78)
    strings = []
    for _ in range(200000):
        nd = rng.randrange(1, 22)
        strings.append(rng.choice(["", "", "-", "+"]) + "".join(rng.choice("0123456789") for _ in range(nd)))
    must = ["0", "-0", "+7", "007", "9223372036854775807", "-9223372036854775808", "1234567890123456789", "2147483648", "-2147483649"]
    deferred = ["9223372036854775808", "-9223372036854775809", "99999999999999999999", "", "+", "-", " 7", "7 ", "abc", "1.0", "1e3", "0x10", "--1", "7%"]
    strings += must + deferred
    n = len(strings)
    blob, offs = _blob(strings)
    acc, rok = (ctypes.c_uint8 * n)(), (ctypes.c_uint8 * n)()
    val, rval = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
    sim.hsi_check_ints(blob, offs, n, acc, val, rok, rval)
    for i, s in enumerate(strings):
        fits = re.fullmatch(r"[+-]?[0-9]+", s) is not None and -2**63 <= int(s) <= 2**63 - 1
        assert bool(acc[i]) == fits, s
        if acc[i]:
            assert rok[i] and val[i] == rval[i] == int(s), s
    assert all(acc[strings.index(s)] for s in must) and not any(acc[strings.index(s)] for s in deferred)


# ---- the hand-made VCF -----------------------------------------------------------------------------------------------------
def _cells(buf):
    out, off = [], 0
    while off < len(buf):
        row, col, size, end = struct.unpack_from("<qqQq", buf, off)
        out.append((row, col, end, buf[off:off + size]))
        off += size
    return out


def _f32(x):
    return struct.pack("<f", x)


def test_hand_made_vcf(gdb, sim):
    v, c = _paths(*HAND)
    raw = open(os.path.join(INPUTS, "vcfs", "import_hand.vcf"), "rb").read()
    assert b"\r\n\r\n" in raw and not raw.endswith(b"\n")          # \r\n endings, an empty line, no final newline
    for treat in (True, False):
        want, ncells = gdb.import_cells(v, c, file_root=helpers.GOLDEN, treat_deletions_as_intervals=treat)
        got, st = sim_import(sim, v, c, treat)
        assert got == want and st["cells"] == ncells == 8 and st["records"] == 4
        assert st["deferred"] == HAND_DEFERRED
    cells = {(r, col): (end, raw) for r, col, end, raw in _cells(sim_import(sim, v, c, True)[0])}
    off2 = 249250621
    assert sorted(cells) == [(0, 99), (0, 199), (0, 299), (0, off2 + 49), (1, 99), (1, 199), (1, 299), (1, off2 + 49)]
    # END=150;END=180: the last one counts.  REF C, ALT '&', no ID, QUAL null, no FILTER
    end, b = cells[(0, 99)]
    assert end == 179
    assert b[24:].startswith(struct.pack("<qi", 179, 1) + b"C" + struct.pack("<i", 1) + b"&" + struct.pack("<i", 0) + struct.pack("<I", 0x7F7FFFFF) + struct.pack("<i", 0))
    # INFO DP=7 among 2 samples: 4 and 3 (the vid's first INFO attribute after END, right behind FILTER)
    fixed = 24 + 8 + 5 + 5 + 4 + 4 + 4
    assert struct.unpack_from("<i", cells[(0, 99)][1], fixed)[0] == 4 and struct.unpack_from("<i", cells[(1, 99)][1], fixed)[0] == 3
    # GT 0/0 in the PP layout: 3 values 0, unphased, 0; GT '.': one missing allele
    assert struct.pack("<iiii", 3, 0, 0, 0) in cells[(0, 99)][1] and cells[(1, 99)][1].count(struct.pack("<ii", 1, -1)) >= 1
    # the lower-case deletion ACGt -> A is an interval of 4 when deletions are intervals
    end, b = cells[(0, 199)]
    assert end == 202 and sim_import(sim, v, c, False)[0] != sim_import(sim, v, c, True)[0]
    assert struct.pack("<i", 7) + b"rs1;rs2" in b and struct.pack("<i", 3) + b"A|&" in b
    assert _f32(1234.5678901234567) + struct.pack("<i", 2) in b                     # deferred QUAL, then a two-name FILTER
    assert _f32(1e-30) in b and struct.pack("<I", 0x7FC00000) in b                  # deferred MQ=1e-30 and FS=nan
    assert struct.pack("<i", 2) + _f32(0.5) + struct.pack("<I", 0x7F800001) in b    # AF=0.5,. : bcf missing inside a vector
    assert _f32(1.5) + struct.pack("<I", 0x7F800001) in b                           # fixed-length FQ=1.5,.
    assert struct.pack("<iiii", 1, -2**31, 3, 4) in b                               # SB=1,.,3,4
    assert struct.pack("<iiii", 3, 0, 1, 1) in b                                    # GT 0|1
    dp = 24 + 8 + 8 + 7 + 11 + 4 + 12
    assert struct.unpack_from("<i", b, dp)[0] == -1 and struct.unpack_from("<i", cells[(1, 199)][1], dp)[0] == -2      # DP=-3: floor division
    assert struct.pack("<iiii", 3, -1, 0, -1) in cells[(1, 199)][1]                 # GT ./.
    # haploid and triploid GT; QUAL Inf (deferred); MLEAC=5,3 among 2 samples
    b0, b1 = cells[(0, off2 + 49)][1], cells[(1, off2 + 49)][1]
    assert struct.pack("<I", 0x7F800000) in b0 and struct.pack("<iii", 2, 3, 2) in b0 and struct.pack("<iii", 2, 2, 1) in b1
    assert struct.pack("<ii", 1, 1) in b0 and struct.pack("<iiiiii", 5, 0, 0, 1, 0, 2) in b1
    assert struct.pack("<i", 5) + b"hello" in b0
