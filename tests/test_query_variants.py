"""The variants query: `gt_mpi_gather` without a mode flag (VariantQueryProcessor::gt_get_column_interval, query_variants.cc:687-843;
GA4GHOperator, variant_operations.cc:572-728; print_variants' default format, variant.cc:983-999).

1. the reference's ten "variants" goldens (tests/golden/outputs/*_variants_*, parameters in variants_cases.py), byte for byte, through the
   kernel bodies on the CPU (tests/hostsim_variants) and through CombineEngine.query_variants() on the device;
2. the command line;
3. tests/tools/variants_model.py - a plain-Python restatement on top of the oracle's --print-calls document - for what the goldens do not
   reach: calls whose ALT order differs from the merged order, a haploid call, a deletion reaching a query begin, intervals sharing a cell
   (hand-made input `variants_hand`, with the permuted values also written out by hand), 400 and 1 000 synthetic samples.
   With 200 samples over 3 kb the synthetic generator yields only 24 variants of two and more calls in the four intervals (samples rarely
   share begin, end, REF and ALT set), below the 50 asked for, so the sample count of that input is raised to 400 (92 such variants); the
   generator itself is untouched.  The condition is asserted from the model before anything is compared;
4. the "%.6f" float emitter against this machine's libc;
5. edges: attributes without REF / ALT (this project's query configuration adds them: see EDGE_QUERIES), a single-position interval, an interval without cells, a call above the allele cap.
"""
import ctypes, json, os, struct, subprocess
import numpy as np
import pytest

import helpers
from variants_cases import VARIANTS_CASES
from test_print_calls import calls_query, oracle_print_calls, _synth_calls_query
import variants_model as vm

EMPTY = b'{\n    "variants": [\n\n    ]\n}\n'


@pytest.fixture()
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


_lib = None


def hostsim_variants_lib():
    global _lib
    if _lib is None:
        d = os.path.join(helpers.ROOT, "tests", "hostsim_variants")
        subprocess.check_call(["make", "-s", "-C", d])
        _lib = ctypes.CDLL(os.path.join(d, "libhostsim_variants.so"))
        _lib.hostsim_query_variants.restype = ctypes.c_int
        _lib.hostsim_query_variants.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
                                                ctypes.c_char_p, ctypes.c_uint64]
        _lib.hostsim_variants_free.argtypes = [ctypes.c_void_p]
    return _lib


def hostsim_query_variants(q, cells):
    lib = hostsim_variants_lib()
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    err = ctypes.create_string_buffer(4096)
    rc = lib.hostsim_query_variants(json.dumps(q).encode(), cells, len(cells), ctypes.byref(out), ctypes.byref(n), err, 4096)
    if rc != 0:
        raise RuntimeError("hostsim_variants: " + err.value.decode())
    text = ctypes.string_at(out.value, n.value)
    lib.hostsim_variants_free(out)
    return text


def device_query_variants(gdb, q, cells, windowed=False):
    eng = gdb.CombineEngine(q)
    if windowed:
        eng.open_memory_cells(cells)
    else:
        eng.stage_cells(cells)
    try:
        return eng.query_variants()
    finally:
        eng.close()


# ---- 1. the reference's goldens ---------------------------------------------------------------------------------------------------------
def _check_golden(got, name):
    want = helpers.golden_text(name)
    assert json.loads(got) == json.loads(want)      # structure first (what the reference's own test accepts) ...
    assert got == want                              # ... then the bytes


@pytest.mark.parametrize("case", VARIANTS_CASES, ids=[c[0] for c in VARIANTS_CASES])
def test_kernel_bodies_print_the_reference_variants_goldens(case):
    name, callsets, vid, ranges, attributes = case
    _check_golden(hostsim_query_variants(calls_query(callsets, vid, ranges, attributes), helpers.cells_for(callsets, vid)), name)


@pytest.mark.gpu
@pytest.mark.parametrize("case", VARIANTS_CASES, ids=[c[0] for c in VARIANTS_CASES])
def test_device_prints_the_reference_variants_goldens(gdb, case):
    name, callsets, vid, ranges, attributes = case
    _check_golden(device_query_variants(gdb, calls_query(callsets, vid, ranges, attributes), helpers.cells_for(callsets, vid)), name)


# ---- 2. the command line ------------------------------------------------------------------------------------------------------------------
def _cli(tmp_path, extra):
    name, callsets, vid, ranges, attributes = [c for c in VARIANTS_CASES if c[0] == "t0_1_2_variants_at_12150"][0]
    ws = tmp_path / "ws"
    (ws / "arr").mkdir(parents=True)
    (ws / "arr" / "cells.bin").write_bytes(helpers.cells_for(callsets, vid))
    q = calls_query(callsets, vid, ranges, attributes)
    q["workspace"], q["array"] = str(ws), "arr"
    qf = tmp_path / "q.json"
    qf.write_text(json.dumps(q))
    exe = os.path.join(helpers.ROOT, "genomicsdb_amd", "gt_mpi_gather")
    return name, subprocess.run([exe, "-j", str(qf)] + extra, capture_output=True, timeout=300)


@pytest.mark.gpu
def test_gt_mpi_gather_without_a_mode_flag_prints_the_variants(gdb, tmp_path):
    name, r = _cli(tmp_path, [])
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == helpers.golden_text(name)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["Cotton-JSON", "Positions-JSON", "GA4GH"])
def test_gt_mpi_gather_refuses_the_other_variant_formats(gdb, tmp_path, fmt):
    name, r = _cli(tmp_path, ["-O", fmt])
    assert r.returncode != 0 and fmt.encode() in r.stderr and not r.stdout


# ---- 3. the model ---------------------------------------------------------------------------------------------------------------------------
HAND = ("variants_hand.json", "vid.json")
HAND_ATTRIBUTES = ["REF", "ALT", "MQ", "DP", "GT", "GQ", "AD", "PL", "DP_FORMAT", "MIN_DP"]
# contig "1" starts at column 0: VCF position p is column p - 1.  [1049, 2000] begins inside the reference blocks of all three samples,
# [2000, 2499] shares the cells at column 2000 with it, [3001, 3010] begins inside the deletions TAC -> T that begin at 3000
HAND_RANGES = [{"range_list": [{"low": 1049, "high": 2000}, {"low": 2000, "high": 2499}, {"low": 3001, "high": 3010}]}]


def _model(q, cells):
    doc = json.loads(oracle_print_calls(q, cells))
    return vm.variants_from_calls(doc, q["attributes"], vm.vid_lengths(q["vid_mapping_file"]))


def _multi(model):
    return [v for v in model["variants"] if len(v["variant_calls"]) >= 2]


def _assert_equals_model(got, model):
    doc = json.loads(got)
    assert vm.round6(doc) == vm.round6(model)


def _hand():
    cells = helpers.cells_for(*HAND)
    q = calls_query(HAND[0], HAND[1], HAND_RANGES, HAND_ATTRIBUTES)
    model = _model(q, cells)
    permuted = [v for v in _multi(model) if any(c["fields"]["ALT"] != v["common_fields"]["ALT"] for c in v["variant_calls"])]
    assert len(permuted) >= 1                      # the condition of the input, from the model
    return q, cells, model


def _check_hand_written(doc):
    """the variant at column 2000 (G -> A,C,<NON_REF> / C,A,<NON_REF> / haploid C,A,<NON_REF>), derived by hand from remap_GT_field,
    remap_data_based_on_alleles and remap_data_based_on_genotype: merged order is the first call's, A,C,<NON_REF>; the second and third call
    carry allele 1 = C = merged 2 and allele 2 = A = merged 1, so m2i = [0, 2, 1, 3].  Diploid PL: merged genotype (j, k) at k(k+1)/2 + j
    reads input genotype (m2i[j], m2i[k]): 0<-0, 1<-(0,2)=3, 2<-(2,2)=5, 3<-(0,1)=1, 4<-(1,2)=4, 5<-(1,1)=2, 6<-6, 7<-(2,3)=8, 8<-(1,3)=7, 9<-9."""
    at = [v for v in doc["variants"] if v["interval"] == [2000, 2000]]
    assert len(at) == 2                            # once per query interval that holds the cell
    for v in at:
        assert v["common_fields"] == {"REF": "G", "ALT": ["A", "C", "<NON_REF>"]}
        c0, c1, c2 = v["variant_calls"]
        assert [c["row"] for c in (c0, c1, c2)] == [0, 1, 2]
        assert c0["fields"]["ALT"] == ["A", "C", "<NON_REF>"] and c1["fields"]["ALT"] == ["C", "A", "<NON_REF>"] and c2["fields"]["ALT"] == ["C", "A", "<NON_REF>"]
        assert c0["fields"]["GT"] == [1, 2] and c0["fields"]["AD"] == [10, 20, 30, 4] and c0["fields"]["PL"] == [900, 0, 810, 40, 0, 777, 950, 960, 970, 999]
        assert c1["fields"]["GT"] == [2, 1] and c1["fields"]["AD"] == [11, 31, 21, 5]
        assert c1["fields"]["PL"] == [100, 103, 105, 101, 104, 102, 106, 108, 107, 109]
        assert c2["fields"]["GT"] == [2] and c2["fields"]["AD"] == [7, 9, 8, 1] and c2["fields"]["PL"] == [50, 52, 51, 53]
    # the deletions that begin in front of the third interval: found by the left sweep, one variant of two calls, identity remap
    dels = [v for v in doc["variants"] if v["interval"] == [3000, 3002]]
    assert len(dels) == 1 and [c["row"] for c in dels[0]["variant_calls"]] == [0, 1] and dels[0]["common_fields"] == {"REF": "TAC", "ALT": ["T", "<NON_REF>"]}
    # the reference blocks that reach column 1049: rows 0 and 1 share begin and end, row 2 ends earlier
    blocks = [v for v in doc["variants"] if v["interval"][0] == 1000]
    assert [[c["row"] for c in v["variant_calls"]] for v in blocks] == [[0, 1], [2]]
    assert blocks[0]["common_fields"] == {"REF": "C", "ALT": ["<NON_REF>"]} and blocks[1]["common_fields"] == {}


def test_hand_made_input_kernel_bodies_against_the_model_and_the_hand_written_values():
    q, cells, model = _hand()
    got = hostsim_query_variants(q, cells)
    _check_hand_written(json.loads(got))
    _check_hand_written(model)
    _assert_equals_model(got, model)


@pytest.mark.gpu
def test_hand_made_input_device_against_the_model_and_the_hand_written_values(gdb):
    q, cells, model = _hand()
    got = device_query_variants(gdb, q, cells)
    _check_hand_written(json.loads(got))
    _assert_equals_model(got, model)
    assert got == hostsim_query_variants(q, cells)


def _synth(tmp_path, N, L, ranges):
    from genomicsdb_amd import synth
    B = 10_000_000
    cells, _ = synth.Generator(N, B, L).chunk_bytes(B + L)
    q = _synth_calls_query(tmp_path, N, [{"range_list": [{"low": B + lo, "high": B + hi} for lo, hi in ranges]}])
    model = _model(q, cells)
    assert len(_multi(model)) >= 50                # the condition of the input, from the model
    return q, cells, model


def test_400_synthetic_samples_kernel_bodies_against_the_model(tmp_path):
    """the four interval shapes of test_oracle_and_kernel_bodies_agree_on_synthetic_cells"""
    q, cells, model = _synth(tmp_path, 400, 3000, [(700, 900), (1500, 1500), (2000, 2600), (50_000, 50_010)])
    _assert_equals_model(hostsim_query_variants(q, cells), model)


@pytest.mark.gpu
def test_400_synthetic_samples_device_against_the_model(gdb, tmp_path):
    q, cells, model = _synth(tmp_path, 400, 3000, [(700, 900), (1500, 1500), (2000, 2600), (50_000, 50_010)])
    got = device_query_variants(gdb, q, cells)
    _assert_equals_model(got, model)
    assert got == hostsim_query_variants(q, cells)


@pytest.mark.gpu
def test_1000_samples_resident_and_through_column_windows(gdb, tmp_path, monkeypatch):
    """1 000 samples x 20 kb: the resident array and the same array streamed through HBM in column windows give the same bytes, equal to the model"""
    q, cells, model = _synth(tmp_path, 1000, 20_000, [(5000, 15_000), (17_000, 17_000)])
    got = device_query_variants(gdb, q, cells)
    monkeypatch.setenv("GDBAMD_STAGE_BUDGET_BYTES", str(len(cells) // 7))
    got2 = device_query_variants(gdb, q, cells, windowed=True)
    assert got2 == got
    _assert_equals_model(got, model)


# ---- 4. float spelling ------------------------------------------------------------------------------------------------------------------------
def test_fixed6_float_text_equals_libc():
    """put_float_fixed6 against snprintf("%.6f", (double)f) - what std::fixed << std::setprecision(6) << float prints - for 100 000 random bit
    patterns and the special values"""
    lib = hostsim_variants_lib()
    libc = ctypes.CDLL(None)
    libc.snprintf.restype = ctypes.c_int
    rng = np.random.default_rng(20240607)
    bits = rng.integers(0, 1 << 32, size=100_000, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00400000, 0x00800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
                        0x7F800001, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F000000, 0x358637BD, 0x3A83126F, 0x49742400, 0x4B000000, 0x4B800000, 0x36A7C5AC, 0x3727C5AC], dtype=np.uint32)
    vals = np.concatenate([special, bits]).view(np.float32)
    buf = ctypes.create_string_buffer(64 * len(vals))
    fn = lib.hostsim_put_float_fixed6_many
    fn.restype = ctypes.c_int64
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_char_p, ctypes.c_uint64]
    n = fn(vals.ctypes.data, len(vals), buf, len(buf))
    assert n > 0
    mine = buf.raw[:n].split(b"\n")[:-1]
    assert len(mine) == len(vals)
    one = ctypes.create_string_buffer(128)
    for v, m in zip(vals, mine):
        k = libc.snprintf(one, 128, b"%.6f", ctypes.c_double(float(v)))
        assert m == one.raw[:k], (hex(struct.unpack("<I", struct.pack("<f", v))[0]), m, one.raw[:k])


# ---- 5. edges ---------------------------------------------------------------------------------------------------------------------------------
EDGE_QUERIES = {
    # VariantQueryConfig of this project adds END, REF and ALT to every query (host/variant_query_config.cc), so a query JSON cannot ask for calls
    # without them: the one-variant-per-call branch of find_or_insert is out of reach from here, and what such a query gives is what the model
    # gives for the attributes in effect (grouped, REF / ALT printed)
    "attributes_without_REF_and_ALT": (["GQ", "DP_FORMAT", "MIN_DP"], HAND_RANGES),
    "single_position": (HAND_ATTRIBUTES, [{"range_list": [{"low": 1049, "high": 1049}]}]),
    "no_cells": (HAND_ATTRIBUTES, [{"range_list": [{"low": 500_000, "high": 500_100}]}]),
}


def _edge(name):
    attributes, ranges = EDGE_QUERIES[name]
    cells = helpers.cells_for(*HAND)
    q = calls_query(HAND[0], HAND[1], ranges, attributes)
    return q, cells, _model(q, cells)


def _check_edge(name, got, model):
    _assert_equals_model(got, model)
    doc = json.loads(got)
    if name == "attributes_without_REF_and_ALT":
        assert all("REF" in c["fields"] and "ALT" in c["fields"] and "PL" not in c["fields"] for v in doc["variants"] for c in v["variant_calls"])
    if name == "single_position":
        assert [v["interval"] for v in doc["variants"]] == [[1000, 1099], [1000, 1059]]      # the left sweep only
    if name == "no_cells":
        assert got == EMPTY


@pytest.mark.parametrize("name", list(EDGE_QUERIES))
def test_edges_kernel_bodies(name):
    q, cells, model = _edge(name)
    _check_edge(name, hostsim_query_variants(q, cells), model)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGE_QUERIES))
def test_edges_device(gdb, name):
    q, cells, model = _edge(name)
    _check_edge(name, device_query_variants(gdb, q, cells), model)


def _cells_with_too_many_alleles():
    """the hand-made cells with one ALT string of 64 alleles (65 with REF, above GDB_MAX_INPUT_ALLELES = 64) in place of `A|C|&` of row 0"""
    cells = helpers.cells_for(*HAND)
    old = struct.pack("<i", 5) + b"A|C|&"
    assert cells.count(old) == 1
    alt = "|".join("A" * (i + 2) for i in range(63)) + "|&"
    at = cells.index(old)
    # the cell: row, column, size (int64, int64, uint64) then END, REF ("G"), ALT: the size field sits 8 + 4 + 1 + 8 bytes in front of the ALT length
    size_at = at - (8 + 4 + 1) - 8
    (size,) = struct.unpack_from("<Q", cells, size_at)
    new = struct.pack("<i", len(alt)) + alt.encode()
    return cells[:size_at] + struct.pack("<Q", size + len(new) - len(old)) + cells[size_at + 8:at] + new + cells[at + len(old):]


def test_a_call_above_the_allele_cap_is_an_error_kernel_bodies():
    q = calls_query(HAND[0], HAND[1], HAND_RANGES, HAND_ATTRIBUTES)
    with pytest.raises(RuntimeError, match="error bits"):
        hostsim_query_variants(q, _cells_with_too_many_alleles())


@pytest.mark.gpu
def test_a_call_above_the_allele_cap_is_an_error_device(gdb):
    q = calls_query(HAND[0], HAND[1], HAND_RANGES, HAND_ATTRIBUTES)
    with pytest.raises(Exception, match="GDB_MAX_INPUT_ALLELES"):
        device_query_variants(gdb, q, _cells_with_too_many_alleles())
