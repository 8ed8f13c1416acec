"""CombineEngine.record_tensors: the pages of a "bu" engine decoded on the device into typed column tensors (kernels/gdb_columns.hip), against the
plain-Python model tests/tools/columns_model.py applied (a) to the same engine's own BCF2 stream fetched with run_interval - every column, floats
and QUAL as bits - and (b) to the oracle's VCF text - the integer, GT and site columns.  tests/test_columns_bodies_cpu.py holds the model against
the kernel bodies and against itself without a device."""
import json
import struct

import numpy as np
import pytest

import helpers
import bcf2text
import columns_model as cm
import hot_record_inputs as hri
from golden_cases import CASES

pytestmark = pytest.mark.gpu
QUERY_CASES = [c for c in CASES if c[5] == "query"]


def offsets_of(q):
    c = json.load(open(q["vid_mapping_file"]))["contigs"]
    items = c.items() if isinstance(c, dict) else [(x["name"], x) for x in c]
    return {name: x["tiledb_column_offset"] for name, x in items}


def intervals_of(q):
    r = q["query_column_ranges"][0]
    if isinstance(r, dict):
        return [(x["low"], x["high"]) for x in r["range_list"]]
    return [(x, x) if isinstance(x, int) else (x[0], x[1]) for x in r]


def to_numpy(page):
    """one page of record_tensors as numpy arrays that own their memory; float32 tensors as their bits"""
    import torch
    out = {}
    for name, t in page.items():
        if t.dtype == torch.float32:
            t = t.view(torch.int32)
            out[name] = t.cpu().numpy().view(np.uint32).copy()
        else:
            out[name] = t.cpu().numpy().copy()
    return out


def split_records(body):
    at, recs = 0, []
    while at < len(body):
        l_shared, l_indiv = struct.unpack_from("<II", body, at)
        recs.append(body[at:at + 8 + l_shared + l_indiv])
        at += 8 + l_shared + l_indiv
    return recs


def same(got, want, names=None):
    for name in (names if names is not None else want):
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].dtype, got[name].shape, want[name].dtype, want[name].shape)
        assert np.array_equal(got[name], want[name]), name


def engine_columns(e, ivs, fields, arena_bytes=1 << 26, stats=None):
    pages = []
    for b, en in ivs:
        pages += [to_numpy(p) for p in e.record_tensors(b, en, fields=fields, arena_bytes=arena_bytes, stats=stats)]
    return pages


def own_stream_model(e, ivs, fields, n_sample, offsets, arena_bytes=1 << 26):
    """the model over the records of the engine's own "bu" stream"""
    records = []
    for b, en in ivs:
        records += split_records(e.run_interval(b, en, arena_bytes=arena_bytes)[0])
    return cm.columns_from_records(e.header.decode(), records, n_sample, fields, offsets), records


# ---- 1. goldens --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_goldens_as_columns(case):
    import genomicsdb_amd
    name, callsets, vid, ov, golden, mode = case
    cells = helpers.cells_for(callsets, vid)
    q, _ = helpers.query_json(callsets, vid, ov, mode)
    text, _, _ = helpers.oracle_run(q, cells)
    assert text == helpers.golden_text(golden)
    offsets, ivs = offsets_of(q), intervals_of(q)
    e = genomicsdb_amd.CombineEngine(q, output_format="bu")
    try:
        e.stage_cells(cells)
        fields = cm.numeric_fields(e.header.decode())
        n_sample = 0 if ov.get("sites_only_query") else len(e.header.decode().split("#CHROM")[1].split("\n")[0].split("\t")) - 9
        want, records = own_stream_model(e, ivs, fields, n_sample, offsets)
        got = cm.pad_and_concatenate(engine_columns(e, ivs, fields))
        assert len(records) > 0 and sorted(got) == sorted(want)
        same(got, want)
        from_text = cm.columns_from_text(text, fields, offsets)
        assert set(from_text) >= set(cm.SITE) | ({"INFO/DP"} if "INFO/DP" in fields else set())
        assert cm.agree(got, from_text) == []
        if name == "t0_haploid_triploid_1_2_3_triploid_deletion_vcf_produce_GT":
            gt = want["GT"]
            assert gt.shape[2] == 3 and (gt[:, :, 2] == cm.VEND["int8"]).any() and (gt[:, :, 2] >= 0).any()
    finally:
        e.close()


# ---- 2. sample counts around the wavefront, one page and several ---------------------------------------------------------------------------
SYNTH_FIELDS = {"GT": "int8", "DP": "int16", "GQ": "int16", "MIN_DP": "int16", "AD": "int32", "PL": "int32"}


@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_sample_counts_around_the_wavefront(tmp_path, N):
    import genomicsdb_amd
    from genomicsdb_amd import synth
    B, L = 10_000_000, 2000
    g = synth.Generator(N, B, L)
    cells, _ = g.chunk_bytes(B + L)
    q = helpers.synth_query(tmp_path, N, B, B + L - 1)
    text, nrec, _ = helpers.oracle_run_synth(q, cells, synth.SEED)
    offsets = offsets_of(q)
    from_text = cm.columns_from_text(text, SYNTH_FIELDS, offsets)
    e = genomicsdb_amd.CombineEngine(q, output_format="bu")
    try:
        e.stage_cells(cells)
        e.set_reference(B, synth.reference(B, L + 16))
        _, st = e.run_interval(B, B + L - 1, arena_bytes=1 << 28, fetch=False)
        assert st.pages == 1 and st.num_records == nrec
        small = st.bytes_out // 4       # (a page holds one record at least)
        _, st_small = e.run_interval(B, B + L - 1, arena_bytes=small, fetch=False)
        assert st_small.pages >= 3
        want, records = own_stream_model(e, [(B, B + L - 1)], SYNTH_FIELDS, N, offsets, arena_bytes=1 << 28)
        one = engine_columns(e, [(B, B + L - 1)], SYNTH_FIELDS, arena_bytes=1 << 28)
        stats = []
        several = engine_columns(e, [(B, B + L - 1)], SYNTH_FIELDS, arena_bytes=small, stats=stats)
        assert len(one) == 1 and len(several) == st_small.pages == len(stats) and sum(s["records"] for s in stats) == nrec
        assert one[0]["GT"].shape[:2] == (nrec, N) and one[0]["GT"].dtype == np.int8 and one[0]["DP"].dtype == np.int16
        joined = cm.pad_and_concatenate(several)
        same(one[0], want)
        same(joined, want)
        assert cm.agree(joined, from_text) == [] and set(from_text) >= set(SYNTH_FIELDS) | set(cm.SITE)
    finally:
        e.close()


# ---- 3. hot records -------------------------------------------------------------------------------------------------------------------------
class FixedCall(hri.Call):
    """a call G -> T,<NON_REF> of tests/hot_record_inputs.py with its GQ and PL written down instead of drawn"""

    def __init__(self, pos, gq=20, pl=None):
        hri.Call.__init__(self, pos, "G", ["T"], pl=pl is not None)
        self.gq, self.pl_values = gq, pl

    def line(self, rnd):
        fmt, val = "GT:AD:DP:GQ", "0/1:3,3,3:9:%d" % self.gq
        if self.pl_values is not None:
            fmt, val = fmt + ":PL", val + ":" + ",".join(map(str, self.pl_values))
        return "1\t%d\t.\tG\tT,<NON_REF>\t100\t.\tDP=9;MQ=40.5\t%s\t%s\n" % (self.pos, fmt, val)


def header_samples(e):
    return len(e.header.decode().split("#CHROM")[1].split("\n")[0].split("\t")) - 9


def test_hot_records_with_long_mixed_vectors(tmp_path):
    """the hot record of hot_record_inputs.first_appearance (40 calls that list 1-3 of 30 insertions: PL of hundreds of int16 elements) with, in the
    same page, a record whose PL fits int8 and one whose PL needs int32"""
    import random
    import genomicsdb_amd
    rnd = random.Random(11)
    pool = hri._pool(rnd, 30)
    samples = [[hri.Call(hri.HOT, "G", rnd.sample(pool, rnd.randint(1, 3)), nr=row % 4 != 1)] for row in range(40)]
    samples[0].append(FixedCall(hri.HOT + 10, pl=[0, 7, 90, 12, 100, 127]))
    samples[1].append(FixedCall(hri.HOT + 10, pl=[5, 0, 60, 9, 70, 80]))
    samples[2].append(FixedCall(hri.HOT + 20, pl=[0, 70000, 90, 12, 100, 127]))
    cells, q = hri._import(tmp_path, samples, 11)
    facts = hri.interval_facts(samples, hri.HOT, hri.HOT + 20)
    assert facts["calls"][hri.HOT - 1] >= 25 and facts["distinct"][hri.HOT - 1] >= 20 and facts["num_records"] == 3
    iv = [(facts["begin"], facts["end"])]
    text, _, _ = helpers.oracle_run(hri.query_for(q, facts), cells)
    offsets = offsets_of(q)
    fields = {"GT": "int8", "DP": "int16", "GQ": "int16", "AD": "int32", "PL": "int32"}
    e = genomicsdb_amd.CombineEngine(q, output_format="bu")
    try:
        e.stage_cells(cells)
        want, records = own_stream_model(e, iv, fields, header_samples(e), offsets)
        key = {n: i for i, n in bcf2text.Header(e.header.decode()).ids.items()}
        pl = [cm.parse_record(r)["fmt"][key["PL"]] for r in records]
        pages = engine_columns(e, iv, fields)
        assert len(pages) == 1 and len(records) == 3                        # one page ...
        assert max(len(per[0]) for _, per in pl) > 14                         # ... whose PL vectors overflow the descriptor's count ...
        assert {t for t, _ in pl} == {bcf2text.BT_INT8, bcf2text.BT_INT16, bcf2text.BT_INT32}      # ... and come in all three integer classes
        same(pages[0], want)
        assert cm.agree(pages[0], cm.columns_from_text(text, fields, offsets)) == []
    finally:
        e.close()


def test_real_values_that_equal_a_sentinel_of_the_dtype_asked_for(tmp_path):
    """-127 and -128 in an int16 block are numbers, not int8's end-of-vector and missing; -32767 in an int32 block is no int16 end-of-vector: asked for
    in the narrow dtype they are errors, in the block's own they come through"""
    import genomicsdb_amd
    exc = genomicsdb_amd.api.GenomicsDBException
    gq = {20100: (5, -120), 20200: (300, -127), 20300: (300, -128), 20400: (70000, -32767)}
    samples = [[FixedCall(pos, gq=v[row]) for pos, v in gq.items()] for row in (0, 1)]
    cells, q = hri._import(tmp_path, samples, 1)
    offsets = offsets_of(q)
    e = genomicsdb_amd.CombineEngine(q, output_format="bu")
    try:
        e.stage_cells(cells)
        key = {n: i for i, n in bcf2text.Header(e.header.decode()).ids.items()}
        for pos, block, narrow, wide in ((20100, bcf2text.BT_INT8, None, "int8"), (20200, bcf2text.BT_INT16, "int8", "int16"), (20300, bcf2text.BT_INT16, "int8", "int16"),
                                         (20400, bcf2text.BT_INT32, "int16", "int32")):
            iv = [(pos - 1, pos - 1)]
            want, records = own_stream_model(e, iv, {"GQ": wide}, 2, offsets)
            assert len(records) == 1 and cm.parse_record(records[0])["fmt"][key["GQ"]] == (block, [[gq[pos][0]], [gq[pos][1]]])
            got = engine_columns(e, iv, {"GQ": wide})
            same(got[0], want)
            assert got[0]["GQ"][0, :, 0].tolist() == list(gq[pos])
            if narrow:
                with pytest.raises(cm.ColumnsError) as m:
                    cm.columns_from_records(e.header.decode(), records, 2, {"GQ": narrow}, offsets)
                assert (m.value.kind, m.value.field, m.value.pos) == ("range", "GQ", pos)
                with pytest.raises(exc, match=r"field GQ .*%s.*pos %d\)" % (narrow, pos)):
                    engine_columns(e, iv, {"GQ": narrow})
    finally:
        e.close()


# ---- 4. lifetime and refusals -----------------------------------------------------------------------------------------------------------------
def _t0(output_format="bu", **kw):
    import genomicsdb_amd
    case = [c for c in CASES if c[0] == "t0_1_2_vcf_at_0"][0]
    cells = helpers.cells_for(case[1], case[2])
    q, _ = helpers.query_json(case[1], case[2], case[3], case[5])
    e = genomicsdb_amd.CombineEngine(q, output_format=output_format, **kw)
    e.stage_cells(cells)
    return e, q


def test_a_clone_outlives_the_page():
    e, q = _t0()
    try:
        fields = {"GT": "int8", "DP": "int32", "PL": "int32"}
        want, records = own_stream_model(e, [(0, 10**9)], fields, 3, offsets_of(q))
        small = max(len(r) for r in records) + 1
        kept = []
        for page in e.record_tensors(0, 10**9, fields=fields, arena_bytes=small):
            kept.append({k: v.clone() for k, v in page.items()})
        assert len(kept) >= 3
        same(cm.pad_and_concatenate([to_numpy(p) for p in kept]), want)
    finally:
        e.close()


def test_refusals_name_what_they_refuse():
    import ctypes
    import genomicsdb_amd
    from genomicsdb_amd import _lib
    exc = genomicsdb_amd.api.GenomicsDBException
    e, _ = _t0(output_format="")
    with pytest.raises(exc, match='output format is "".*"bu"'):
        next(e.record_tensors(fields={"GT": "int8"}))
    e.close()
    e, _ = _t0(use_missing_values_only_not_vector_end=True)
    with pytest.raises(exc, match="use_missing_values_only_not_vector_end"):
        next(e.record_tensors(fields={"GT": "int8"}))
    e.close()
    e, _ = _t0()
    try:
        for fields, words in (({"PGT": None}, "PGT is a string field"), ({"NOPE": "int32"}, "NOPE is neither a FORMAT nor an INFO id"), ({"ID": None}, "ID is a column of strings"),
                              ({"FILTER": None}, "FILTER is a column of strings"), ({"DP": "float32"}, "field DP holds integers"), ({"BaseQRankSum": "int8"}, "field BaseQRankSum holds floats")):
            with pytest.raises(exc, match=words):
                next(e.record_tensors(fields=fields))
        # no page: nothing asked for yet, and an interval that is exhausted
        L = _lib.lib()
        req = (_lib.ColumnRequest * 1)()
        req[0].name, req[0].dtype, req[0].width = b"GT", 1, 0
        assert L.gdbamd_engine_columns_select(e._e, req, 1) == 0
        cols, n, st = (_lib.Column * 16)(), ctypes.c_int(), _lib.ColumnsStats()
        assert L.gdbamd_engine_page_columns(e._e, cols, 16, ctypes.byref(n), ctypes.byref(st)) == -1 and "there is no page" in _lib.last_error()
        assert len(list(e.pages(0, 10**9))) >= 1
        assert L.gdbamd_engine_page_columns(e._e, cols, 16, ctypes.byref(n), ctypes.byref(st)) == -1 and "there is no page" in _lib.last_error()
    finally:
        e.close()


def test_value_errors_name_field_and_pos():
    import genomicsdb_amd
    exc = genomicsdb_amd.api.GenomicsDBException
    e, q = _t0()
    try:
        fields = {"PL": "int32", "DP": "int32", "GQ": "int32"}
        want, _ = own_stream_model(e, [(0, 10**9)], fields, 3, offsets_of(q))
        # a width below a record's L: the first record whose PL is longer than one element
        assert want["PL"].shape[2] > 1
        longer = (want["PL"][:, :, 1] != cm.VEND["int32"]).any(axis=1)
        pos = int(want["pos"][np.argmax(longer)])
        with pytest.raises(cm.ColumnsError) as m:
            cm.columns_from_records(e.header.decode(), own_stream_model(e, [(0, 10**9)], {}, 3, offsets_of(q))[1], 3, {"PL": ("int32", 1)}, offsets_of(q))
        assert (m.value.field, m.value.pos) == ("PL", pos)
        with pytest.raises(exc, match=r"field PL .*width 1 .*pos %d\)" % pos):
            list(e.record_tensors(0, 10**9, fields={"DP": "int32", "PL": ("int32", 1)}))
        # int8 with a value above 127: the first record that has one
        big = {f: ((want[f] > 127).any(axis=(1, 2))) for f in ("PL", "GQ", "DP")}
        f = [f for f in ("PL", "GQ", "DP") if big[f].any()][0]
        pos = int(want["pos"][np.argmax(big[f])])
        with pytest.raises(exc, match=r"field %s .*int8.*pos %d\)" % (f, pos)):
            list(e.record_tensors(0, 10**9, fields={"GT": "int8", f: "int8"}))
    finally:
        e.close()
