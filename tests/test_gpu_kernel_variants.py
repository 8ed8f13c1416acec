"""Byte parity of every knob-selected sizing and page-assembly kernel of gdb_pipeline.hip (and of the non-default BGZF kernels) on
the small shapes of variant_shapes.py.  Which kernel a run takes depends on environment knobs and on the interval
(prepare_interval, begin_page, launch_assemble_size), so every case asserts four things: the oracle's bytes, the record count,
IntervalStats.page_kernel - the decimal digits S K W C II the launch sites leave - and all of that for two pagings: pages of 1 MiB
(several pages of a few hundred records) and arena_bytes = 1 (pages of the largest record's size: grids of fewer than 8 workgroups,
the `per == 0` branch of xcd_aware_unit).

  S sizing kernel: 0 k_assemble_size, 1 k_assemble_size3<8>, 2 k_assemble_size3<16>, 3 k_size2, 4 k_assemble_size_ev
  K page kernel:   1 k_assemble_write, 2 k_write2, 3 k_write3, 4 k_assemble_write_ev, 5 BCF2 kernels
  W wavefronts per workgroup, C COOP_U (0: none), II LDS image in KiB

The expected code stands next to every case, and is checked against variant_shapes.expected_code - the tests' own copy of the
dispatch - so the two cannot drift apart.  Instantiations, ticked off against begin_page / launch_assemble_size:
  k_assemble_write <1,4096> 111204  <1,8192> 111208  <2,4096> 112204  <2,8192> 112208  <4,4096> 114204  <4,6144> 114206  <4,8192> 114208
                   <1,8192,4> 111408
  k_write2         <1,4096> 321004  <1,6144> 321006  <1,8192> 321008  <4,4096> 324004  <4,8192> 324008
  k_write3         <1,4096> 331004  <1,8192> 331008
  k_assemble_write_ev <1> 441008  <4> 444008 (sized by k_assemble_size_ev: S = 4)
  BCF2 kernels     S51000 (an engine in BCF2 mode; the stream hides the statistics)
  k_assemble_size 0xxxxx (GDBAMD_SIZE3=0, GDBAMD_RUN=70000)   k_assemble_size3<8> 1xxxxx   <16> 2xxxxx   k_size2 3xxxxx

The knobs that are read once per process (GDBAMD_RES_LAYOUT, _SLOT_REGROUP, _SITE_ORDER, GDBAMD_BGZF_BLOCK, _WAVES, _TEXT) run in
fresh child processes (tests/tools/variant_child.py), one after another; the parent judges what they wrote.  After a child that
ended by a signal or at its time limit no further child is started."""
import gzip
import json
import os
import subprocess
import sys

import pytest

import helpers
import variant_shapes as vs
from golden_cases import CASES

pytestmark = pytest.mark.gpu

KNOBS = ("ASM_PATH", "MAX_TYPES", "RESOLVED_MB", "RES_COMPACT", "ORDER_BLOCK_LOG2", "WRITE_WAVES", "WRITE_IMAGE_KB", "SIZE3", "SIZE3_CHECK",
         "RUN", "RUN_W", "RUN_W2", "RUN_F", "EVENTS", "EV_RUN", "COOP_UNROLL", "XCD_AWARE", "SLOT_STRIP")
PROCESS_KNOBS = ("RES_LAYOUT", "SLOT_REGROUP", "SITE_ORDER", "BGZF_BLOCK", "BGZF_WAVES", "BGZF_TEXT")
MIB, ONE_PAGE = 1 << 20, 1 << 30


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


class _Engines:
    """one CombineEngine per shape, made when a test first asks for it (the knobs of the in-process tests are read per interval)"""

    def __init__(self, gdb, tmpdir):
        self.gdb, self.tmpdir, self.made = gdb, tmpdir, {}

    def get(self, name):
        if name not in self.made:
            shape = vs.build(name, self.tmpdir)
            eng = self.gdb.CombineEngine(shape.query)
            eng.stage_cells(shape.cells)
            eng.set_reference(shape.begin, vs.reference_bases(shape.begin, shape.end))
            self.made[name] = (shape, eng)
        return self.made[name]

    def close(self):
        for _, eng in self.made.values():
            eng.close()


@pytest.fixture(scope="module")
def engines(gdb, tmp_path_factory):
    e = _Engines(gdb, tmp_path_factory.mktemp("kernel_variants"))
    yield e
    e.close()


def _env(**knobs):
    return {"GDBAMD_" + k: str(v) for k, v in knobs.items()}


def _check(engines, monkeypatch, name, knobs, want_code, arenas=(MIB, 1), untabled=False, entry_bytes=None):
    """one case: shape `name` under `knobs` on every paging of `arenas`.  want_code: the code of every paging, or {arena: code}"""
    shape, eng = engines.get(name)
    for k in KNOBS:
        monkeypatch.delenv("GDBAMD_" + k, raising=False)
    env = _env(**knobs)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for arena in arenas:
        what = (name, knobs, arena)
        code = want_code[arena] if isinstance(want_code, dict) else want_code
        assert vs.expected_code(shape, env, arena, untabled=untabled) == code, ("the test's own tables disagree", what)
        got, st = eng.run_interval(shape.begin, shape.end, arena_bytes=arena)
        assert st.page_kernel == code, (what, st.page_kernel)
        assert st.num_records == shape.nrec, what
        assert got == shape.want, what
        assert st.pages == len(vs.page_ranges(vs.record_bytes(shape.want), arena, _event_block(shape, env, arena))), what
        if entry_bytes is not None:
            assert st.resolved_entry_bytes == entry_bytes, what


def _event_block(shape, env, arena):
    """the order block pages are cut back to, when the change-list path is in use"""
    code = vs.expected_code(shape, env, ONE_PAGE)
    return 1 << int(env.get("GDBAMD_ORDER_BLOCK_LOG2", "12")) if code // 100000 == vs.SIZE_EVENTS else None


# ---- k_assemble_write -------------------------------------------------------------------------------------------------------------
#                 (GDBAMD_WRITE_WAVES, GDBAMD_WRITE_IMAGE_KB) -> code; with 1 or 2 wavefronts an image of 6 selects the 8192 kernel
ASSEMBLE_WRITE = {(1, 4): 111204, (1, 6): 111208, (1, 8): 111208,
                  (2, 4): 112204, (2, 6): 112208, (2, 8): 112208,
                  (4, 4): 114204, (4, 6): 114206, (4, 8): 114208}


@pytest.mark.parametrize("name", ["plain", "mid", "wide"])
def test_assemble_write_every_workgroup_and_image_size(engines, monkeypatch, name):
    """all seven <W, L> instantiations; mid and wide have chunks over every image size (another number of LDS passes for 4, 6 and 8 KiB);
    wide's entries over 255 bytes force the 8-byte matrix, plain and mid keep the compact one"""
    for (ww, kb), code in ASSEMBLE_WRITE.items():
        _check(engines, monkeypatch, name, dict(WRITE_WAVES=ww, WRITE_IMAGE_KB=kb), code, entry_bytes=8 if name == "wide" else 5)
    _check(engines, monkeypatch, name, {}, 111204, entry_bytes=8 if name == "wide" else 5)     # no knob at all: <1, 4096> by the average chunk


def test_assemble_write_matrix_layouts_on_mid(engines, monkeypatch):
    """compact and wide matrix, for the whole interval and resolved page by page (GDBAMD_RESOLVED_MB=0: the sizing kernel runs again per
    page, with the page kernel's run length)"""
    for (ww, kb), code in ASSEMBLE_WRITE.items():
        if kb == 6 and ww != 4:
            continue
        for compact in (0, 1):
            _check(engines, monkeypatch, "mid", dict(WRITE_WAVES=ww, WRITE_IMAGE_KB=kb, RES_COMPACT=compact), code, entry_bytes=5 if compact else 8)
            _check(engines, monkeypatch, "mid", dict(WRITE_WAVES=ww, WRITE_IMAGE_KB=kb, RES_COMPACT=compact, RESOLVED_MB=0), code, entry_bytes=5 if compact else 8)


def test_assemble_write_long_entries(engines, monkeypatch):
    """long: entries over 512 bytes are copied pool -> page by the whole wavefront, 436 of them are larger than a 4 KiB image.  With one
    wavefront per workgroup the host picks <1, 8192, 4> whatever image was asked for; GDBAMD_COOP_UNROLL=0 keeps COOP_U = 2"""
    for kb in (4, 6, 8):
        _check(engines, monkeypatch, "long", dict(WRITE_WAVES=1, WRITE_IMAGE_KB=kb), 111408, entry_bytes=8)
    _check(engines, monkeypatch, "long", {}, 111408, entry_bytes=8)
    _check(engines, monkeypatch, "long", dict(COOP_UNROLL=0), 111204, entry_bytes=8)
    _check(engines, monkeypatch, "long", dict(COOP_UNROLL=0, WRITE_IMAGE_KB=4), 111204, entry_bytes=8)
    _check(engines, monkeypatch, "long", dict(COOP_UNROLL=0, WRITE_IMAGE_KB=8), 111208, entry_bytes=8)
    _check(engines, monkeypatch, "long", dict(COOP_UNROLL=0, WRITE_IMAGE_KB=8, RESOLVED_MB=0), 111208, entry_bytes=8)
    for (ww, kb), code in ASSEMBLE_WRITE.items():
        if ww > 1:
            _check(engines, monkeypatch, "long", dict(WRITE_WAVES=ww, WRITE_IMAGE_KB=kb), code, entry_bytes=8)
    _check(engines, monkeypatch, "long", dict(WRITE_WAVES=4, WRITE_IMAGE_KB=6, RESOLVED_MB=0), 114206, entry_bytes=8)


def test_assemble_write_without_xcd_aware_numbering(engines, monkeypatch):
    for name in ("mid", "long"):
        _check(engines, monkeypatch, name, dict(XCD_AWARE=0, WRITE_WAVES=1, WRITE_IMAGE_KB=8, COOP_UNROLL=0), 111208)
        _check(engines, monkeypatch, name, dict(XCD_AWARE=0, WRITE_WAVES=2, WRITE_IMAGE_KB=4), 112204)
        _check(engines, monkeypatch, name, dict(XCD_AWARE=0, WRITE_WAVES=4, WRITE_IMAGE_KB=6), 114206)
    _check(engines, monkeypatch, "long", dict(XCD_AWARE=0), 111408)


# ---- k_write2, k_write3, k_fill2 --------------------------------------------------------------------------------------------------
WRITE2 = {(1, 4): 321004, (1, 6): 321006, (1, 8): 321008, (4, 4): 324004, (4, 6): 324008, (4, 8): 324008}
WRITE3 = {4: 331004, 6: 331008, 8: 331008}


@pytest.mark.parametrize("name", ["plain", "mid", "long"])
def test_matrix_free_page_kernels(engines, monkeypatch, name):
    """GDBAMD_ASM_PATH=1: the five k_write2 instantiations; 3: both of k_write3; no matrix (resolved_entry_bytes 0); k_size2 sizes"""
    for (ww, kb), code in WRITE2.items():
        _check(engines, monkeypatch, name, dict(ASM_PATH=1, WRITE_WAVES=ww, WRITE_IMAGE_KB=kb), code, entry_bytes=0)
    _check(engines, monkeypatch, name, dict(ASM_PATH=1, WRITE_WAVES=4, WRITE_IMAGE_KB=8, XCD_AWARE=0), 324008, entry_bytes=0)
    for kb, code in WRITE3.items():
        _check(engines, monkeypatch, name, dict(ASM_PATH=3, WRITE_IMAGE_KB=kb), code, entry_bytes=0)
    _check(engines, monkeypatch, name, dict(ASM_PATH=3, WRITE_WAVES=4), 331004, entry_bytes=0)       # (k_write3 has one wavefront per workgroup only)
    _check(engines, monkeypatch, name, dict(ASM_PATH=3, XCD_AWARE=0), 331004, entry_bytes=0)


@pytest.mark.parametrize("name", ["plain", "mid", "long"])
def test_path_3_with_untabled_records_falls_back_to_the_default_kernels(engines, monkeypatch, name):
    """GDBAMD_MAX_TYPES=2: records of the other types have a slot per (record, sample), which the piece lists do not carry: path 0 takes over"""
    code = 111408 if name == "long" else 111204
    _check(engines, monkeypatch, name, dict(ASM_PATH=3, MAX_TYPES=2), code, untabled=True, entry_bytes=8 if name == "long" else 5)
    _check(engines, monkeypatch, name, dict(ASM_PATH=3, MAX_TYPES=0, WRITE_WAVES=4), 114204, untabled=True, entry_bytes=8 if name == "long" else 5)


@pytest.mark.parametrize("name", ["plain", "mid", "long"])
def test_piece_walker_matrix_at_every_fill_run_length(engines, monkeypatch, name):
    """GDBAMD_ASM_PATH=2: k_size2 + k_fill2 fill the matrix k_assemble_write reads, whole and page by page"""
    code = 311408 if name == "long" else 311204
    for frun in (1, 64, 300):
        _check(engines, monkeypatch, name, dict(ASM_PATH=2, RUN_F=frun), code, entry_bytes=8)
        _check(engines, monkeypatch, name, dict(ASM_PATH=2, RUN_F=frun, RESOLVED_MB=0), code, entry_bytes=8)
    _check(engines, monkeypatch, name, dict(ASM_PATH=2, RUN_F=300, WRITE_WAVES=4, WRITE_IMAGE_KB=6), 314206, entry_bytes=8)


# ---- run lengths ------------------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (1, 5, 64, 65, 200)        # 65 and 200: the 64-record batch loop of the page kernels runs more than once, with a short last batch


@pytest.mark.parametrize("name", ["mid", "long"])
def test_page_run_lengths(engines, monkeypatch, name):
    long_ = name == "long"
    for run in RUN_LENGTHS:
        _check(engines, monkeypatch, name, dict(RUN_W=run), 111408 if long_ else 111204)
        _check(engines, monkeypatch, name, dict(RUN_W=run, WRITE_WAVES=4, WRITE_IMAGE_KB=8), 114208)
        _check(engines, monkeypatch, name, dict(RUN_W=run, WRITE_WAVES=2, RESOLVED_MB=0), 112204)          # (the per-page sizing takes the same run length)
        _check(engines, monkeypatch, name, dict(RUN_W2=run, ASM_PATH=1), 321004)
        _check(engines, monkeypatch, name, dict(RUN_W2=run, ASM_PATH=1, WRITE_WAVES=4, WRITE_IMAGE_KB=8), 324008)
        _check(engines, monkeypatch, name, dict(RUN_W2=run, ASM_PATH=3), 331004)


@pytest.mark.parametrize("name", ["mid", "long"])
def test_sizing_run_lengths(engines, monkeypatch, name):
    """GDBAMD_RUN: records one wavefront of the sizing pass takes in a row; more than 65 536 fall back to k_assemble_size (S = 0)"""
    tail = 11408 if name == "long" else 11204
    for run in (1, 5, 64, 1000, 70000):
        big = run > 65536
        _check(engines, monkeypatch, name, dict(RUN=run), (0 if big else 100000) + tail)
        _check(engines, monkeypatch, name, dict(RUN=run, SIZE3=16), (0 if big else 200000) + tail)
        _check(engines, monkeypatch, name, dict(RUN=run, SIZE3=0), tail)
        _check(engines, monkeypatch, name, dict(RUN=run, RESOLVED_MB=0), (0 if big else 100000) + tail)


# ---- sizing kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "mid", "wide", "long"])
def test_every_sizing_kernel(engines, monkeypatch, name):
    """k_assemble_size, k_assemble_size3<8> and <16>; GDBAMD_SIZE3_CHECK=1 is the product's own word-for-word comparison of the piece-wise
    kernels with k_assemble_size (sizes and the wide matrix): it raises on a difference"""
    tail = 11408 if name == "long" else 11204
    wide = name in ("wide", "long")
    for size3, s in ((0, 0), (8, 1), (16, 2)):
        _check(engines, monkeypatch, name, dict(SIZE3=size3), s * 100000 + tail, entry_bytes=8 if wide else 5)
        _check(engines, monkeypatch, name, dict(SIZE3=size3, RES_COMPACT=0), s * 100000 + tail, entry_bytes=8)
        _check(engines, monkeypatch, name, dict(SIZE3=size3, RESOLVED_MB=0), s * 100000 + tail, entry_bytes=8 if wide else 5)
    for size3, s in ((8, 1), (16, 2)):
        _check(engines, monkeypatch, name, dict(SIZE3=size3, SIZE3_CHECK=1), s * 100000 + tail, entry_bytes=8)
        _check(engines, monkeypatch, name, dict(SIZE3=size3, SIZE3_CHECK=1, RESOLVED_MB=0), s * 100000 + tail, entry_bytes=8)


# ---- change-list path -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "mid", "long"])
def test_change_list_kernels(engines, monkeypatch, name):
    """GDBAMD_EVENTS=1: k_assemble_size_ev leaves the changes of every (run, chunk), k_assemble_write_ev<1> / <4> replay them.  A run must
    divide the order block (2^GDBAMD_ORDER_BLOCK_LOG2), or the interval takes the default kernels (a run of 64 with blocks of 32).  One
    page over the interval always reads 44W008; a page that does not start and end on an order-block boundary falls back to
    k_assemble_write, so the code of a paged run is the one of its last page (the tests' model of the paging says which).  Every record
    of `long` has entries over 512 bytes: the event kernel's own whole-wavefront copy (v_alignbyte)"""
    shape, _ = engines.get(name)
    fallback_w = {1: 111408 if name == "long" else 111204, 4: 114204}
    for log2 in (5, 6, 12):
        for evrun in (1, 32, 64):
            for ww in (1, 4):
                knobs = dict(EVENTS=1, WRITE_WAVES=ww, EV_RUN=evrun, ORDER_BLOCK_LOG2=log2)
                usable = (1 << log2) % evrun == 0
                one_page = (441008 if ww == 1 else 444008) if usable else fallback_w[ww]
                codes = {ONE_PAGE: one_page}
                for arena in (MIB, 1):
                    codes[arena] = vs.expected_code(shape, _env(**knobs), arena)
                    assert codes[arena] in (one_page, 400000 + fallback_w[ww] % 100000), (knobs, arena, codes)
                _check(engines, monkeypatch, name, knobs, codes, arenas=(ONE_PAGE, MIB, 1), entry_bytes=0)


@pytest.mark.parametrize("name", ["plain", "long"])
def test_change_list_fallbacks(engines, monkeypatch, name):
    write = 11408 if name == "long" else 11204
    # a run length that does not divide the order block: the default sizing and page kernels
    _check(engines, monkeypatch, name, dict(EVENTS=1, EV_RUN=7), 100000 + write, arenas=(ONE_PAGE, MIB, 1), entry_bytes=0)
    # no room for the change list: the same
    _check(engines, monkeypatch, name, dict(EVENTS=1, RESOLVED_MB=0), 100000 + write, arenas=(ONE_PAGE, MIB, 1), entry_bytes=0)
    # pages that are not aligned to the order block of 4096 records: sized by k_assemble_size_ev, resolved per page, written by k_assemble_write
    _check(engines, monkeypatch, name, dict(EVENTS=1), {ONE_PAGE: 441008, MIB: 400000 + write, 1: 400000 + write}, arenas=(ONE_PAGE, MIB, 1), entry_bytes=0)
    _check(engines, monkeypatch, name, dict(EVENTS=1, WRITE_WAVES=4, WRITE_IMAGE_KB=6), {ONE_PAGE: 444008, MIB: 414206, 1: 414206}, arenas=(ONE_PAGE, MIB, 1), entry_bytes=0)


# ---- entry-table strips -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mid", "long"])
def test_entry_table_strips(engines, monkeypatch, name):
    """GDBAMD_SLOT_STRIP: the 128- and 256-byte LDS strips of the k_slots kernels, with every record type tabled, two of them, and none"""
    for strip in (128, 256):
        _check(engines, monkeypatch, name, dict(SLOT_STRIP=strip, WRITE_WAVES=4), 114204)
        for max_types in (0, 2):
            _check(engines, monkeypatch, name, dict(SLOT_STRIP=strip, MAX_TYPES=max_types, WRITE_WAVES=4), 114204, untabled=True)
            _check(engines, monkeypatch, name, dict(SLOT_STRIP=strip, MAX_TYPES=max_types, WRITE_WAVES=4, ASM_PATH=1), 324004, untabled=True)


# ---- BCF2 -------------------------------------------------------------------------------------------------------------------------
def test_bcf2_pages_after_every_sizing_kernel(gdb, monkeypatch):
    """the BCF2 kernels read the matrix the sizing kernel left (the statistics are not reachable through the stream: the decoded text decides)"""
    _, callsets, vid, ov, golden, mode = [c for c in CASES if c[0] == "t0_1_2_vcf_at_0"][0]
    cells = helpers.cells_for(callsets, vid)
    q, _ = helpers.query_json(callsets, vid, ov, mode)
    for k in KNOBS:
        monkeypatch.delenv("GDBAMD_" + k, raising=False)
    monkeypatch.setenv("GDBAMD_WRITE_WAVES", "4")
    for size3 in ("0", "8", "16"):
        monkeypatch.setenv("GDBAMD_SIZE3", size3)
        s = gdb.GenomicsDBQueryStream(query_json=q, cells=cells, buffer_capacity=1 << 20, is_bcf=True)
        raw = s.read()
        s.close()
        assert raw[:5] == b"BCF\x02\x02" and helpers.bcf_stream_to_text(raw) == helpers.golden_text(golden), size3


def test_bcf2_kernels_report_their_sizing_kernel_on_mid(gdb, engines, monkeypatch):
    """an engine in BCF2 mode gives the statistics the stream hides: K = 5 behind every sizing kernel (odd GDBAMD_ASM_PATH values have no
    matrix to read, so they become path 2: k_size2 + k_fill2), whole and paged; the records decode to the oracle's text"""
    import struct
    import bcf2text
    shape, text_engine = engines.get("mid")
    header = bcf2text.Header(text_engine.header.decode())
    eb = gdb.CombineEngine(shape.query, is_bcf=True)
    eb.stage_cells(shape.cells)
    eb.set_reference(shape.begin, vs.reference_bases(shape.begin, shape.end))
    first = None
    #             knobs -> code
    for knobs, code in ((dict(), 151000), (dict(SIZE3=0), 51000), (dict(SIZE3=16), 251000), (dict(RUN=70000), 51000), (dict(RES_COMPACT=0), 151000),
                        (dict(ASM_PATH=1), 351000), (dict(ASM_PATH=2), 351000), (dict(ASM_PATH=3, RUN_F=64), 351000), (dict(EVENTS=1), 151000)):
        for k in KNOBS:
            monkeypatch.delenv("GDBAMD_" + k, raising=False)
        for k, v in _env(**knobs).items():
            monkeypatch.setenv(k, v)
        for arena in (ONE_PAGE, 1 << 18, 1):
            assert vs.expected_code(shape, _env(**knobs), arena, bcf=True) == code, ("the test's own tables disagree", knobs)
            body, st = eb.run_interval(shape.begin, shape.end, arena_bytes=arena)
            assert st.page_kernel == code, (knobs, arena, st.page_kernel)
            assert st.num_records == shape.nrec and (st.pages == 1 if arena == ONE_PAGE else st.pages >= 2), (knobs, arena, st.pages)
            if first is None:
                at, lines = 0, []
                while at < len(body):
                    l_shared, l_indiv = struct.unpack_from("<II", body, at)
                    lines.append(bcf2text.record_to_text(header, body[at:at + 8 + l_shared + l_indiv], helpers.format_float))
                    at += 8 + l_shared + l_indiv
                assert ("\n".join(lines) + "\n").encode() == shape.want
                first = body
            assert body == first, (knobs, arena)
    eb.close()


# ---- knobs read once per process: fresh children ----------------------------------------------------------------------------------
CHILD = os.path.join(helpers.ROOT, "tests", "tools", "variant_child.py")
_child_lost = []          # why no further child may start: one ended by a signal or at its time limit (the card may have faulted)


def _run_child(kind, outdir, what, knobs, timeout):
    assert not _child_lost, "no child is started after one that was lost: " + _child_lost[0]
    env = {k: v for k, v in os.environ.items() if not (k.startswith("GDBAMD_") and k[7:] in KNOBS + PROCESS_KNOBS)}
    env.update(_env(**knobs))
    try:
        r = subprocess.run([sys.executable, CHILD, kind, str(outdir), what], env=env, capture_output=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _child_lost.append("%s %s %r ran into its time limit of %d s" % (kind, what, knobs, timeout))
        raise AssertionError(_child_lost[0])
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _child_lost.append("%s %s %r ended with status %d: %s" % (kind, what, knobs, r.returncode, r.stderr.decode(errors="replace")[-2000:]))
        raise AssertionError(_child_lost[0])
    assert r.returncode == 0 and os.path.exists(os.path.join(str(outdir), "done")), r.stderr.decode(errors="replace")[-4000:]


#                 knob of the child                runs inside it: per-interval knobs -> code
PIPELINE_CHILDREN = {
    "RES_LAYOUT=1": (dict(RES_LAYOUT=1), [({}, 111204), (dict(RESOLVED_MB=0), 111204), (dict(RES_COMPACT=0), 111204), (dict(WRITE_WAVES=4, WRITE_IMAGE_KB=6), 114206),
                                          (dict(WRITE_WAVES=2, WRITE_IMAGE_KB=8, RESOLVED_MB=0, RES_COMPACT=0), 112208), (dict(SIZE3=0), 11204), (dict(SIZE3=16, RESOLVED_MB=0), 211204),
                                          (dict(SIZE3=16, SIZE3_CHECK=1), 211204), (dict(ASM_PATH=2), 311204)]),
    "SLOT_REGROUP=0": (dict(SLOT_REGROUP=0), [({}, 111204), (dict(ASM_PATH=1), 321004), (dict(SLOT_STRIP=256, WRITE_WAVES=4), 114204)]),
    "SITE_ORDER=0": (dict(SITE_ORDER=0), [({}, 111204), (dict(ASM_PATH=3), 331004)]),
}


@pytest.mark.parametrize("child", list(PIPELINE_CHILDREN))
def test_pipeline_knobs_read_once_per_process(engines, tmp_path, child):
    """the chunk-major matrix (GDBAMD_RES_LAYOUT=1: sizing kernels write it, k_assemble_write reads it, whole and per page), the entry
    table without regrouped slots, the site kernels in record order: `mid`, two pagings per run, judged here against the oracle"""
    shape, _ = engines.get("mid")
    process_knobs, cases = PIPELINE_CHILDREN[child]
    runs = [{"arena_bytes": arena, "env": _env(**knobs)} for knobs, _ in cases for arena in (MIB, 1)]
    (tmp_path / "runs.json").write_text(json.dumps(runs))
    _run_child("pipeline", tmp_path, "mid", process_knobs, timeout=180)
    results = json.loads((tmp_path / "results.json").read_text())
    assert len(results) == len(runs)
    for i, (run, res) in enumerate(zip(runs, results)):
        code = cases[i // 2][1]
        assert vs.expected_code(shape, run["env"], run["arena_bytes"]) == code, ("the test's own tables disagree", run)
        assert res["page_kernel"] == code, (run, res)
        assert res["num_records"] == shape.nrec, (run, res)
        assert (tmp_path / ("run%d.bin" % i)).read_bytes() == shape.want, run
        assert res["pages"] == len(vs.page_ranges(vs.record_bytes(shape.want), run["arena_bytes"])), (run, res)


BGZF_CHILDREN = {"BLOCK=4096": (dict(BGZF_BLOCK=4096), 4096), "BLOCK=6144": (dict(BGZF_BLOCK=6144), 6144), "BLOCK=16384": (dict(BGZF_BLOCK=16384), 16384),
                 "WAVES=1": (dict(BGZF_WAVES=1), 8192), "TEXT=0": (dict(BGZF_TEXT=0), 8192)}


@pytest.mark.parametrize("child", list(BGZF_CHILDREN))
def test_bgzf_knobs_read_once_per_process(gdb, tmp_path, child):
    """the 4, 6 and 16 KiB blocks with their CRC shift tables, the one-wavefront deflate kernel, the byte-level kernel for text pages: the
    hostile inputs of test_bgzf.py through both entry points, and a golden as a "z" stream.  zlib is the reference (bgzf_blocks checks
    every header field, CRC-32 and ISIZE), the blocks have the length asked for, and the device inflater inverts every output"""
    import test_bgzf
    knobs, block = BGZF_CHILDREN[child]
    _run_child("bgzf", tmp_path, "t0_1_2_vcf_at_0", knobs, timeout=300)
    for prefix, inputs in (("h", test_bgzf.HOSTILE_INPUTS), ("t", test_bgzf.HOSTILE_TEXT_INPUTS)):
        for i, (name, data) in enumerate(inputs.items()):
            for mode in ("bytes", "text"):
                what = (child, name, mode)
                comp = (tmp_path / ("%s%s%d.bgzf" % (prefix, mode, i))).read_bytes()
                blocks = test_bgzf.bgzf_blocks(comp)
                assert b"".join(r for _, r in blocks) == data, what
                assert len(blocks) == (len(data) + block - 1) // block and all(len(r) == block for _, r in blocks[:-1]), what
                if data:
                    assert gdb.bgzf_decompress(comp)[0] == data, what
    _, _, _, _, golden, _ = [c for c in CASES if c[0] == "t0_1_2_vcf_at_0"][0]
    z = (tmp_path / "golden.z").read_bytes()
    want = helpers.golden_text(golden)
    assert z.endswith(test_bgzf.EOF_BLOCK)
    blocks = test_bgzf.bgzf_blocks(z)
    assert blocks[-1][1] == b"" and b"".join(r for _, r in blocks) == want and gzip.decompress(z) == want
    assert gdb.bgzf_decompress(z)[0] == want
