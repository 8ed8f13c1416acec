"""The product's choice of an interval's sizing and page kernels (kernels/gdb_assembly_choice.hpp: the knob reader, choose_sizing,
page_end, choose_page - what prepare_interval and begin_page launch by) against the tests' own copy of the dispatch
(variant_shapes.expected_code / page_ranges), on the CPU: tests/hostsim_dispatch drives the header page by page over the record sizes
of the four shapes of variant_shapes.py.  For every combination of knobs three figures are compared: the number of pages, the
IntervalStats.page_kernel code of the last page, and resolved_entry_bytes by the rule the GPU tests state (0 whenever GDBAMD_EVENTS is
set or the path is matrix-free, 5 on path 0 when no entry exceeds 255 bytes and neither GDBAMD_RES_COMPACT=0 nor GDBAMD_SIZE3_CHECK is
set, else 8).  The knob dictionaries of test_gpu_kernel_variants.py are repeated here with their codes, so that a drift between the two
tables shows without a GPU."""
import ctypes
import itertools
import random

import pytest

import variant_shapes as vs

MIB, ONE_PAGE = 1 << 20, 1 << 30
ARENAS = (ONE_PAGE, MIB, 1)

# every setting of every knob that takes part in the choice (None: unset)
SETTINGS = {
    "ASM_PATH": (None, 0, 1, 2, 3, 7, -1),
    "EVENTS": (None, 0, 1),
    "SIZE3": (None, 0, 5, 8, 16),
    "RUN": (None, 1, 70000),
    "WRITE_WAVES": (None, 1, 2, 4),
    "WRITE_IMAGE_KB": (None, 4, 6, 8),
    "RESOLVED_MB": (None, 0),
    "EV_RUN": (None, 7, 64, 100),
    "ORDER_BLOCK_LOG2": (None, 5, 6),
    "COOP_UNROLL": (None, 0),
    "RES_COMPACT": (None, 0),
    "SIZE3_CHECK": (None, 1),
}
N_SAMPLED = 2500


def _env(**knobs):
    return {"GDBAMD_" + k: str(v) for k, v in knobs.items()}


def singles_and_pairs():
    yield {}
    one = [(k, v) for k, vals in SETTINGS.items() for v in vals if v is not None]
    for k, v in one:
        yield {k: v}
    for (k1, v1), (k2, v2) in itertools.combinations(one, 2):
        if k1 != k2:
            yield {k1: v1, k2: v2}


def sampled():
    rng = random.Random(20241019)
    for _ in range(N_SAMPLED):
        yield {k: v for k, v in ((k, rng.choice(vals)) for k, vals in SETTINGS.items()) if v is not None}


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    d = tmp_path_factory.mktemp("assembly_choice")
    return {name: vs.build(name, d) for name in vs.SHAPES}


@pytest.fixture(scope="module")
def product():
    """product(shape, env, arena, untabled, bcf) -> (pages, page_kernel of the last page, resolved_entry_bytes) by the header"""
    from genomicsdb_amd import build as b
    L = ctypes.CDLL(b.build_hostsim_dispatch())
    c = ctypes
    L.hostsim_dispatch.restype = None
    L.hostsim_dispatch.argtypes = [c.POINTER(c.c_char_p), c.POINTER(c.c_char_p), c.c_int, c.POINTER(c.c_uint64), c.c_int64, c.c_int32, c.c_int, c.c_int, c.c_int,
                                   c.c_uint64, c.POINTER(c.c_int64)]
    facts = {}

    def run(shape, env, arena, untabled, bcf):
        if shape.name not in facts:
            rec = vs.record_bytes(shape.want)
            over255 = max(max(e) for e in vs.entry_lengths(shape.want)) > 255
            facts[shape.name] = ((c.c_uint64 * len(rec))(*rec), len(rec), int(over255))
        rec, P, over255 = facts[shape.name]
        names = (c.c_char_p * len(env))(*[k.encode() for k in env])
        values = (c.c_char_p * len(env))(*[v.encode() for v in env.values()])
        out = (c.c_int64 * 11)()
        L.hostsim_dispatch(names, values, len(env), rec, P, shape.N, int(bcf), int(untabled), over255, arena, out)
        return tuple(out) if details else tuple(out[:3])
    details = False

    def run_details(*args):
        nonlocal details
        details = True
        try:
            return run(*args)
        finally:
            details = False
    run.details = run_details
    return run


@pytest.fixture(scope="module")
def model(shapes):
    """model(shape, env, arena, untabled, bcf) -> the same three figures by the tests' copy of the dispatch"""
    pages = {}             # the greedy paging is the slow part of the model: once per (shape, arena, order block)
    over255 = {n: max(max(e) for e in vs.entry_lengths(s.want)) > 255 for n, s in shapes.items()}

    def run(shape, env, arena, untabled, bcf):
        def knob(name, default):
            v = env.get("GDBAMD_" + name, "")
            return int(v) if v != "" else default
        code = vs.expected_code(shape, env, arena, untabled=untabled, bcf=bcf)
        # pages are cut back to order blocks when the change-list path is in use (as _event_block of test_gpu_kernel_variants.py finds out)
        events_used = (code if arena == ONE_PAGE else vs.expected_code(shape, env, ONE_PAGE, untabled=untabled, bcf=bcf)) // 100000 == vs.SIZE_EVENTS
        block = 1 << knob("ORDER_BLOCK_LOG2", 12) if events_used else None
        key = (shape.name, arena, block)
        if key not in pages:
            pages[key] = len(vs.page_ranges(vs.record_bytes(shape.want), arena, block))
        events_on = knob("EVENTS", 0) != 0
        path = 0 if events_on else min(3, max(0, knob("ASM_PATH", 0)))
        if bcf and path & 1:
            path = 2
        if path == 3 and untabled:
            path = 0
        if events_on or path in (1, 3):
            entry_bytes = 0
        elif path == 0 and not over255[shape.name] and knob("RES_COMPACT", 1) != 0 and knob("SIZE3_CHECK", 0) == 0:
            entry_bytes = 5
        else:
            entry_bytes = 8
        return pages[key], code, entry_bytes
    return run


def _compare(shapes, product, model, knob_sets, names=tuple(vs.SHAPES)):
    n = 0
    for knobs in knob_sets:
        env = _env(**knobs)
        for name in names:
            for bcf in (False, True):
                for untabled in (False, True):
                    for arena in ARENAS:
                        got, want = product(shapes[name], env, arena, untabled, bcf), model(shapes[name], env, arena, untabled, bcf)
                        assert got == want, ("(pages, page_kernel, resolved_entry_bytes): product %r, tests' copy %r" % (got, want), name, knobs, bcf, untabled, arena)
                        n += 1
    return n


def test_every_knob_setting_alone_and_in_pairs(shapes, product, model):
    assert _compare(shapes, product, model, singles_and_pairs()) > 10000


def test_sampled_full_combinations(shapes, product, model):
    assert _compare(shapes, product, model, sampled()) == N_SAMPLED * len(vs.SHAPES) * 4 * len(ARENAS)


# ---- the cases of test_gpu_kernel_variants.py: shapes, knobs, the code it expects on pages of 1 MiB and 1 byte, untabled ---------------
ASSEMBLE_WRITE = {(1, 4): 111204, (1, 6): 111208, (1, 8): 111208,
                  (2, 4): 112204, (2, 6): 112208, (2, 8): 112208,
                  (4, 4): 114204, (4, 6): 114206, (4, 8): 114208}
WRITE2 = {(1, 4): 321004, (1, 6): 321006, (1, 8): 321008, (4, 4): 324004, (4, 6): 324008, (4, 8): 324008}
WRITE3 = {4: 331004, 6: 331008, 8: 331008}


def gpu_cases():
    """(shape, knobs, code, untabled, entry_bytes or None) of every _check of test_gpu_kernel_variants.py with one code for both pagings"""
    for name in ("plain", "mid", "wide"):              # test_assemble_write_every_workgroup_and_image_size
        for (ww, kb), code in ASSEMBLE_WRITE.items():
            yield name, dict(WRITE_WAVES=ww, WRITE_IMAGE_KB=kb), code, False, 8 if name == "wide" else 5
        yield name, {}, 111204, False, 8 if name == "wide" else 5
    for (ww, kb), code in ASSEMBLE_WRITE.items():      # test_assemble_write_matrix_layouts_on_mid
        if kb == 6 and ww != 4:
            continue
        for compact in (0, 1):
            yield "mid", dict(WRITE_WAVES=ww, WRITE_IMAGE_KB=kb, RES_COMPACT=compact), code, False, 5 if compact else 8
            yield "mid", dict(WRITE_WAVES=ww, WRITE_IMAGE_KB=kb, RES_COMPACT=compact, RESOLVED_MB=0), code, False, 5 if compact else 8
    for kb in (4, 6, 8):                               # test_assemble_write_long_entries
        yield "long", dict(WRITE_WAVES=1, WRITE_IMAGE_KB=kb), 111408, False, 8
    yield "long", {}, 111408, False, 8
    yield "long", dict(COOP_UNROLL=0), 111204, False, 8
    yield "long", dict(COOP_UNROLL=0, WRITE_IMAGE_KB=4), 111204, False, 8
    yield "long", dict(COOP_UNROLL=0, WRITE_IMAGE_KB=8), 111208, False, 8
    yield "long", dict(COOP_UNROLL=0, WRITE_IMAGE_KB=8, RESOLVED_MB=0), 111208, False, 8
    for (ww, kb), code in ASSEMBLE_WRITE.items():
        if ww > 1:
            yield "long", dict(WRITE_WAVES=ww, WRITE_IMAGE_KB=kb), code, False, 8
    yield "long", dict(WRITE_WAVES=4, WRITE_IMAGE_KB=6, RESOLVED_MB=0), 114206, False, 8
    for name in ("mid", "long"):                       # test_assemble_write_without_xcd_aware_numbering
        yield name, dict(XCD_AWARE=0, WRITE_WAVES=1, WRITE_IMAGE_KB=8, COOP_UNROLL=0), 111208, False, None
        yield name, dict(XCD_AWARE=0, WRITE_WAVES=2, WRITE_IMAGE_KB=4), 112204, False, None
        yield name, dict(XCD_AWARE=0, WRITE_WAVES=4, WRITE_IMAGE_KB=6), 114206, False, None
    yield "long", dict(XCD_AWARE=0), 111408, False, None
    for name in ("plain", "mid", "long"):
        for (ww, kb), code in WRITE2.items():          # test_matrix_free_page_kernels
            yield name, dict(ASM_PATH=1, WRITE_WAVES=ww, WRITE_IMAGE_KB=kb), code, False, 0
        yield name, dict(ASM_PATH=1, WRITE_WAVES=4, WRITE_IMAGE_KB=8, XCD_AWARE=0), 324008, False, 0
        for kb, code in WRITE3.items():
            yield name, dict(ASM_PATH=3, WRITE_IMAGE_KB=kb), code, False, 0
        yield name, dict(ASM_PATH=3, WRITE_WAVES=4), 331004, False, 0
        yield name, dict(ASM_PATH=3, XCD_AWARE=0), 331004, False, 0
        long_ = name == "long"                         # test_path_3_with_untabled_records_falls_back_to_the_default_kernels
        yield name, dict(ASM_PATH=3, MAX_TYPES=2), 111408 if long_ else 111204, True, 8 if long_ else 5
        yield name, dict(ASM_PATH=3, MAX_TYPES=0, WRITE_WAVES=4), 114204, True, 8 if long_ else 5
        for frun in (1, 64, 300):                      # test_piece_walker_matrix_at_every_fill_run_length
            yield name, dict(ASM_PATH=2, RUN_F=frun), 311408 if long_ else 311204, False, 8
            yield name, dict(ASM_PATH=2, RUN_F=frun, RESOLVED_MB=0), 311408 if long_ else 311204, False, 8
        yield name, dict(ASM_PATH=2, RUN_F=300, WRITE_WAVES=4, WRITE_IMAGE_KB=6), 314206, False, 8
    for name in ("mid", "long"):
        long_ = name == "long"
        tail = 11408 if long_ else 11204
        for run in (1, 5, 64, 65, 200):                # test_page_run_lengths
            yield name, dict(RUN_W=run), 111408 if long_ else 111204, False, None
            yield name, dict(RUN_W=run, WRITE_WAVES=4, WRITE_IMAGE_KB=8), 114208, False, None
            yield name, dict(RUN_W=run, WRITE_WAVES=2, RESOLVED_MB=0), 112204, False, None
            yield name, dict(RUN_W2=run, ASM_PATH=1), 321004, False, None
            yield name, dict(RUN_W2=run, ASM_PATH=1, WRITE_WAVES=4, WRITE_IMAGE_KB=8), 324008, False, None
            yield name, dict(RUN_W2=run, ASM_PATH=3), 331004, False, None
        for run in (1, 5, 64, 1000, 70000):            # test_sizing_run_lengths
            big = run > 65536
            yield name, dict(RUN=run), (0 if big else 100000) + tail, False, None
            yield name, dict(RUN=run, SIZE3=16), (0 if big else 200000) + tail, False, None
            yield name, dict(RUN=run, SIZE3=0), tail, False, None
            yield name, dict(RUN=run, RESOLVED_MB=0), (0 if big else 100000) + tail, False, None
        for strip in (128, 256):                       # test_entry_table_strips
            yield name, dict(SLOT_STRIP=strip, WRITE_WAVES=4), 114204, False, None
            for max_types in (0, 2):
                yield name, dict(SLOT_STRIP=strip, MAX_TYPES=max_types, WRITE_WAVES=4), 114204, True, None
                yield name, dict(SLOT_STRIP=strip, MAX_TYPES=max_types, WRITE_WAVES=4, ASM_PATH=1), 324004, True, None
    for name in ("plain", "mid", "wide", "long"):      # test_every_sizing_kernel
        tail = 11408 if name == "long" else 11204
        wide = name in ("wide", "long")
        for size3, s in ((0, 0), (8, 1), (16, 2)):
            yield name, dict(SIZE3=size3), s * 100000 + tail, False, 8 if wide else 5
            yield name, dict(SIZE3=size3, RES_COMPACT=0), s * 100000 + tail, False, 8
            yield name, dict(SIZE3=size3, RESOLVED_MB=0), s * 100000 + tail, False, 8 if wide else 5
        for size3, s in ((8, 1), (16, 2)):
            yield name, dict(SIZE3=size3, SIZE3_CHECK=1), s * 100000 + tail, False, 8
            yield name, dict(SIZE3=size3, SIZE3_CHECK=1, RESOLVED_MB=0), s * 100000 + tail, False, 8
    for name in ("plain", "long"):                     # test_change_list_fallbacks (the cases with one code for every paging)
        write = 11408 if name == "long" else 11204
        yield name, dict(EVENTS=1, EV_RUN=7), 100000 + write, False, 0
        yield name, dict(EVENTS=1, RESOLVED_MB=0), 100000 + write, False, 0
    # test_pipeline_knobs_read_once_per_process: what runs inside the children (their own knob does not take part in the code)
    for knobs, code in (({}, 111204), (dict(RESOLVED_MB=0), 111204), (dict(RES_COMPACT=0), 111204), (dict(WRITE_WAVES=4, WRITE_IMAGE_KB=6), 114206),
                        (dict(WRITE_WAVES=2, WRITE_IMAGE_KB=8, RESOLVED_MB=0, RES_COMPACT=0), 112208), (dict(SIZE3=0), 11204), (dict(SIZE3=16, RESOLVED_MB=0), 211204),
                        (dict(SIZE3=16, SIZE3_CHECK=1), 211204), (dict(ASM_PATH=2), 311204), (dict(ASM_PATH=1), 321004), (dict(SLOT_STRIP=256, WRITE_WAVES=4), 114204),
                        (dict(ASM_PATH=3), 331004)):
        for layout in ({}, dict(RES_LAYOUT=1)):
            yield "mid", dict(knobs, **layout), code, False, None


def test_the_cases_of_the_gpu_kernel_variant_tests(shapes, product, model):
    for name, knobs, code, untabled, entry_bytes in gpu_cases():
        for arena in (MIB, 1):
            got = product(shapes[name], _env(**knobs), arena, untabled, False)
            assert got == model(shapes[name], _env(**knobs), arena, untabled, False), (name, knobs, arena)
            assert got[1] == code and (entry_bytes is None or got[2] == entry_bytes), (name, knobs, arena, got)
    # test_change_list_kernels and the paged cases of test_change_list_fallbacks: the code depends on the paging
    for name in ("plain", "mid", "long"):
        fallback_w = {1: 111408 if name == "long" else 111204, 4: 114204}
        for log2, evrun, ww in itertools.product((5, 6, 12), (1, 32, 64), (1, 4)):
            knobs = dict(EVENTS=1, WRITE_WAVES=ww, EV_RUN=evrun, ORDER_BLOCK_LOG2=log2)
            one_page = (441008 if ww == 1 else 444008) if (1 << log2) % evrun == 0 else fallback_w[ww]
            for arena in ARENAS:
                got = product(shapes[name], _env(**knobs), arena, False, False)
                assert got == model(shapes[name], _env(**knobs), arena, False, False), (name, knobs, arena)
                assert got[1] in (one_page, 400000 + fallback_w[ww] % 100000) and (arena != ONE_PAGE or got[1] == one_page) and got[2] == 0, (name, knobs, arena, got)
    for name in ("plain", "long"):
        write = 11408 if name == "long" else 11204
        for knobs, codes in ((dict(EVENTS=1), {ONE_PAGE: 441008, MIB: 400000 + write, 1: 400000 + write}),
                             (dict(EVENTS=1, WRITE_WAVES=4, WRITE_IMAGE_KB=6), {ONE_PAGE: 444008, MIB: 414206, 1: 414206})):
            for arena in ARENAS:
                assert product(shapes[name], _env(**knobs), arena, False, False)[1:] == (codes[arena], 0), (name, knobs, arena)
    # test_bcf2_kernels_report_their_sizing_kernel_on_mid
    for knobs, code in ((dict(), 151000), (dict(SIZE3=0), 51000), (dict(SIZE3=16), 251000), (dict(RUN=70000), 51000), (dict(RES_COMPACT=0), 151000),
                        (dict(ASM_PATH=1), 351000), (dict(ASM_PATH=2), 351000), (dict(ASM_PATH=3, RUN_F=64), 351000), (dict(EVENTS=1), 151000)):
        for arena in (ONE_PAGE, 1 << 18, 1):
            got = product(shapes["mid"], _env(**knobs), arena, False, True)
            assert got == model(shapes["mid"], _env(**knobs), arena, False, True) and got[1] == code, (knobs, arena, got)


def test_the_reader_clamps_and_defaults(product, shapes):
    """what the reader makes of values outside a knob's range, seen through the code: GDBAMD_ASM_PATH 7 is 3 and -1 is 0, GDBAMD_SIZE3=5 is the
    piece-wise kernel in rounds of 8, GDBAMD_EV_RUN=100 is 64 (which divides no order block of 32), an empty string is unset"""
    mid = shapes["mid"]
    def code(**knobs):
        return product(mid, _env(**knobs), ONE_PAGE, False, False)[1]
    assert code(ASM_PATH=7) == code(ASM_PATH=3) == 331004 and code(ASM_PATH=-1) == code() == 111204
    assert code(SIZE3=5) == 111204 and code(SIZE3=0) == 11204 and code(SIZE3=99) == 211204
    assert code(EVENTS=1, EV_RUN=100) == code(EVENTS=1, EV_RUN=64) == 441008 and code(EVENTS=1, EV_RUN=100, ORDER_BLOCK_LOG2=5) == 111204
    assert code(ASM_PATH="", SIZE3="", EVENTS="", WRITE_IMAGE_KB="", RUN="") == 111204


def test_run_lengths_streams_and_matrix_rows(shapes, product):
    """what the code does not show: the page kernel's run length, whether it goes to the forked stream, how a page's records are resolved
    when the matrix is over its budget, the row count a chunk-major matrix is read with, k_fill2's run length, and the reading of
    GDBAMD_RUN_W, _RUN_W2, _RUN_F, _RES_LAYOUT, _XCD_AWARE and _PAGE_PRIORITY - by the rules of begin_page before the choice moved"""
    settings = {"RUN_W": (None, 1, 200, 70000), "RUN_W2": (None, 5), "RUN_F": (None, 0, 64), "RES_LAYOUT": (None, 0, 1), "XCD_AWARE": (None, 0, 1),
                "PAGE_PRIORITY": (None, 0, 1, 2), "ASM_PATH": (None, 1, 2, 3), "EVENTS": (None, 1), "EV_RUN": (None, 16), "RESOLVED_MB": (None, 0), "SIZE3": (None, 0, 16)}
    rng, last_page, recs = random.Random(7), {}, {n: vs.record_bytes(shapes[n].want) for n in ("mid", "long")}
    for _ in range(600):
        knobs = {k: v for k, v in ((k, rng.choice(vals)) for k, vals in settings.items()) if v is not None}
        env = _env(**knobs)
        for name, bcf, arena in itertools.product(("mid", "long"), (False, True), ARENAS):
            shape = shapes[name]
            what = (name, knobs, bcf, arena)
            pages, code, _, run, forks, resolve, res_rows, frun, chunk_major, xcd_aware, priority = product.details(shape, env, arena, False, bcf)
            S, K = code // 100000, code // 10000 % 10
            events_on = "EVENTS" in knobs
            path = 0 if events_on else knobs.get("ASM_PATH", 0)
            path = 2 if bcf and path & 1 else path
            assert frun == max(1, knobs.get("RUN_F", 128)) and xcd_aware == (knobs.get("XCD_AWARE", 1) != 0), what
            assert priority == (knobs["PAGE_PRIORITY"] if knobs.get("PAGE_PRIORITY") in (0, 1) else -1), what
            assert forks == (K in (vs.PAGE_WRITE, vs.PAGE_BCF)), what
            assert chunk_major == (knobs.get("RES_LAYOUT") == 1 and not bcf and path != 2), what
            if K == vs.PAGE_BCF:
                assert (resolve, res_rows) == (-1, 0), what
                continue
            want_run = knobs.get("EV_RUN", 32) if K == vs.PAGE_EVENTS else knobs.get("RUN_W2", 64) if K in (vs.PAGE_WRITE2, vs.PAGE_WRITE3) else knobs.get("RUN_W", 32)
            assert run == want_run, what
            if K != vs.PAGE_WRITE:
                assert (resolve, res_rows) == (-1, 0), what
                continue
            rec = recs[name]
            events_fit = events_on and 4096 % knobs.get("EV_RUN", 32) == 0
            whole = len(rec) * 3 * 64 * 8 <= (knobs.get("RESOLVED_MB", 32 << 10) << 20) and not events_fit
            size3 = knobs.get("SIZE3", 8)
            by_sizing = vs.SIZE_PLAIN if size3 == 0 or want_run > 65536 else vs.SIZE_3X16 if size3 >= 16 else vs.SIZE_3X8
            assert resolve == (-1 if whole else vs.SIZE_PIECES if path == 2 else by_sizing), what
            key = (name, arena, 4096 if S == vs.SIZE_EVENTS else None)
            if key not in last_page:
                last_page[key] = vs.page_ranges(rec, arena, key[2])[-1]
            kp, ke = last_page[key]
            assert res_rows == ((len(rec) if whole else ke - kp) if chunk_major else 0), what
