"""The smallest synthetic inputs at which the knob-selected sizing and page-assembly kernels of gdb_pipeline.hip can go wrong, and the
tests' own copy of the dispatch of prepare_interval / begin_page / launch_assemble_size (the expected IntervalStats.page_kernel code).

A "chunk" is the text of one record's 64-sample group, tabs included: what one wavefront of a page kernel puts into its LDS image.
130 samples are 3 chunks, the last with 2 samples: the chunk count is a multiple of neither 2 nor 4, so the workgroups of the 2- and
4-wavefront kernels straddle records and run boundaries.

  plain  no dense region: every entry fits the 128 bytes a lane keeps in registers, nearly every chunk fits the 4 KiB image
  mid    a dense region of 4 alleles: entries of up to 139 bytes (past the registers), chunks in every bin (4096, 6144], (6144, 8192]
         and over 8192 with no entry over 512 bytes: the multi-pass branch of the LDS image, with another pass count per image size
  wide   the same with 8 alleles: entries over 255 bytes (the 8-byte matrix by itself), none over 512
  long   64 alleles, 150 samples: entries over 512 bytes (copied by the whole wavefront), several over 4096

test_variant_shapes.py asserts these properties from the oracle's text on the CPU; the GPU tests rely on them."""
import collections
import os

import helpers

B = 10_000_000
TAIL = 2500          # columns generated behind the interval (cells that begin inside it end there)

#        name      N    L     dense region                     query overrides
SHAPES = {
    "plain": (130, 2000, None, {}),
    "mid": (130, 1500, (B + 100, 300, 50, 4), {}),
    "wide": (130, 1500, (B + 100, 300, 50, 8), {}),
    "long": (150, 1500, (B + 100, 200, 50, 64), {"max_diploid_alt_alleles_that_can_be_genotyped": 64}),
}

Shape = collections.namedtuple("Shape", "name N begin end cells query want nrec")


def inputs(name, tmpdir):
    """(N, begin, end, cells, query) of a named shape; the metadata files go to tmpdir/name"""
    from genomicsdb_amd import synth
    N, L, dense, overrides = SHAPES[name]
    g = synth.Generator(N, B, L + TAIL, dense=dense)
    cells, _ = g.chunk_bytes(B + L + TAIL)
    g.close()
    d = os.path.join(str(tmpdir), name)
    os.makedirs(d, exist_ok=True)
    q = helpers.synth_query(d, N, B, B + L - 1)
    q.update(overrides)
    return N, B, B + L - 1, cells, q


def build(name, tmpdir):
    """a named shape with the oracle's bytes (no header) and record count"""
    from genomicsdb_amd import synth
    N, begin, end, cells, q = inputs(name, tmpdir)
    want, nrec, _ = helpers.oracle_run_synth(q, cells, synth.SEED, with_header=False)
    return Shape(name, N, begin, end, cells, q, want, nrec)


def reference_bases(begin, end):
    from genomicsdb_amd import synth
    return synth.reference(begin, end - begin + 1 + TAIL + 4096)


def records(want):
    return [l for l in want.split(b"\n") if l]


def entry_lengths(want):
    """bytes of every sample entry (no tab), record by record"""
    return [[len(c) for c in l.split(b"\t")[9:]] for l in records(want)]


def chunk_lengths(want):
    """bytes of every (record, 64-sample chunk), tabs included"""
    return [sum(e[i:i + 64]) + len(e[i:i + 64]) for e in entry_lengths(want) for i in range(0, len(e), 64)]


def record_bytes(want):
    return [len(l) + 1 for l in records(want)]


# ---- the tests' copy of the dispatch ------------------------------------------------------------------------------------------------
SIZE_PLAIN, SIZE_3X8, SIZE_3X16, SIZE_PIECES, SIZE_EVENTS = 0, 1, 2, 3, 4
PAGE_WRITE, PAGE_WRITE2, PAGE_WRITE3, PAGE_EVENTS, PAGE_BCF = 1, 2, 3, 4, 5
COOPERATIVE_ENTRY = 512          # kCooperativeEntry


def code(S, K, W, C, II):
    return S * 100000 + K * 10000 + W * 1000 + C * 100 + II


def page_ranges(rec_bytes, arena_bytes, event_block=None):
    """[(first record, end record)] of the pages begin_page cuts: as many whole records as fit max(arena, largest record); on the
    change-list path a page that starts on an order-block boundary is cut back to one"""
    P = len(rec_bytes)
    cap = max(arena_bytes, max(rec_bytes))
    if sum(rec_bytes) <= cap:
        return [(0, P)]
    out, kp = [], 0
    while kp < P:
        ke, used = kp, 0
        while ke < P and used + rec_bytes[ke] <= cap:
            used += rec_bytes[ke]
            ke += 1
        if event_block and ke < P and kp % event_block == 0 and (ke // event_block) * event_block > kp:
            ke = (ke // event_block) * event_block
        out.append((kp, ke))
        kp = ke
    return out


_rec_cache = {}


def _record_bytes_of(shape):
    key = (shape.name, len(shape.want))
    if key not in _rec_cache:
        _rec_cache[key] = record_bytes(shape.want)
    return _rec_cache[key]


def expected_code(shape, env, arena_bytes, untabled=False, bcf=False):
    """IntervalStats.page_kernel of the LAST page of shape's interval under the knobs in env (a dict of GDBAMD_* -> str), derived from
    the oracle's text and the knobs alone; bcf: an engine that writes BCF2 records (no matrix-free path: odd paths become 2, and no events)"""
    def knob(name, default):
        v = env.get("GDBAMD_" + name, "")
        return int(v) if v != "" else default
    rec = _record_bytes_of(shape)
    P, nchunks = len(rec), (shape.N + 63) // 64
    events_on = knob("EVENTS", 0) != 0
    path = 0 if events_on else min(3, max(0, knob("ASM_PATH", 0)))
    if bcf and path & 1:
        path = 2
    if path == 3 and untabled:
        path = 0
    size3 = knob("SIZE3", 8)
    rounds = 0 if size3 == 0 else 16 if size3 >= 16 else 8
    run = max(1, knob("RUN", 128 if rounds else 64))
    budget = knob("RESOLVED_MB", 32 << 10) << 20
    ww = knob("WRITE_WAVES", 1)
    avg_chunk = sum(rec) // (P * nchunks)
    wl = knob("WRITE_IMAGE_KB", 4 if avg_chunk <= 3400 else 8)
    blk = 1 << min(30, max(0, knob("ORDER_BLOCK_LOG2", 12)))
    evrun = max(1, min(64, knob("EV_RUN", 32)))
    use_events = not bcf and events_on and (-(-P // evrun)) * nchunks * evrun * 64 * 8 <= budget and blk % evrun == 0
    if use_events:
        S = SIZE_EVENTS
    elif path != 0:
        S = SIZE_PIECES
    else:
        S = SIZE_PLAIN if rounds == 0 or run > 65536 else SIZE_3X16 if rounds == 16 else SIZE_3X8
    if bcf:
        return code(S, PAGE_BCF, 1, 0, 0)
    kp, ke = page_ranges(rec, arena_bytes, blk if use_events else None)[-1]
    if use_events and kp % blk == 0 and (ke == P or ke % blk == 0):
        return code(S, PAGE_EVENTS, 4 if ww >= 4 else 1, 0, 8)
    if path == 3:
        return code(S, PAGE_WRITE3, 1, 0, 4 if wl <= 4 else 8)
    if path == 1:
        if ww >= 4:
            return code(S, PAGE_WRITE2, 4, 0, 4 if wl <= 4 else 8)
        return code(S, PAGE_WRITE2, 1, 0, 4 if wl <= 4 else 6 if wl <= 6 else 8)
    # k_assemble_write: the largest record's average entry decides on the 4-word cooperative copy
    long_entries = knob("COOP_UNROLL", 1) != 0 and max(rec) // (nchunks * 64) > COOPERATIVE_ENTRY
    if long_entries and ww == 1:
        return code(S, PAGE_WRITE, 1, 4, 8)
    if ww >= 4:
        return code(S, PAGE_WRITE, 4, 2, 4 if wl <= 4 else 6 if wl <= 6 else 8)
    if ww == 2:
        return code(S, PAGE_WRITE, 2, 2, 4 if wl <= 4 else 8)
    return code(S, PAGE_WRITE, 1, 2, 4 if wl <= 4 else 8)
