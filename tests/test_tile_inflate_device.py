"""The tile inflater of compressed fragment files on the device: k_inflate_tiles driven directly (genomicsdb_amd.inflate_tiles: the
same kernel, launch shape and buffer sizes as the fragment reader) and through the file path around it (save_fragment /
load_fragment / the query stream over a workspace).  Every stream sent to the device has gone through the CPU harness of the same
body (tests/hostsim_tile_inflate) in the same test first; the device's verdict per tile, its bytes and the untouched tails of the
output slots must equal the harness's and zlib's.  What the device adds to a CPU run of the body: neighbouring lanes of one
wavefront hold different block kinds, lengths, and accepted and refused tiles side by side."""
import os
import random
import sys
import zlib

import pytest

import helpers
from golden_cases import CASES

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import fragment_file  # noqa: E402
import tile_streams as ts  # noqa: E402
import test_tile_inflate_bodies_cpu as bodies  # noqa: E402
from tile_streams import OK, TILE  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = bodies.FILL


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    from genomicsdb_amd import _lib
    assert _lib.lib().gdb_mi355_device_count() > 0, "no HIP device"
    return genomicsdb_amd


@pytest.fixture(scope="module")
def sim():
    return bodies.load_sim()


@pytest.fixture(scope="module")
def hand():
    return ts.hand_made_cases()


@pytest.fixture(scope="module")
def grid():
    return ts.zlib_grid()


def launch(gdb, sim, jobs, refs=None):
    """jobs [(stream, want)] through the harness, then as ONE launch through the kernel; both must give zlib's verdict and bytes and
    leave every slot untouched behind `want`, and the device must give the harness's TileErr and slot, byte for byte.  -> status"""
    streams, wants = [j[0] for j in jobs], [j[1] for j in jobs]
    refs = [ts.zlib_verdict(s, w) for s, w in jobs] if refs is None else refs
    cpu_status, cpu_out = bodies.inflate_many(sim, streams, wants)
    dev_status, dev_out = gdb.inflate_tiles(streams, wants, fill=FILL)
    assert len(dev_status) == len(jobs) and len(dev_out) == len(jobs) * TILE
    for name, status, out in (("harness", cpu_status, cpu_out), ("device", dev_status, dev_out)):
        for k, ((s, want), ref) in enumerate(zip(jobs, refs)):
            slot = out[k * TILE:(k + 1) * TILE]
            assert (status[k] == OK) == (ref is not None), "%s, tile %d: zlib %s, TileErr %d" % (name, k, "accepts" if ref is not None else "refuses", status[k])
            if ref is not None:
                assert slot[:want] == ref, "%s, tile %d: accepted with other bytes than zlib's" % (name, k)
            assert slot[want:] == bytes([FILL]) * (TILE - want), "%s, tile %d: bytes behind want = %d were written" % (name, k, want)
    assert dev_status == cpu_status, [(k, a, b) for k, (a, b) in enumerate(zip(dev_status, cpu_status)) if a != b][:10]
    if dev_out != cpu_out:
        k = [k for k in range(len(jobs)) if dev_out[k * TILE:(k + 1) * TILE] != cpu_out[k * TILE:(k + 1) * TILE]][0]
        raise AssertionError("tile %d (TileErr %d): the device's slot differs from the harness's" % (k, dev_status[k]))
    return dev_status


def shuffled_jobs(hand, grid, seed=64):
    jobs = [(c.stream, c.want, c.expect) for c in hand] + [(z, len(d), OK) for z, d in grid]
    random.Random(seed).shuffle(jobs)
    return jobs


def test_whole_case_list_in_one_launch(gdb, sim, hand, grid):
    """the hand-made list and the zlib grid, shuffled: the 64 lanes of a wavefront hold stored, fixed and dynamic blocks, streams of
    2 bytes and of 8 KiB, accepted and refused tiles side by side"""
    jobs = shuffled_jobs(hand, grid)
    status = launch(gdb, sim, [(s, w) for s, w, _ in jobs])
    assert list(status) == [e for _, _, e in jobs]
    for w0 in range(0, len(jobs) - 63, 64):                 # every full wavefront holds both accepted and refused tiles
        assert 0 < sum(e == OK for _, _, e in jobs[w0:w0 + 64]) < 64


@pytest.mark.parametrize("ntiles", [1, 63, 64, 65, 130])
def test_tile_counts_around_the_block(gdb, sim, hand, grid, ntiles):
    """tile counts around the 64-thread block; the last tile's stream (dynamic codes, decoded to its last bit) ends at the last
    byte of the input"""
    jobs = [(s, w) for s, w, _ in shuffled_jobs(hand, grid, seed=ntiles)][:ntiles - 1]
    last = [c for c in hand if c.name == "dynamic stream of zlib"][0]
    jobs.append((last.stream, last.want))
    status = launch(gdb, sim, jobs)
    assert status[-1] == OK


def test_want_edges(gdb, sim, grid):
    jobs = []
    for n in (0, 1, TILE - 1, TILE):
        for z, d in [g for g in grid if len(g[1]) == n]:
            jobs.append((z, n, OK))
            if n > 0:
                jobs.append((z, n - 1, ts.E_OUTPUT))
            if n < TILE:
                jobs.append((z, n + 1, ts.E_SIZE))
    for z, d in [g for g in grid[50:90] if len(g[1]) < TILE]:
        jobs += [(z, len(d) - 1, ts.E_OUTPUT), (z, len(d), OK), (z, len(d) + 1, ts.E_SIZE)]
    assert {w for _, w, e in jobs if e == OK} >= {0, 1, TILE - 1, TILE}
    status = launch(gdb, sim, [(s, w) for s, w, _ in jobs])
    assert list(status) == [e for _, _, e in jobs]


def test_mutations_in_one_launch(gdb, sim, grid):
    """the 4 000 seeded mutations of tests/test_tile_inflate_bodies_cpu.py::test_mutation_fuzz: zlib's verdict and bytes, tile by tile"""
    muts = ts.mutations(grid)
    refs = bodies.mutation_answers(muts)
    assert len(muts) == 4000 and 3 * sum(r is None for r in refs) >= len(muts) and 10 * sum(r is not None and r != m[3] for r, m in zip(refs, muts)) >= len(muts)
    launch(gdb, sim, [(m[0], m[1]) for m in muts], refs)


# ---- the file path around the kernel

def _one_literal_per_block_then_level_1(raw):
    b = ts.Bits()
    for x in raw[:100]:
        ts.fixed_block([x], final=False, b=b)
    ts.stored_block(b"", final=False, b=b)                  # (an empty stored block: what follows is byte-aligned, as zlib wrote it)
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    return b.bytes() + co.compress(raw[100:]) + co.flush()


def _flushed(raw):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return b"".join(co.compress(raw[a:a + 700]) + co.flush(zlib.Z_SYNC_FLUSH) for a in range(0, len(raw), 700)) + co.flush()


def _with(level, strategy=zlib.Z_DEFAULT_STRATEGY):
    def w(raw):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        return co.compress(raw) + co.flush()
    return w


WRITERS = [_with(0), _with(6, zlib.Z_FIXED), _with(9), _with(6, zlib.Z_HUFFMAN_ONLY), _with(6, zlib.Z_RLE), _flushed, _one_literal_per_block_then_level_1]


def mixed_v3(raw_blob):
    """the version-3 file of a raw (version-2) file whose tile i, counted over the whole file, comes from writer i mod 7; every
    stream is checked with zlib on the way.  -> (file bytes, parsed raw file, tiles written per writer)"""
    frag = fragment_file.parse(raw_blob)
    count = [0]
    used = [0] * len(WRITERS)

    def writer(raw, sec, i):
        k = count[0] % len(WRITERS)
        count[0] += 1
        used[k] += 1
        z = WRITERS[k](raw)
        assert ts.zlib_verdict(z, len(raw)) == raw
        return z
    return fragment_file.write_v3(frag, writer), frag, used


def _small_synthetic(tmp_path):
    from test_gpu_parity import _synth_cells
    N, B, L = 40, 10_000_000, 6_000                         # the array of test_damaged_fragment_columns_are_refused
    cells, _ = _synth_cells(N, B, L)
    return cells, helpers.synth_query(tmp_path, N, B, B + L - 1)


def _golden(name):
    case = [c for c in CASES if c[0] == name][0]
    q, _ = helpers.query_json(case[1], case[2], case[3], case[5])
    return helpers.cells_for(case[1], case[2]), q


@pytest.mark.parametrize("source", ["synthetic", "t0_1_2_loading", "t6_7_8_loading"])
def test_round_trip_through_hbm(gdb, tmp_path, source):
    """cells -> raw file -> version-3 file with seven kinds of tile writers -> load_fragment (inflated on the device) -> raw file
    again: the two raw files are compared byte for byte, every section and not only what a query prints.  The goldens have
    sections shorter than one tile; an empty data section is no tile and an index of one offset."""
    cells, q = _small_synthetic(tmp_path) if source == "synthetic" else _golden(source)
    e = gdb.CombineEngine(q)
    e.stage_cells(cells)
    e.save_fragment(tmp_path / "raw1.gdbamd")
    e.close()
    raw1 = (tmp_path / "raw1.gdbamd").read_bytes()
    z_blob, frag, used = mixed_v3(raw1)
    if source == "synthetic":
        assert min(used) >= 2 and max(s.ntiles for s in frag.sections) >= 3
    else:
        assert all(s.ntiles <= 1 for s in frag.sections)      # (a field no cell has a value for gives a data section without tiles)
    (tmp_path / "mixed.gdbamd").write_bytes(z_blob)
    e = gdb.CombineEngine(q)
    e.load_fragment(tmp_path / "mixed.gdbamd")
    e.save_fragment(tmp_path / "raw2.gdbamd")
    e.close()
    raw2 = (tmp_path / "raw2.gdbamd").read_bytes()
    # (the 88 header bytes hold the source's size and time, which the engine that loaded a file does not know: compared field by field below)
    assert raw2[88:] == raw1[88:]
    assert raw2[:40] == raw1[:40]                           # magic, version, field / cell / marker / row counts
    a, b = fragment_file.parse(raw1), fragment_file.parse(raw2)
    assert [(s.name, s.raw) for s in a.sections] == [(s.name, s.raw) for s in b.sections]


def test_windows_begin_and_end_inside_tiles(gdb, tmp_path, monkeypatch):
    """the mixed-writer file as the array of a workspace, read in windows of a ninth of the cells: the stream equals the resident one"""
    import json
    cells, q = _small_synthetic(tmp_path)
    monkeypatch.delenv("GDBAMD_STAGE_BUDGET_BYTES", raising=False)
    s = gdb.GenomicsDBQueryStream(query_json=q, cells=cells, buffer_capacity=1 << 20)
    resident = s.read()
    s.close()
    e = gdb.CombineEngine(q)
    e.stage_cells(cells)
    e.save_fragment(tmp_path / "raw.gdbamd")
    e.close()
    ws = tmp_path / "ws"
    (ws / "arr").mkdir(parents=True)
    z_blob, frag, _ = mixed_v3((tmp_path / "raw.gdbamd").read_bytes())
    (ws / "arr" / "fragment.gdbamd").write_bytes(z_blob)
    assert max(s.ntiles for s in frag.sections) >= 3 and (frag.C // 9 * 4) % TILE != 0      # (a ninth of the cells is no whole number of tiles)
    q2 = dict(q, workspace=str(ws), array="arr")
    qf = tmp_path / "query.json"
    qf.write_text(json.dumps(q2))
    monkeypatch.setenv("GDBAMD_STAGE_BUDGET_BYTES", str(len(cells) // 9))
    s = gdb.GenomicsDBQueryStream(query_json_file=str(qf), buffer_capacity=1 << 20)
    got = s.read()
    s.close()
    assert got == resident and len(resident) > 10000


def test_damage_names_its_place(gdb, tmp_path):
    """a tile whose stream is cut short (the tile index says so: the file is consistent) is refused with the section, the tile and
    the reason in the message"""
    cells, q = _small_synthetic(tmp_path)
    e = gdb.CombineEngine(q)
    e.stage_cells(cells)
    e.save_fragment(tmp_path / "raw.gdbamd")
    e.close()
    frag = fragment_file.parse((tmp_path / "raw.gdbamd").read_bytes())
    # a data section: the host side reads tiles of `begin` and of the offsets with zlib when it opens the file, data tiles only the device reads
    victim = [s for s in frag.sections if s.name.endswith(" data") and s.ntiles >= 3][0]
    tile = victim.ntiles - 2

    def writer(raw, sec, i):
        z = WRITERS[1](raw)
        return z[:-2] if sec is victim and i == tile else z
    good = fragment_file.write_v3(frag, lambda raw, sec, i: WRITERS[1](raw))
    (tmp_path / "good.gdbamd").write_bytes(good)
    e = gdb.CombineEngine(q)
    e.load_fragment(tmp_path / "good.gdbamd")
    e.close()
    (tmp_path / "bad.gdbamd").write_bytes(fragment_file.write_v3(frag, writer))
    e = gdb.CombineEngine(q)
    with pytest.raises(gdb.GenomicsDBException, match="inflate|corrupt|tile") as ei:
        e.load_fragment(tmp_path / "bad.gdbamd")
    e.close()
    msg = str(ei.value)
    assert "does not inflate to its size (corrupt file)" in msg
    assert "section %s, tile %d: stream ends early" % (victim.name, tile) in msg, msg
    assert victim.field.name in msg
