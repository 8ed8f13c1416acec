"""The body of the tile inflater of compressed fragment files (csrc/core/gdb_tile_inflate.hpp: gdbtile::tile_inflate, what every
thread of k_inflate_tiles runs) on the CPU, through the harness tests/hostsim_tile_inflate.  Every stream is compared with
zlib.decompressobj(-15): same verdict (accepted as a stream of exactly `want` bytes, or not), the same bytes when accepted, the
expected TileErr when refused, and the output slot untouched behind `want`.  The streams are hand-made for this decoder
(tests/tools/tile_streams.py), zlib-made, and seeded mutations of those.  Host code only - no device."""
import ctypes
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import tile_streams as ts  # noqa: E402
from tile_streams import OK, E_CODE, E_INPUT, E_SIZE, E_OUTPUT, TILE  # noqa: E402

FILL = 0xA5
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_tile_inflate")


def load_sim():
    from genomicsdb_amd import build as b
    lib, _ = b.build_hostsim_tile_inflate()
    L = ctypes.CDLL(lib)
    c = ctypes
    L.hostsim_tile_inflate.argtypes = [c.c_char_p, c.c_uint32, c.c_uint32, c.c_uint8, c.c_char_p]
    L.hostsim_tile_inflate_many.argtypes = [c.c_char_p, c.POINTER(c.c_uint64), c.POINTER(c.c_uint32), c.c_uint64, c.c_uint8, c.c_char_p, c.c_char_p]
    L.hostsim_tile_bytes.restype = c.c_uint32
    L.hostsim_tile_scratch_bytes.restype = c.c_uint32
    return L


@pytest.fixture(scope="module")
def sim():
    return load_sim()


@pytest.fixture(scope="module")
def hand():
    return ts.hand_made_cases()


@pytest.fixture(scope="module")
def grid():
    return ts.zlib_grid()


def inflate(L, stream, want):
    """-> (TileErr, the slot of 8192 bytes)"""
    slot = ctypes.create_string_buffer(TILE)
    err = L.hostsim_tile_inflate(bytes(stream), len(stream), want, FILL, slot)
    assert 0 <= err <= 9
    return err, slot.raw


def inflate_many(L, streams, wants):
    """the harness over a job list, as the kernel gets it -> (status bytes, slots)"""
    n = len(streams)
    offs = (ctypes.c_uint64 * (n + 1))()
    for i, s in enumerate(streams):
        offs[i + 1] = offs[i] + len(s)
    out, status = ctypes.create_string_buffer(max(n, 1) * TILE), ctypes.create_string_buffer(max(n, 1))
    assert L.hostsim_tile_inflate_many(b"".join(streams), offs, (ctypes.c_uint32 * n)(*wants), n, FILL, out, status) == 0
    return status.raw[:n], out.raw[:n * TILE]


def agrees_with_zlib(err, slot, stream, want, what):
    """the four properties of every case; -> zlib's bytes or None"""
    ref = ts.zlib_verdict(stream, want)
    assert (err == OK) == (ref is not None), "%s: zlib %s, the body says TileErr %d" % (what, "accepts" if ref is not None else "refuses", err)
    if ref is not None:
        assert slot[:want] == ref, "%s: accepted with other bytes than zlib's" % what
    assert slot[want:] == bytes([FILL]) * (TILE - want), "%s: bytes behind want = %d were written" % (what, want)
    return ref


def test_constants(sim):
    assert sim.hostsim_tile_bytes() == TILE and sim.hostsim_tile_scratch_bytes() == 1024


def test_hand_made_streams(sim, hand):
    assert len(hand) > 300 and len({c.name for c in hand}) == len(hand)
    for c in hand:
        err, slot = inflate(sim, c.stream, c.want)
        ref = agrees_with_zlib(err, slot, c.stream, c.want, c.name)
        assert err == c.expect, "%s: TileErr %d, expected %d" % (c.name, err, c.expect)
        if c.expect == OK:
            assert ref == c.payload, "%s: the stream does not say what the case means" % c.name


@pytest.mark.parametrize("name", ["a single literal / length code of two bits", "a single distance code of two bits"])
def test_one_code_of_two_bits_is_not_the_permitted_incomplete_code(sim, hand, name):
    """RFC 1951 permits an incomplete code only as one code of ONE bit; zlib, the host side of the fragment reader (zlib) and the
    BGZF inflater (INF_ERR_CODE) refuse one code of two bits, and so does the tile inflater."""
    c = [c for c in hand if c.name == name][0]
    assert ts.zlib_verdict(c.stream, c.want) is None
    err, _ = inflate(sim, c.stream, c.want)
    assert err == E_CODE


def test_trailing_bytes_are_accepted_as_zlib_accepts_them(sim, hand):
    cs = [c for c in hand if "bytes behind " in c.name]
    assert len(cs) == 10
    for c in cs:
        assert inflate(sim, c.stream, c.want)[0] == OK and ts.zlib_verdict(c.stream, c.want) == c.payload


def test_zlib_made_streams(sim, grid):
    assert len(grid) == 300 and {len(d) for _, d in grid} >= set(range(41)) | {TILE - 1, TILE}
    assert {(z[0] >> 1) & 3 for z, _ in grid} == {0, 1, 2}           # stored, fixed and dynamic first blocks
    for i, (z, d) in enumerate(grid):
        err, slot = inflate(sim, z, len(d))
        assert agrees_with_zlib(err, slot, z, len(d), "stream %d" % i) == d and err == OK
        if d:
            err, slot = inflate(sim, z, len(d) - 1)
            agrees_with_zlib(err, slot, z, len(d) - 1, "stream %d, want - 1" % i)
            assert err == E_OUTPUT
        if len(d) < TILE:
            err, slot = inflate(sim, z, len(d) + 1)
            agrees_with_zlib(err, slot, z, len(d) + 1, "stream %d, want + 1" % i)
            assert err == E_SIZE
        assert inflate(sim, z[:-1], len(d))[0] == E_INPUT


def mutation_answers(muts):
    """zlib's answer to every mutation"""
    return [ts.zlib_verdict(m[0], m[1]) for m in muts]


def test_mutation_fuzz(sim, grid, capsys):
    muts = ts.mutations(grid)
    refs = mutation_answers(muts)
    refused = sum(r is None for r in refs)
    # accepted as a stream of the same size, but with other bytes than the unchanged stream has
    changed = sum(r is not None and r != m[3] for r, m in zip(refs, muts))
    flips = [(r, m) for r, m in zip(refs, muts) if m[2] == "flip"]
    flips_changed = sum(r is not None and r != m[3] for r, m in flips)
    with capsys.disabled():
        print("\n  mutation fuzz: %d mutations, zlib refuses %d (%.1f %%), accepts %d as same-size streams with other bytes (%.1f %%); "
              "one-bit flips: %d of %d (%.1f %%) accepted with other bytes"
              % (len(muts), refused, 100.0 * refused / len(muts), changed, 100.0 * changed / len(muts), flips_changed, len(flips), 100.0 * flips_changed / len(flips)))
    assert len(muts) == 4000
    assert 3 * refused >= len(muts)
    assert 10 * changed >= len(muts)
    status, out = inflate_many(sim, [m[0] for m in muts], [m[1] for m in muts])
    for k, ((s, want, kind, _), ref) in enumerate(zip(muts, refs)):
        slot = out[k * TILE:(k + 1) * TILE]
        assert (status[k] == OK) == (ref is not None), "mutation %d (%s): zlib %s, the body says TileErr %d" % (k, kind, "accepts" if ref is not None else "refuses", status[k])
        if ref is not None:
            assert slot[:want] == ref, "mutation %d (%s): accepted with other bytes than zlib's" % (k, kind)
        assert slot[want:] == bytes([FILL]) * (TILE - want), "mutation %d (%s): bytes behind want were written" % (k, kind)


def test_stand_alone_program_under_the_sanitizers(sim, hand, grid, tmp_path):
    """tile_inflate_fuzz is built with -fsanitize=address,undefined -fno-sanitize-recover=all: exact-size heap blocks for every stream
    and every slot.  It runs the hand-made list, the zlib grid (as cases) and its own seeded mutations, each compared with zlib."""
    subprocess.check_call(["make", "-s", "-C", DIR])
    cases = list(hand) + [ts.Case("grid %d" % i, z, len(d), OK, d) for i, (z, d) in enumerate(grid)]
    path = tmp_path / "cases.bin"
    ts.write_case_file(path, cases)
    r = subprocess.run([os.path.join(DIR, "tile_inflate_fuzz"), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases" % len(cases) in r.stdout and "4000 mutations" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
