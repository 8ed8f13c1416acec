"""The shapes of variant_shapes.py must keep the properties the GPU tests of test_gpu_kernel_variants.py rely on to reach their
branches: recomputed here from the oracle's text alone (no GPU), so that a change of the generator shows on the CPU."""
import pytest

import variant_shapes as vs


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    d = tmp_path_factory.mktemp("variant_shapes")
    return {name: vs.build(name, d) for name in vs.SHAPES}


def test_shapes_reach_the_branches_the_kernel_variant_tests_need(shapes):
    # the tests' model of begin_page's paging, on a hand-made case first
    rec = [10, 10, 10, 30, 10, 10, 10, 10]
    assert vs.page_ranges(rec, 1000) == [(0, 8)]
    assert vs.page_ranges(rec, 1) == [(0, 3), (3, 4), (4, 7), (7, 8)]                 # pages of the largest record's size
    assert vs.page_ranges(rec, 1, event_block=2) == [(0, 2), (2, 3), (3, 4), (4, 6), (6, 8)]   # cut back to an order-block boundary where one is inside
    longest = {n: max(max(e) for e in vs.entry_lengths(s.want)) for n, s in shapes.items()}
    chunks = {n: vs.chunk_lengths(s.want) for n, s in shapes.items()}
    for n, s in shapes.items():
        assert len(vs.records(s.want)) == s.nrec and s.nrec > 1000, n            # more than one order block of 32 / 64, many runs
        assert all(len(e) == s.N for e in vs.entry_lengths(s.want)), n
        assert (s.N + 63) // 64 == 3 and s.N % 64 not in (0, 63), n              # 3 chunks (no multiple of 2 or 4), a short last one
    # plain: the register path only, (nearly) every chunk in a 4 KiB image
    assert longest["plain"] <= 128
    assert sum(c > 4096 for c in chunks["plain"]) * 100 < len(chunks["plain"])
    # mid: texts past the 128 bytes in registers, the compact matrix, every image size takes a different number of passes
    assert 128 < longest["mid"] <= 255
    assert any(4096 < c <= 6144 for c in chunks["mid"])
    assert any(6144 < c <= 8192 for c in chunks["mid"])
    assert any(c > 8192 for c in chunks["mid"])
    # wide: the 8-byte matrix by itself, still everything through the LDS image
    assert 255 < longest["wide"] <= vs.COOPERATIVE_ENTRY
    assert any(c > 8192 for c in chunks["wide"])
    # long: the whole-wavefront copy, entries longer than a 4 KiB image; the largest record's AVERAGE entry is a long one (COOP_U = 4)
    long_entries = [e for rec in vs.entry_lengths(shapes["long"].want) for e in rec]
    assert any(e > vs.COOPERATIVE_ENTRY for e in long_entries) and any(e > 4096 for e in long_entries)
    assert max(vs.record_bytes(shapes["long"].want)) // (3 * 64) > vs.COOPERATIVE_ENTRY
    for n in ("plain", "mid", "wide"):
        assert max(vs.record_bytes(shapes[n].want)) // (3 * 64) <= vs.COOPERATIVE_ENTRY, n
    # the two pagings of the GPU tests: several pages of many records, and (arena_bytes = 1) pages of the largest record's size - with
    # the default runs of 32 records a grid of 3 or 6 units, fewer than the 8 workgroups xcd_aware_unit deals round; long's largest
    # record is larger than 1 MiB, so its two pagings are the same one
    for n, s in shapes.items():
        rec = vs.record_bytes(s.want)
        assert sum(rec) == len(s.want)
        assert 2 <= len(vs.page_ranges(rec, 1 << 20)) < s.nrec // 8, n
        tiny = vs.page_ranges(rec, 1)
        if n == "long":
            assert tiny == vs.page_ranges(rec, 1 << 20)
        else:
            assert len(tiny) > 100 and max(ke - kp for kp, ke in tiny) <= 64, n
