"""Crafted sources of the windowed merge (genomicsdb_amd.merge_cell_files), shared by its CPU harness test and its GPU test: the
shapes at which a round can go wrong - a read that ends at every place of a cell, a source that waits while the other is merged,
runs of one key and cells larger than a source's share of the window - and the sources of its refusals.  The yardstick of every
shape is merge_inputs.sorted_merge."""
import merge_inputs as mi

MIXED = (0, 1, 15, 16, 17, 63, 64, 65)
TILE = 1024
# 64-byte cells: a window of 640 bytes ends a one-source read at a cell end, 641 and 663 1 and 23 bytes into a header, 664 at the end
# of a header, 680 inside a payload
BOUNDARY_WINDOWS = (640, 641, 663, 664, 680)


def cells64(n, row=0, col0=0, step=1):
    """n cells of exactly 64 bytes in one row, columns col0, col0 + step, .."""
    return [mi.cell(row, col0 + i * step, bytes([(i * 7 + row) % 251]) * 40) for i in range(n)]


def shapes():
    """[(name, sources, windows, expectations)]; expectations: dict of "grown" / "rounds" / "carried" -> "pos" | "one" | "zero" """
    out = []
    one = b"".join(cells64(200))
    out.append(("one source of 64-byte cells", [one], BOUNDARY_WINDOWS, dict(rounds="pos", carried="pos", grown="zero")))
    two = [b"".join(cells64(200, row=0, step=2)), b"".join(cells64(200, row=1, col0=1, step=2))]
    out.append(("two sources of 64-byte cells", two, BOUNDARY_WINDOWS + tuple(2 * w for w in BOUNDARY_WINDOWS), dict(rounds="pos", carried="pos", grown="zero")))
    rng = mi.rng(5)
    lo = b"".join(mi.cell(i % 2, i // 2, rng.randbytes(rng.choice(MIXED))) for i in range(2 * TILE + 3))
    hi = b"".join(mi.cell(2 + i % 2, 10**6 + i // 2, rng.randbytes(rng.choice(MIXED))) for i in range(TILE + 7))
    out.append(("lo before hi", [lo, hi], (4096,), dict(rounds="pos", carried="pos")))
    out.append(("hi listed before lo", [hi, lo], (4096,), dict(rounds="pos", carried="pos")))
    even = b"".join(mi.cell(0, i, rng.randbytes(rng.choice(MIXED))) for i in range(0, 2 * TILE + 2, 2))
    odd = b"".join(mi.cell(1, i, rng.randbytes(rng.choice(MIXED))) for i in range(1, 2 * TILE + 1, 2))
    out.append(("alternation", [even, odd], (4096,), dict(rounds="pos", carried="pos")))
    out.append(("alternation, odd first", [odd, even], (4096,), dict(rounds="pos", carried="pos")))
    # runs of one key longer than any share of the window; the other source's keys fall before, between and behind the runs
    runs = b"".join(mi.cell(0, 10, b"first run %d" % i) for i in range(1324)) + b"".join(mi.cell(0, 20, b"second run %d" % i) for i in range(2049))
    other = mi.crafted_stream(mi.rng(6), 500, (1, 2), 30, MIXED)
    out.append(("equal-key runs", [runs, other], (4096,), dict(grown="pos", rounds="pos")))
    out.append(("equal-key runs, listed second", [other, runs], (4096,), dict(grown="pos", rounds="pos")))
    r = mi.rng(7)
    with_big = b"".join(mi.cell(i % 2 * 2, i // 2, r.randbytes(20000 if i == 150 else r.choice(MIXED))) for i in range(300))
    out.append(("an oversized cell", [with_big, mi.crafted_stream(mi.rng(9), 300, (1, 3), 40, MIXED)], (4096,), dict(grown="pos", rounds="pos")))
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        r = mi.rng(n)
        A = mi.crafted_stream(r, n // 2, (0, 2, 4), 97, MIXED)
        B = mi.crafted_stream(r, n - n // 2, (1, 3), 97, MIXED)
        out.append(("total %d in one round" % n, [A, B], (1 << 22,), dict(rounds="one", carried="zero", grown="zero")))
        out.append(("total %d in one round, 1 and the rest" % n, [mi.crafted_stream(r, 1, (0,), 97, MIXED), mi.crafted_stream(r, n - 1, (1, 3), 97, MIXED)], (1 << 22,),
                    dict(rounds="one", carried="zero", grown="zero")))
    five = [mi.crafted_stream(mi.rng(20 + s), 300 + 41 * s, (s,), 61, MIXED) for s in range(5)]
    out.append(("five sources", five, (4096, 1 << 22), dict()))
    a = mi.cell(3, 7, b"abc")
    out.append(("no cells at all", [b"", b""], (1, 4096), dict(rounds="one")))
    out.append(("an empty source beside a non-empty one", [b"", mi.crafted_stream(mi.rng(30), 200, (0, 1), 50, MIXED)], (512,), dict(rounds="pos")))
    out.append(("a single cell", [a], (1, 4096), dict()))
    out.append(("one source: a windowed copy", [mi.crafted_stream(mi.rng(31), 300, (0, 1, 2), 50, MIXED)], (2048,), dict(rounds="pos")))
    return out


def refusals():
    """[(name, sources, window, regular expression of the message)]; every one involves a chunk boundary.  With a one-source window of
    640 bytes and 64-byte cells, round 0 loads cells 0..9 and every later round nine more: cells 19, 28, .. are the first of a chunk"""
    out = []
    cells = cells64(200)
    swapped = list(cells)
    swapped[18], swapped[19] = swapped[19], swapped[18]
    out.append(("a swapped pair across a chunk boundary", [b"".join(swapped)], 640, r"stream 0 is not sorted by \(column, row\): cell 19 comes before cell 18"))
    inside = list(cells)
    inside[23], inside[24] = inside[24], inside[23]
    out.append(("a swapped pair inside a late chunk", [b"".join(inside)], 640, r"stream 0 is not sorted by \(column, row\): cell 24 comes before cell 23"))
    good = b"".join(cells64(100, row=7, col0=1000))
    out.append(("a swapped pair in the second source", [good, b"".join(swapped)], 1280, r"stream 1 is not sorted by \(column, row\): cell 19 comes before cell 18"))
    head = b"".join([mi.cell(5, 0, b"x" * 40)] + cells64(150, row=0, col0=1))
    tail = b"".join(cells64(150, row=1, col0=1) + [mi.cell(5, 10**6, b"y" * 40)])
    out.append(("one shared row, at a head and at a tail", [head, tail], 1280, r"row 5 is in more than one stream"))
    negative = list(cells)
    negative[150] = mi.cell(-1, 150, b"n" * 40)
    out.append(("a negative row in a late chunk", [b"".join(negative)], 640, r"stream 0: cell 150 has a negative row"))
    out.append(("a negative row in a late chunk of the second source", [good, b"".join(negative)], 1280, r"stream 1: cell 150 has a negative row"))
    broken = bytearray(b"".join(cells))
    broken[50 * 64 + 16:50 * 64 + 24] = (7).to_bytes(8, "little")
    out.append(("a chain broken beyond the first chunk", [bytes(broken)], 640, r"stream 0: cell_size 7 at byte offset 3200 is smaller than a cell header"))
    whole = b"".join(cells)
    out.append(("a chain that runs past the end", [good, whole[:-1]], 1280, r"stream 1: the size chain runs past the end of the stream.*byte offset %d" % (199 * 64)))
    out.append(("a header cut by the end", [whole + b"\0" * 23], 640, r"stream 0: the size chain runs past the end of the stream: a cell header at byte offset 12800 of 12823 bytes"))
    return out
