"""The windowed merge measured (profiles/device_merge_files.md): an array file plus a batch merged to a new array file, in the shape of
profiles/device_merge.md - by default 9 000 000 + 1 000 000 cells of 160 bytes, 1 440 MB + 160 MB, crafted here (rows 0..899 of
10 000 columns are the array, rows 900..999 the batch; the merge reads nothing but the headers, so the payload is a byte pattern).
Two routes, alternating in one call, files on one filesystem, the page cache warm for both:
  parent    what vcf2tiledb does without --merge-window-bytes: read the array file whole, merge_cells (merge_cell_streams_device), write
            the result.  Reported as wall clock of the Python calls and, without the copies behind the C ABI and ctypes that the tool
            does not pay, as read + the call's own s_total + write
  windowed  merge_cell_files(array file, batch bytes) at each window of --windows and at one round (a window that holds everything)
Prints one JSON document; per windowed run the statistics, from which the overlap follows: the host thread's s_read + s_write +
s_wait_device against s_total.

    python tests/tools/merge_files_bench.py --dir /tmp/merge_files_bench --runs 3"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def crafted(rows_lo, rows_hi, columns, cell_bytes):
    """cells of rows [rows_lo, rows_hi) at every column, in (column, row) order"""
    import numpy as np
    rows = rows_hi - rows_lo
    n = rows * columns
    cells = np.empty((n, cell_bytes // 8), dtype=np.int64)
    cells[:, 3:] = np.arange(n, dtype=np.int64)[:, None]
    cells[:, 0] = np.tile(np.arange(rows_lo, rows_hi, dtype=np.int64), columns)
    cells[:, 1] = np.repeat(np.arange(columns, dtype=np.int64), rows)
    cells[:, 2] = cell_bytes
    return cells.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--batch-rows", type=int, default=100)
    ap.add_argument("--columns", type=int, default=10000)
    ap.add_argument("--cell-bytes", type=int, default=160)
    ap.add_argument("--windows", default="67108864,268435456,1073741824")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/merge_files_bench")
    a = ap.parse_args()
    import genomicsdb_amd as gdb
    os.makedirs(a.dir, exist_ok=True)
    array_file, out_file = os.path.join(a.dir, "cells.bin"), os.path.join(a.dir, "cells.new.bin")
    cut = a.rows - a.batch_rows
    batch = crafted(cut, a.rows, a.columns, a.cell_bytes)
    with open(array_file, "wb") as f:
        f.write(crafted(0, cut, a.columns, a.cell_bytes))
    array_bytes = os.path.getsize(array_file)
    out = {"array_bytes": array_bytes, "batch_bytes": len(batch), "cell_bytes": a.cell_bytes, "cells": a.rows * a.columns, "runs": a.runs}
    windows = [int(w) for w in a.windows.split(",") if w] + [2 * (array_bytes + len(batch)) + 4096]      # the last: one round

    def timed(fn):
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r

    def parent():
        st = {}
        t_read, old = timed(lambda: open(array_file, "rb").read())
        t_merge, (merged, n) = timed(lambda: gdb.merge_cells([old, batch], stats=st))
        del old

        def write():
            with open(out_file, "wb") as f:
                f.write(merged)
        t_write, _ = timed(write)
        return {"wall": t_read + t_merge + t_write, "read": t_read, "merge_call": t_merge, "write": t_write, "merge_s_total": st["s_total"],
                "without_abi_copies": t_read + st["s_total"] + t_write, "stats": st}, merged

    def windowed(window):
        st = {}
        try:
            t, n = timed(lambda: gdb.merge_cell_files([array_file, batch], out_file, window_bytes=window, stats=st))
        except gdb.GenomicsDBException as e:      # (a window whose buffers the device or the pinned memory cannot hold)
            return {"wall": -1.0, "error": str(e)[:300]}
        host = st["s_read"] + st["s_write"] + st["s_wait_device"]
        return {"wall": t, "host_busy_or_waiting": host, "wait_device_share": st["s_wait_device"] / st["s_total"] if st["s_total"] else 0.0, "stats": st}

    # warm-up of both routes (code objects, allocator, page cache), and the bytes compared once
    _, want = parent()
    windowed(windows[0])
    with open(out_file, "rb") as f:
        out["identical_to_in_core"] = f.read() == want
    del want
    runs = {"parent": []}
    for w in windows:
        runs["windowed_%d" % w] = []
    for _ in range(a.runs):      # alternating
        runs["parent"].append(parent()[0])
        for w in windows:
            runs["windowed_%d" % w].append(windowed(w))
    for name, rs in runs.items():
        walls = [r["wall"] for r in rs]
        med = rs[walls.index(statistics.median_low(walls))]
        out[name] = {"wall_seconds": [round(x, 3) for x in walls], "wall_median": round(statistics.median(walls), 3), "median_run": med}
    out["parent"]["without_abi_copies_median"] = round(statistics.median(r["without_abi_copies"] for r in runs["parent"]), 3)
    os.remove(out_file)
    os.remove(array_file)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
