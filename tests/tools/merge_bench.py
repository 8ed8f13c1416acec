"""Incremental import measured (profiles/device_merge.md): a batch of samples merged into an array on the device
(merge_cells, csrc/kernels/gdb_merge.hip) against the only alternative before it, importing every sample again, on synthetic
gVCF text (tests/tools/synth_gvcf_text.py through import_bench.make_inputs).  Per-phase HIP-event times of the merge, the rate of
the gather against a device-to-device copy of the same bytes (torch), wall clock of both routes; optionally the cost of ranking the
same keys by the importer's radix-sort route (tests/tools/microbench/merge_rank_radix, a scratch program).  Prints one JSON document.

    python tests/tools/merge_bench.py --files 1000 --batch 100 --lines 10000 --distinct 8 --dir /tmp/merge_bench"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--lines", type=int, default=10000)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default="/tmp/merge_bench")
    ap.add_argument("--radix-program", default="")
    a = ap.parse_args()
    import torch
    import genomicsdb_amd as gdb
    import import_bench
    os.makedirs(a.dir, exist_ok=True)
    t0 = time.time()
    v, c, text_bytes = import_bench.make_inputs(a.dir, a.files, a.lines, a.distinct)
    out = {"files": a.files, "batch_files": a.batch, "lines_per_file": a.lines, "distinct": a.distinct, "text_bytes": text_bytes,
           "seconds_generating": round(time.time() - t0, 1)}
    cut = a.files - a.batch

    def timed(fn):
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r

    gdb.import_cells(v, c, file_root=a.dir, device=0, lb_callset_row_idx=cut)        # warm-up: code objects, allocator
    # the alternative on the parent commit: every sample again
    secs, whole = [], None
    for _ in range(3):
        s, (whole, n_whole) = timed(lambda: gdb.import_cells(v, c, file_root=a.dir, device=0))
        secs.append(s)
    out["reimport_all"] = {"seconds": [round(x, 3) for x in secs], "median": round(statistics.median(secs), 3), "cells": n_whole, "bytes": len(whole)}
    s_arr, (array, n_array) = timed(lambda: gdb.import_cells(v, c, file_root=a.dir, device=0, ub_callset_row_idx=cut - 1))
    secs = []
    for _ in range(3):
        s, (batch, n_batch) = timed(lambda: gdb.import_cells(v, c, file_root=a.dir, device=0, lb_callset_row_idx=cut))
        secs.append(s)
    out["import_batch"] = {"seconds": [round(x, 3) for x in secs], "median": round(statistics.median(secs), 3), "cells": n_batch, "bytes": len(batch)}
    out["array"] = {"cells": n_array, "bytes": len(array), "seconds_importing": round(s_arr, 3)}
    gdb.merge_cells([array, batch])        # warm-up
    runs, walls = [], []
    for _ in range(a.runs):
        st = {}
        s, (merged, n) = timed(lambda: gdb.merge_cells([array, batch], stats=st))
        walls.append(s)
        runs.append(st)
    moved = 2 * len(merged)        # the gather reads and writes every byte once
    med = runs[walls.index(statistics.median_low(walls))]
    out["merge"] = {"identical_to_reimport": merged == whole, "cells": n, "bytes": len(merged), "wall_seconds": [round(x, 3) for x in walls],
                    "wall_median": round(statistics.median(walls), 3), "stats_of_median_run": med,
                    "ms_per_phase_all_runs": [{k: round(r[k], 3) for k in ("ms_keys", "ms_rank", "ms_scan", "ms_gather")} for r in runs],
                    "gather_GB_per_s": round(moved / 1e6 / med["ms_gather"], 1), "all_kernels_GB_per_s":
                    round(moved / 1e6 / (med["ms_keys"] + med["ms_rank"] + med["ms_scan"] + med["ms_gather"]), 1)}
    out["merge_plus_batch_import_wall"] = round(out["merge"]["wall_median"] + out["import_batch"]["median"], 3)
    # the bound of the gather: the same bytes, device to device
    src = torch.empty(len(merged), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    out["device_to_device_copy"] = {"ms": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3), "GB_per_s": round(moved / 1e6 / statistics.median(ms), 1)}
    out["gather_over_copy"] = round(med["ms_gather"] / statistics.median(ms), 2)
    del src, dst
    if a.radix_program:
        fa, fb = os.path.join(a.dir, "array.bin"), os.path.join(a.dir, "batch.bin")
        open(fa, "wb").write(array)
        open(fb, "wb").write(batch)
        r = subprocess.run([a.radix_program, fa, fb, str(a.runs)], capture_output=True, timeout=300)
        out["radix_route"] = json.loads(r.stdout.decode()) if r.returncode == 0 else {"error": r.stderr.decode()[-500:], "rc": r.returncode}
        os.remove(fa)
        os.remove(fb)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
