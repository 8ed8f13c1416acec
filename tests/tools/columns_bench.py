"""The column decoder (CombineEngine.record_tensors, kernels/gdb_columns.hip) on the c2 window of bench.py: --samples samples x --window-bp columns
of the synthetic array, an engine with output format "bu", fields GT int8, DP int16, GQ int16.  One warm-up pass, then --runs timed ones; per pass
the statistics of gdbamd_columns_stats summed over the window's pages (HIP-event time of measure, site and scatter, bytes read and written).
Beside them, in the same process: the page kernel's time for the same window (ms_write_kernel_avg of run_interval, k_bcf_write) and a
device-to-device torch copy_ that moves as many bytes as the decoder read and wrote together.  Prints one JSON document.

    python tests/tools/columns_bench.py --samples 1000 --window-bp 1000000 --runs 5"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIELDS = {"GT": "int8", "DP": "int16", "GQ": "int16"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--window-bp", type=int, default=1_000_000)
    ap.add_argument("--base", type=int, default=10_000_000)
    ap.add_argument("--arena-mb", type=int, default=49152)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import torch
    import helpers
    import genomicsdb_amd
    from genomicsdb_amd import synth
    N, B, W, arena = a.samples, a.base, a.window_bp, a.arena_mb << 20
    q = helpers.synth_query(tempfile.mkdtemp(prefix="gdbamd_columns_bench_"), N, B, B + W - 1)
    eng = genomicsdb_amd.CombineEngine(q, output_format="bu")
    t0 = time.time()
    gen = synth.Generator(N, B, W)
    eng.stage_cells_begin()
    ptr, nbytes, ncells = gen.next_chunk(B + W, nthreads=min(16, os.cpu_count() or 1))
    eng.stage_cells_append(ptr, nbytes)
    eng.stage_cells_end()
    eng.set_reference(B, synth.reference(B, W + 4096))
    out = {"samples": N, "window_bp": W, "cells": ncells, "fields": FIELDS, "seconds_generating_and_staging": round(time.time() - t0, 1), "runs": []}

    def decode():
        st, shapes = [], {}
        for page in eng.record_tensors(B, B + W - 1, fields=FIELDS, arena_bytes=arena, stats=st):
            shapes = {k: list(v.shape) for k, v in page.items()}
        tot = {k: sum(s[k] for s in st) for k in ("records", "bytes_read", "bytes_written", "ms_measure", "ms_site", "ms_scatter")}
        tot["pages"], tot["width"], tot["shapes_of_last_page"] = len(st), st[-1]["width"], shapes
        return tot

    decode()
    out["runs"] = [decode() for _ in range(a.runs)]
    total = [r["ms_measure"] + r["ms_site"] + r["ms_scatter"] for r in out["runs"]]
    med = out["runs"][total.index(statistics.median_low(total))]
    out["median_run"] = dict(med)
    for r in out["runs"]:
        r.pop("shapes_of_last_page")      # (the same in every run: kept in median_run)
    # the page kernel of the same window, same process
    writes = []
    for _ in range(a.runs):
        _, st = eng.run_interval(B, B + W - 1, arena_bytes=arena, fetch=False)
        writes.append({"ms_write_kernel_avg": st.ms_write_kernel_avg, "ms_write": st.ms_write, "ms_total": st.ms_total, "pages": st.pages, "bytes_out": st.bytes_out,
                       "num_records": st.num_records})
    out["page_kernel_runs"] = writes
    # the yardstick of profiles/device_merge.md: a device-to-device copy that moves the same number of bytes (n read + n written)
    n = (med["bytes_read"] + med["bytes_written"]) // 2
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    src.zero_()
    dst.copy_(src)
    copies = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        copies.append(e0.elapsed_time(e1))
    out["copy"] = {"bytes_each_way": n, "ms": copies}
    ms_copy, ms_dec = statistics.median_low(copies), med["ms_measure"] + med["ms_site"] + med["ms_scatter"]
    out["summary"] = {"ms_decoder": ms_dec, "ms_copy_of_the_same_bytes": ms_copy, "decoder_over_copy": ms_dec / ms_copy,
                      "ms_k_bcf_write": statistics.median_low([w["ms_write_kernel_avg"] for w in writes]),
                      "decoder_gb_per_s": (med["bytes_read"] + med["bytes_written"]) / ms_dec / 1e6}
    eng.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
