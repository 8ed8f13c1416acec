"""The device importer on the same cells from two inputs: synthetic gVCF text (tests/tools/synth_gvcf_text.py, as import_bench.py
makes it) and the CSV cell file tests/tools/cells2csv.py prints of the cells that text gives.  Per input: wall clock of
import_cells (median of --runs runs after one warm-up), the HIP-event time per phase, bytes in and out, and measure + write time
per output byte.  Prints one JSON document.

    python tests/tools/import_csv_bench.py --files 100 --lines 5000 --distinct 8 --dir /tmp/import_csv_bench"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PHASES = ("ms_index", "ms_measure", "ms_write", "ms_sort_gather")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=100)
    ap.add_argument("--lines", type=int, default=5000)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/import_csv_bench")
    ap.add_argument("--budget", type=int, default=0)
    a = ap.parse_args()
    import cells2csv
    import genomicsdb_amd as gdb
    import import_bench
    t0 = time.time()
    v, c, text_bytes = import_bench.make_inputs(a.dir, a.files, a.lines, a.distinct)
    cells, ncells = gdb.import_cells(v, c, file_root=a.dir, device=0, text_budget_bytes=a.budget)        # (also the warm-up)
    t1 = time.time()
    csv = cells2csv.csv_text(cells, v).encode("latin-1")
    with open(os.path.join(a.dir, "cells.csv"), "wb") as f:
        f.write(csv)
    m = json.load(open(c))
    for cs in m["callsets"].values():
        cs["filename"] = "cells.csv"
    m["sorted_csv_files"] = ["cells.csv"]
    c_csv = os.path.join(a.dir, "callsets_csv.json")
    json.dump(m, open(c_csv, "w"))
    out = {"files": a.files, "lines_per_file": a.lines, "cells": ncells, "cell_bytes": len(cells), "vcf_text_bytes": text_bytes, "csv_bytes": len(csv),
           "seconds_generating_text": round(t1 - t0, 1), "seconds_printing_csv": round(time.time() - t1, 1), "text_budget_bytes": a.budget}
    for name, mapping in (("vcf_text", c), ("csv", c_csv)):
        gdb.import_cells(v, mapping, file_root=a.dir, device=0, text_budget_bytes=a.budget)
        secs, stats, same = [], [], True
        for _ in range(a.runs):
            st = {}
            t = time.perf_counter()
            got, _ = gdb.import_cells(v, mapping, file_root=a.dir, device=0, text_budget_bytes=a.budget, stats=st)
            secs.append(time.perf_counter() - t)
            stats.append(st)
            same = same and got == cells
        med = stats[secs.index(statistics.median_low(secs))]
        out[name] = {"seconds": [round(x, 3) for x in secs], "same_cells": same, "ms_per_phase_all_runs": [{k: round(s[k], 2) for k in PHASES} for s in stats],
                     "bytes_in": med["text_bytes"], "bytes_out": med["num_bytes"], "num_batches": med["num_batches"], "num_deferred_values": med["num_deferred_values"],
                     "measure_plus_write_ns_per_output_byte": round((med["ms_measure"] + med["ms_write"]) * 1e6 / med["num_bytes"], 4),
                     "s_read": round(med["s_read"], 3), "s_h2d": round(med["s_h2d"], 3), "s_deferred": round(med["s_deferred"], 3), "s_d2h": round(med["s_d2h"], 3)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
