"""Host importer against device importer on synthetic gVCF text (tests/tools/synth_gvcf_text.py), stored uncompressed so that
zlib is not what is timed.  Wall clock of import_cells per path (median and spread of --runs runs after one warm-up run of the
device path), the device path's HIP-event time per phase, the text rate of the measure + write kernels and the split of the
rest (file read, H2D, host parse of deferred tokens, sort + gather, D2H).  Prints one JSON document.

    python tests/tools/import_bench.py --files 200 --lines 50000 --distinct 8 --dir /tmp/import_bench
--distinct N: only N files are generated; the others repeat their record text under a sample name of their own."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def make_inputs(d, files, lines, distinct):
    import synth_gvcf_text as sg
    distinct = min(distinct, files)
    v, c = sg.write_inputs(d, n_files=distinct, n_lines=lines, multi=0)
    cs = json.load(open(c))["callsets"]
    texts = [open(os.path.join(d, "s%04d.g.vcf" % i)).read() for i in range(distinct)]
    for i in range(distinct, files):
        name, fn = "S%04d" % i, "s%04d.g.vcf" % i
        with open(os.path.join(d, fn), "w") as f:
            f.write(texts[i % distinct].replace("\tS%04d\n" % (i % distinct), "\t%s\n" % name, 1))
        cs[name] = {"row_idx": i, "idx_in_file": 0, "filename": fn}
    json.dump({"callsets": cs}, open(c, "w"))
    return v, c, sum(os.path.getsize(os.path.join(d, "s%04d.g.vcf" % i)) for i in range(files))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--lines", type=int, default=50000)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/import_bench")
    ap.add_argument("--budget", type=int, default=0)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    import genomicsdb_amd as gdb
    t0 = time.time()
    v, c, text_bytes = make_inputs(a.dir, a.files, a.lines, a.distinct)
    out = {"files": a.files, "lines_per_file": a.lines, "text_bytes": text_bytes, "seconds_generating": round(time.time() - t0, 1), "text_budget_bytes": a.budget}

    def timed(**kw):
        t = time.perf_counter()
        cells, n = gdb.import_cells(v, c, file_root=a.dir, **kw)
        return time.perf_counter() - t, cells, n

    host_cells = None
    if not a.skip_host:
        hs = []
        for _ in range(a.runs):
            s, host_cells, n = timed()
            hs.append(s)
        out["host"] = {"seconds": [round(x, 3) for x in hs], "median": round(statistics.median(hs), 3), "min": round(min(hs), 3), "max": round(max(hs), 3),
                       "cells": n, "bytes": len(host_cells), "text_MB_per_s": round(text_bytes / 1e6 / statistics.median(hs), 1)}
    timed(device=0, text_budget_bytes=a.budget)        # warm-up: code objects, allocator
    ds, stats = [], []
    for _ in range(a.runs):
        st = {}
        s, cells, n = timed(device=0, text_budget_bytes=a.budget, stats=st)
        ds.append(s)
        stats.append(st)
    med = stats[ds.index(statistics.median_low(ds))]
    kernel_s = (med["ms_measure"] + med["ms_write"]) / 1e3
    out["device"] = {"seconds": [round(x, 3) for x in ds], "median": round(statistics.median(ds), 3), "min": round(min(ds), 3), "max": round(max(ds), 3),
                     "cells": n, "bytes": len(cells), "identical_to_host": (cells == host_cells) if host_cells is not None else None,
                     "stats_of_median_run": med, "ms_per_phase_all_runs": [{k: round(s[k], 2) for k in ("ms_index", "ms_measure", "ms_write", "ms_sort_gather")} for s in stats],
                     "measure_plus_write_text_GB_per_s": round(text_bytes / 1e9 / kernel_s, 2) if kernel_s else None,
                     "index_text_GB_per_s": round(text_bytes / 1e6 / med["ms_index"], 2) if med["ms_index"] else None,
                     "seconds_not_accounted": round(med["s_total"] - med["s_read"] - med["s_h2d"] - med["s_deferred"] - med["s_d2h"]
                                                    - (med["ms_index"] + med["ms_measure"] + med["ms_write"] + med["ms_sort_gather"]) / 1e3, 3)}
    # A/B of the write kernel: cells stored directly against cells staged in LDS and stored as dwords
    ab = {}
    for flag in ("0", "1", "0", "1"):
        os.environ["GDBAMD_IMPORT_STAGE_LDS"] = flag
        st = {}
        s, cells2, _ = timed(device=0, text_budget_bytes=a.budget, stats=st)
        ab.setdefault("stage_in_lds=" + flag, []).append({"ms_write": round(st["ms_write"], 2), "seconds": round(s, 3), "same_bytes": cells2 == cells})
    os.environ.pop("GDBAMD_IMPORT_STAGE_LDS")
    out["write_kernel_ab"] = ab
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
