"""The input histogram (input_histogram, kernels/gdb_histogram.hip) on the BGZF input of tests/tools/split_bench.py: every file counted in
one pass.  Per --bins value one warm-up run, then --runs timed runs; per run the statistics of input_histogram (the HIP-event time of
index / inflate / histogram, the wall seconds of read, H2D, total) and the wall clock around the Python call.  Then, once, the
plain-Python model (tests/tools/histogram_model.py) on the same files, which must give the same counts.  Prints one JSON document.

    python tests/tools/histogram_bench.py --files 64 --lines 50000 --distinct 8 --bins 16,1024,1048576 --dir /tmp/histogram_bench"""
import argparse
import json
import os
import shutil
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bgzf_write  # noqa: E402
import histogram_model  # noqa: E402
import import_bench  # noqa: E402
import synth_gvcf_text  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--lines", type=int, default=50000)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--bins", default="16,1024,1048576")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/histogram_bench")
    ap.add_argument("--budget", type=int, default=0)
    ap.add_argument("--member", type=int, default=65280)
    a = ap.parse_args()
    import genomicsdb_amd as gdb
    t0 = time.time()
    v, c, text_bytes = import_bench.make_inputs(a.dir, a.files, a.lines, a.distinct)
    gz_dir = os.path.join(a.dir, "bgzf")
    os.makedirs(gz_dir, exist_ok=True)
    for p in (v, c):
        shutil.copy(p, gz_dir)
    v, c = os.path.join(gz_dir, os.path.basename(v)), os.path.join(gz_dir, os.path.basename(c))
    gz_bytes = 0
    members = {}          # the files repeat the text of --distinct files behind their own header: equal members are deflated once
    for i in range(a.files):
        raw = open(os.path.join(a.dir, "s%04d.g.vcf" % i), "rb").read()
        p = os.path.join(gz_dir, "s%04d.g.vcf" % i)
        with open(p, "wb") as f:
            for at in range(0, len(raw), a.member):
                chunk = raw[at:at + a.member]
                if chunk not in members:
                    members[chunk] = bgzf_write.member(chunk)
                f.write(members[chunk])
            f.write(bgzf_write.EOF)
        gz_bytes += os.path.getsize(p)
    del members
    max_range = sum(length for _, _, length in synth_gvcf_text.CONTIGS) - 1
    out = {"files": a.files, "lines_per_file": a.lines, "text_bytes": text_bytes, "compressed_bytes_in": gz_bytes, "max_histogram_range": max_range,
           "seconds_generating": round(time.time() - t0, 1), "text_budget_bytes": a.budget, "runs": {}}
    last = None
    for num_bins in [int(x) for x in a.bins.split(",")]:
        def timed():
            st = {}
            t = time.perf_counter()
            counts = gdb.input_histogram(v, c, max_range, num_bins, file_root=gz_dir, text_budget_bytes=a.budget, stats=st)
            return time.perf_counter() - t, st, counts

        timed()               # warm-up: code objects, allocator, page cache
        runs = [timed() for _ in range(a.runs)]
        secs = [r[0] for r in runs]
        med = runs[secs.index(statistics.median_low(secs))][1]
        out["runs"][str(num_bins)] = {"wall_seconds": [round(x, 3) for x in secs], "stats_of_median_run": med, "ms_histogram_every_run": [r[1]["ms_histogram"] for r in runs],
                                      "ms_index_every_run": [r[1]["ms_index"] for r in runs], "ms_inflate_every_run": [r[1]["ms_inflate"] for r in runs],
                                      "per_batch_us": {k: round(1000.0 * med[k] / med["num_batches"], 2) for k in ("ms_histogram", "ms_index", "ms_inflate")},
                                      "nonzero_bins": int((runs[0][2] != 0).sum())}
        last = (num_bins, runs[0][2])
    t = time.perf_counter()
    want = histogram_model.histogram(v, c, gz_dir, max_range, last[0])
    out["python_model"] = {"num_bins": last[0], "wall_seconds": round(time.perf_counter() - t, 3), "equal_counts": want == last[1].tolist()}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
