"""The device splitter (split_files, kernels/gdb_split.hip) on the BGZF input of tests/tools/import_gz_bench.py: every file cut into
--partitions column partitions in one pass.  One warm-up run, then --runs timed runs; per run the statistics of split_files (the
HIP-event time of index / classify / scan + gather / deflate / inflate, the wall seconds of read, H2D, D2H + write, .tbi build) and the
wall clock around the Python call.  Then, on the same files, one warm-up and one timed run of the device importer for its inflate
and index phases (the kernels the splitter shares with it).  Prints one JSON document.

    python tests/tools/split_bench.py --files 200 --lines 50000 --distinct 8 --partitions 8 --dir /tmp/split_bench"""
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
import import_bench  # noqa: E402
import synth_gvcf_text  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--lines", type=int, default=50000)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--partitions", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/split_bench")
    ap.add_argument("--budget", type=int, default=0)
    ap.add_argument("--level", type=int, default=6)
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
                    members[chunk] = bgzf_write.member(chunk, level=a.level)
                f.write(members[chunk])
            f.write(bgzf_write.EOF)
        gz_bytes += os.path.getsize(p)
    del members
    total = sum(length for _, _, length in synth_gvcf_text.CONTIGS)
    begins = [k * total // a.partitions for k in range(a.partitions)]
    parts = [(b, (begins[k + 1] - 1) if k + 1 < len(begins) else 2 ** 63 - 2) for k, b in enumerate(begins)]
    out = {"files": a.files, "lines_per_file": a.lines, "text_bytes": text_bytes, "compressed_bytes_in": gz_bytes, "level": a.level, "member_payload": a.member,
           "partitions": parts, "seconds_generating": round(time.time() - t0, 1), "text_budget_bytes": a.budget}
    res = os.path.join(a.dir, "split")

    def timed():
        shutil.rmtree(res, ignore_errors=True)
        os.makedirs(res)
        st = {}
        t = time.perf_counter()
        done = gdb.split_files(v, c, parts, results_directory=res, file_root=gz_dir, text_budget_bytes=a.budget, stats=st)
        return time.perf_counter() - t, st, len(done)

    timed()               # warm-up: code objects, allocator, page cache
    runs = [timed() for _ in range(a.runs)]
    secs = [r[0] for r in runs]
    med = runs[secs.index(statistics.median_low(secs))][1]
    gb = text_bytes / 1e9

    def rate_ms(ms):
        return round(text_bytes / 1e6 / ms, 2) if ms else None

    out["split"] = {"outputs": runs[0][2], "wall_seconds": [round(x, 3) for x in secs], "median": round(statistics.median(secs), 3), "stats_of_median_run": med,
                    "stats_of_every_run": [r[1] for r in runs],
                    "derived_input_text_GB_per_s": {"wall": round(gb / statistics.median(secs), 3), "inflate_kernel": rate_ms(med["ms_inflate"]), "index": rate_ms(med["ms_index"]),
                                                    "classify": rate_ms(med["ms_classify"]), "scan_gather": rate_ms(med["ms_scan_gather"]), "deflate": rate_ms(med["ms_deflate"])},
                    "derived_compression_ratio_text_out_over_compressed_out": round(med["text_bytes_out"] / med["compressed_bytes_out"], 3)}

    def imported():
        st = {}
        t = time.perf_counter()
        gdb.import_cells(v, c, file_root=gz_dir, device=0, text_budget_bytes=a.budget, stats=st)
        return time.perf_counter() - t, st

    imported()
    t, st = imported()
    out["device_importer_same_files"] = {"wall_seconds": round(t, 3), "ms_inflate": st["ms_inflate"], "ms_index": st["ms_index"], "num_batches": st["num_batches"],
                                         "derived_input_text_GB_per_s": {"inflate_kernel": rate_ms(st["ms_inflate"]), "index": rate_ms(st["ms_index"])}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
