"""BCF2 input of the device importer against the same records as VCF text: three legs that alternate in one process -
uncompressed BCF2 through streams=, plain text through the device text importer, the host importer on the text - one warm-up
round and --runs timed rounds, the bytes compared every run.  Input: tests/tools/synth_gvcf_text.py, encoded by
tests/tools/vcf2bcf.py (--distinct files are generated and encoded, the others repeat a distinct file under a sample name of their
own, which has the same length, so the encoded stream is patched in place).  Prints one JSON document: wall clock per leg, the
HIP-event ms of index / measure / write, record bytes per second, the spread.

    python tests/tools/import_bcf_bench.py --files 32 --lines 20000 --distinct 4 --dir /tmp/import_bcf_bench"""
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
    import vcf2bcf
    distinct = min(distinct, files)
    v, c = sg.write_inputs(d, n_files=distinct, n_lines=lines, multi=0)
    vid = json.load(open(v))
    cs = json.load(open(c))["callsets"]
    texts = [open(os.path.join(d, "s%04d.g.vcf" % i), "rb").read() for i in range(distinct)]
    bcfs = [vcf2bcf.encode(t, vid=vid)[0] for t in texts]
    streams = {}
    for i in range(files):
        name, fn = "S%04d" % i, "s%04d.g.vcf" % i
        old = b"\tS%04d\n" % (i % distinct)
        if i >= distinct:
            with open(os.path.join(d, fn), "wb") as f:
                f.write(texts[i % distinct].replace(old, b"\t%s\n" % name.encode(), 1))
            cs[name] = {"row_idx": i, "idx_in_file": 0, "filename": fn}
        streams[fn] = bcfs[i % distinct].replace(old, b"\t%s\n" % name.encode(), 1)
    json.dump({"callsets": cs}, open(c, "w"))
    text_bytes = sum(os.path.getsize(os.path.join(d, "s%04d.g.vcf" % i)) for i in range(files))
    record_bytes = sum(len(s) - 9 - int.from_bytes(s[5:9], "little") for s in streams.values())
    return v, c, streams, text_bytes, record_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--lines", type=int, default=20000)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/import_bcf_bench")
    a = ap.parse_args()
    import genomicsdb_amd as gdb
    t0 = time.time()
    v, c, streams, text_bytes, record_bytes = make_inputs(a.dir, a.files, a.lines, a.distinct)
    out = {"files": a.files, "lines_per_file": a.lines, "distinct": a.distinct, "text_bytes": text_bytes, "bcf_record_bytes": record_bytes,
           "seconds_generating_and_encoding": round(time.time() - t0, 1)}
    legs = {"bcf_streams": dict(device=0, streams=streams, file_root="/nonexistent"), "text_device": dict(device=0, file_root=a.dir), "host": dict(file_root=a.dir)}
    res = {k: {"seconds": [], "stats": []} for k in legs}
    ref = None
    for rnd in range(a.runs + 1):       # round 0 warms up: code objects, allocator, page cache
        for leg, kw in legs.items():
            st = {}
            if "device" in kw:
                kw = dict(kw, stats=st)
            t = time.perf_counter()
            cells, n = gdb.import_cells(v, c, **kw)
            s = time.perf_counter() - t
            ref = cells if ref is None else ref
            if cells != ref:
                raise SystemExit("leg %s, round %d: the cells differ from the first leg's" % (leg, rnd))
            if rnd:
                res[leg]["seconds"].append(round(s, 4))
                res[leg]["stats"].append(st)
    out["cells"], out["cell_bytes"] = n, len(ref)
    for leg, r in res.items():
        med = statistics.median(r["seconds"])
        r.update(median=med, min=min(r["seconds"]), max=max(r["seconds"]))
        in_bytes = record_bytes if leg == "bcf_streams" else text_bytes
        r["input_MB_per_s"] = round(in_bytes / 1e6 / med, 1)
        if r["stats"][0]:
            st = r["stats"][r["seconds"].index(statistics.median_low(r["seconds"]))]
            r["stats_of_median_run"] = st
            r["ms_per_phase_all_runs"] = [{k: round(s[k], 3) for k in ("ms_index", "ms_measure", "ms_write", "ms_sort_gather")} for s in r["stats"]]
            kernel_ms = st["ms_index"] + st["ms_measure"] + st["ms_write"]
            r["index_measure_write_input_GB_per_s"] = round(in_bytes / 1e6 / kernel_ms, 2) if kernel_ms else None
        del r["stats"]
    out["legs"] = res
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
