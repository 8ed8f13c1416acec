"""The device tabix builder (kernels/gdb_index.hip) measured two ways.  Prints one JSON document.

splitter    the input and partitions of tests/tools/split_bench.py (profiles/device_split.md): every file cut into --partitions column
            partitions.  One warm-up, then --runs runs with the host index builder and --runs with the device builder, alternating, in
            this one process: wall clock, s_index_build and ms_index_kernels of every run.
standalone  one file of that set, its record text repeated until it holds --standalone-gb of text: index_vcf against
            gdbamd_build_output_index, --runs runs each, alternating; the two .tbi files must be equal.

    python tests/tools/index_bench.py --files 200 --lines 50000 --distinct 8 --partitions 8 --dir /tmp/index_bench"""
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


def bgzf_file(path, pieces, member, level):
    """pieces: byte strings, each cut into members of its own, so that a repeated piece is deflated once"""
    cache = {}
    with open(path, "wb") as f:
        for piece in pieces:
            for at in range(0, len(piece), member):
                chunk = piece[at:at + member]
                if chunk not in cache:
                    cache[chunk] = bgzf_write.member(chunk, level=level)
                f.write(cache[chunk])
        f.write(bgzf_write.EOF)
    return os.path.getsize(path)


def spread(xs):
    return round(max(xs) - min(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--lines", type=int, default=50000)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--partitions", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/index_bench")
    ap.add_argument("--budget", type=int, default=0)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--member", type=int, default=65280)
    ap.add_argument("--standalone-gb", type=float, default=1.0)
    a = ap.parse_args()
    import genomicsdb_amd as gdb
    from genomicsdb_amd import _lib
    t0 = time.time()
    v, c, text_bytes = import_bench.make_inputs(a.dir, a.files, a.lines, a.distinct)
    gz_dir = os.path.join(a.dir, "bgzf")
    os.makedirs(gz_dir, exist_ok=True)
    for p in (v, c):
        shutil.copy(p, gz_dir)
    v, c = os.path.join(gz_dir, os.path.basename(v)), os.path.join(gz_dir, os.path.basename(c))
    gz_bytes = 0
    members = {}
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
    out = {"files": a.files, "lines_per_file": a.lines, "text_bytes": text_bytes, "compressed_bytes_in": gz_bytes, "partitions": parts, "text_budget_bytes": a.budget,
           "seconds_generating": round(time.time() - t0, 1)}
    res = os.path.join(a.dir, "split")

    def split(on):
        shutil.rmtree(res, ignore_errors=True)
        os.makedirs(res)
        st = {}
        t = time.perf_counter()
        done = gdb.split_files(v, c, parts, results_directory=res, file_root=gz_dir, text_budget_bytes=a.budget, stats=st, index_on_device=on)
        return {"wall_seconds": round(time.perf_counter() - t, 3), "s_index_build": round(st["s_index_build"], 4), "ms_index_kernels": round(st["ms_index_kernels"], 3),
                "s_d2h_write": round(st["s_d2h_write"], 4), "s_total": round(st["s_total"], 4), "outputs": len(done)}

    split(True)               # warm-up: code objects, allocator, page cache
    runs = {"host": [], "device": []}
    for _ in range(a.runs):
        runs["host"].append(split(False))
        runs["device"].append(split(True))
    summary = {}
    for k, rs in runs.items():
        summary[k] = {m: {"median": statistics.median(r[m] for r in rs), "spread": spread([r[m] for r in rs])} for m in ("wall_seconds", "s_index_build", "ms_index_kernels")}
    gap = summary["host"]["s_index_build"]["median"] - summary["device"]["s_index_build"]["median"]
    out["splitter"] = {"runs": runs, "summary": summary,
                       "device_s_index_build_below_host_by_more_than_the_spread": gap > max(summary["host"]["s_index_build"]["spread"], summary["device"]["s_index_build"]["spread"])}

    # ---- standalone: one file, its records repeated
    raw = open(os.path.join(a.dir, "s0000.g.vcf"), "rb").read()
    head_end = raw.find(b"\n", raw.find(b"#CHROM")) + 1
    head, body = raw[:head_end], raw[head_end:]
    reps = max(1, int(a.standalone_gb * 1e9 / len(body)) + 1)
    big = os.path.join(a.dir, "big.vcf.gz")
    t0 = time.time()
    big_bytes = bgzf_file(big, [head] + [body] * reps, a.member, a.level)
    copy = os.path.join(a.dir, "big_copy.vcf.gz")
    shutil.copy(big, copy)
    L = _lib.lib()
    sa = {"text_bytes": len(head) + reps * len(body), "compressed_bytes": big_bytes, "repeats": reps, "seconds_generating": round(time.time() - t0, 1), "host": [], "device": []}

    def host_once():
        t = time.perf_counter()
        assert L.gdbamd_build_output_index(os.fsencode(copy), 0) == 0, _lib.last_error()
        return round(time.perf_counter() - t, 3)

    def device_once():
        st = {}
        t = time.perf_counter()
        gdb.index_vcf(big, text_budget_bytes=a.budget, stats=st)
        st = {k: (round(x, 4) if isinstance(x, float) else x) for k, x in st.items()}
        st["wall_seconds"] = round(time.perf_counter() - t, 3)
        return st

    device_once()             # warm-up
    for _ in range(a.runs):
        sa["host"].append(host_once())
        sa["device"].append(device_once())
    sa["equal_files"] = open(big + ".tbi", "rb").read() == open(copy + ".tbi", "rb").read()
    sa["median_wall_seconds"] = {"host": statistics.median(sa["host"]), "device": statistics.median(r["wall_seconds"] for r in sa["device"])}
    out["standalone"] = sa
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
