"""Device importer on bgzip'ed input: inflate on the device against inflate on the host (inflate="host" is the behaviour before
the device inflater: a single-threaded zlib read of every file, then the upload of its text).  The input of
tests/tools/import_bench.py, written as BGZF (tests/tools/bgzf_write.py: level 6, members of 65 280 bytes).  One warm-up run of
each leg, then --runs timed runs of each, alternating; the cells of every run are compared with the first.  Per leg: wall
clock, s_read (file read + host inflate), input bytes uploaded to the device (the bytes_h2d statistic: text for the host leg;
compressed members, their descriptors and the header member's tail for the device leg), the inflate kernel's HIP-event time and the rate of inflated text.  Then the A/B of
the two inflate kernels (GDBAMD_INFLATE_KERNEL = wave | thread).  Prints one JSON document.

    python tests/tools/import_gz_bench.py --files 200 --lines 50000 --distinct 8 --dir /tmp/import_gz_bench"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--lines", type=int, default=50000)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/import_gz_bench")
    ap.add_argument("--budget", type=int, default=0)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--member", type=int, default=65280)
    a = ap.parse_args()
    import genomicsdb_amd as gdb
    t0 = time.time()
    v, c, text_bytes = import_bench.make_inputs(a.dir, a.files, a.lines, a.distinct)
    gz_dir = os.path.join(a.dir, "bgzf")          # the BGZF copies live next to the text files, under the same names
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
    out = {"files": a.files, "lines_per_file": a.lines, "text_bytes": text_bytes, "compressed_bytes": gz_bytes, "level": a.level, "member_payload": a.member,
           "seconds_generating": round(time.time() - t0, 1), "text_budget_bytes": a.budget}

    def timed(inflate):
        st = {}
        t = time.perf_counter()
        cells, n = gdb.import_cells(v, c, file_root=gz_dir, device=0, text_budget_bytes=a.budget, stats=st, inflate=inflate)
        return time.perf_counter() - t, cells, n, st

    def leg(runs):
        secs = [r[0] for r in runs]
        med = runs[secs.index(statistics.median_low(secs))][3]
        return {"seconds": [round(x, 3) for x in secs], "median": round(statistics.median(secs), 3), "min": round(min(secs), 3), "max": round(max(secs), 3),
                "spread": round(max(secs) - min(secs), 3), "s_read": [round(r[3]["s_read"], 3) for r in runs], "s_h2d": [round(r[3]["s_h2d"], 3) for r in runs],
                "ms_inflate": [round(r[3]["ms_inflate"], 2) for r in runs],
                "bytes_h2d": med["bytes_h2d"],
                "inflated_text_GB_per_s_wall": round(text_bytes / 1e9 / statistics.median(secs), 3),
                "inflate_kernel_text_GB_per_s": round(text_bytes / 1e6 / med["ms_inflate"], 2) if med["ms_inflate"] else None,
                "stats_of_median_run": med}

    legs = {"host": [], "device": []}
    _, ref_cells, n_cells, _ = timed("host")       # warm-up of each leg: code objects, allocator, page cache
    timed("device")
    same = True
    for _ in range(a.runs):
        for name in ("host", "device"):
            r = timed(name)
            same = same and r[1] == ref_cells
            legs[name].append(r)
    out["cells"] = n_cells
    out["cell_bytes"] = len(ref_cells)
    out["same_bytes_every_run"] = same
    out["inflate_on_host"] = leg(legs["host"])
    out["inflate_on_device"] = leg(legs["device"])
    h, d = out["inflate_on_host"], out["inflate_on_device"]
    out["device_leg_wins_by_s"] = round(h["median"] - d["median"], 3)
    out["host_leg_spread_s"] = h["spread"]
    # A/B of the inflate kernel: one wavefront per member against one thread per member, the same bodies
    ab = {}
    for kernel in ("wave", "thread", "wave", "thread", "wave", "thread"):
        os.environ["GDBAMD_INFLATE_KERNEL"] = kernel
        s, cells, _, st = timed("device")
        ab.setdefault(kernel, []).append({"ms_inflate": round(st["ms_inflate"], 2), "seconds": round(s, 3), "same_bytes": cells == ref_cells})
    os.environ.pop("GDBAMD_INFLATE_KERNEL")
    out["inflate_kernel_ab"] = ab
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
