"""The index of the "z" / "b" query stream built on the device (kernels/gdb_output_index.hip), measured.  Prints one JSON document.

Per format, on one window of the synthetic workload of bench.py (--samples x --window bp):
  stream   positions/s from the stream's init to its last byte read, index off and index on alternating in this one process, --runs
           each after one warm-up.  The margin for "index on is no slower" is twice the spread among the index-off runs.
  index    one more index-on run whose bytes go to a file: write_index wall time and the summed per-page phases, beside the wall time
           of the host builder (gdbamd_build_output_index) on that file; the two index files must be equal.
  hbm      bytes of device memory the record tables held.

    python tests/tools/output_index_bench.py --samples 1000 --window 1000000 --dir /tmp/output_index_bench"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--window", type=int, default=1_000_000)
    ap.add_argument("--begin", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--formats", default="z,b")
    ap.add_argument("--dir", default="/tmp/output_index_bench")
    ap.add_argument("--no-host", action="store_true", help="leave the host builder out (it re-reads the whole file on one core)")
    a = ap.parse_args()
    import torch
    import genomicsdb_amd as gdb
    from genomicsdb_amd import _lib, synth
    import helpers
    os.makedirs(a.dir, exist_ok=True)
    N, B, W = a.samples, a.begin, a.window
    fasta = os.path.join(a.dir, "synth_ref.fa")
    with open(fasta, "wb") as f:
        f.write(b">1\n" + b"N" * B + synth.reference(B, W + 4096) + b"\n")
    q = helpers.synth_query(a.dir, N, B, B + W - 1)
    q["reference_genome"] = fasta
    t0 = time.time()
    gen = synth.Generator(N, B, W)
    ptr, nbytes, ncells = gen.next_chunk(B + W)
    out = {"samples": N, "window_bp": W, "cells": int(ncells), "cell_bytes": int(nbytes), "seconds_generating": round(time.time() - t0, 1), "formats": {}}
    cap = 256 << 20
    dst = torch.empty(cap, dtype=torch.uint8, pin_memory=True)

    def run(fmt, index, path=None):
        t = time.perf_counter()
        s = gdb.GenomicsDBQueryStream(query_json=q, cells=(ptr, nbytes), buffer_capacity=1 << 20, output_format=fmt, index=index)
        t_init = time.perf_counter() - t
        total = 0
        reads = []      # seconds of every read call: where a stall sits
        f = open(path, "wb") if path else None
        while True:
            t_r = time.perf_counter()
            got = s.read_into(dst.data_ptr(), cap)
            reads.append(round(time.perf_counter() - t_r, 4))
            if got <= 0:
                break
            total += got
            if f:
                f.write(memoryview(dst.numpy())[:got])
        secs = time.perf_counter() - t
        if f:
            f.close()
        r = {"seconds_init_to_last_byte": round(secs, 4), "seconds_init": round(t_init, 4), "seconds_per_read": reads, "bytes": total, "device_pages": int(s.stream_stats().pages)}
        if index:
            t = time.perf_counter()
            st = s.write_index((path or os.path.join(a.dir, "timed." + fmt)) + ".dev")
            r["write_index_wall_seconds"] = round(time.perf_counter() - t, 4)
            r["index"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in st.items()}
        s.close()
        return r

    for fmt in a.formats.split(","):
        run(fmt, True)      # warm-up: code objects, allocator, arenas
        runs = {"off": [], "on": []}
        for _ in range(a.runs):
            runs["off"].append(run(fmt, False))
            runs["on"].append(run(fmt, True))
        records = runs["on"][0]["index"]["records"]
        rate = {k: [records / r["seconds_init_to_last_byte"] for r in rs] for k, rs in runs.items()}
        spread_off = max(rate["off"]) - min(rate["off"])
        med = {k: sorted(v)[len(v) // 2] for k, v in rate.items()}
        res = {"records": records, "runs": runs, "positions_per_sec": {k: [round(x) for x in v] for k, v in rate.items()},
               "median_positions_per_sec": {k: round(v) for k, v in med.items()}, "spread_among_index_off_runs": round(spread_off),
               "margin_twice_the_spread": round(2 * spread_off), "index_on_below_off_by": round(med["off"] - med["on"]),
               "index_on_within_margin": med["off"] - med["on"] <= 2 * spread_off}
        path = os.path.join(a.dir, "out." + fmt)
        last = run(fmt, True, path)
        ix = last["index"]
        res["file_bytes"] = os.path.getsize(path)
        res["index_cost"] = {"write_index_wall_seconds": last["write_index_wall_seconds"],
                             "ms_per_page_phases_summed": round(ix["ms_records"] + ix["ms_voff"] + ix["ms_chunks"] + ix["ms_linear"], 3),
                             "ms_records": ix["ms_records"], "ms_voff": ix["ms_voff"], "ms_chunks": ix["ms_chunks"], "ms_linear": ix["ms_linear"], "s_write": ix["s_write"]}
        res["hbm_table_bytes"] = ix["table_bytes"]
        res["hbm_table_bytes_per_record_of_the_largest_page"] = None if not ix["pages"] else round(ix["table_bytes"] / max(1, ix["records"] / ix["pages"]), 1)
        if not a.no_host:
            t = time.perf_counter()
            assert _lib.lib().gdbamd_build_output_index(os.fsencode(path), int(fmt == "b")) == 0, _lib.last_error()
            res["host_builder_wall_seconds"] = round(time.perf_counter() - t, 3)
            res["equal_files"] = open(path + ".dev", "rb").read() == open(path + (".csi" if fmt == "b" else ".tbi"), "rb").read()
        out["formats"][fmt] = res
        print(json.dumps({fmt: res}), flush=True)
    gen.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
