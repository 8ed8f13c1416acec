"""The measurement of profiles/device_import_stream.md: a streamed import (StreamImporter, capacities 64 KiB and 16 MiB) against the
whole-stream import (import_cells(device=0, streams=...)) of the same bytes, the seeded synthetic gVCFs of tests/test_import_device.py
with every stream's records in column order.  Needs a GPU.  python tests/tools/stream_import_bench.py -> one JSON document"""
import json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import genomicsdb_amd as gdb
import stream_import_inputs as sii
import synth_gvcf_text

d = tempfile.mkdtemp()
v, c = synth_gvcf_text.write_inputs(d, n_files=6, n_lines=2000, multi=3)
sources, rows_of = sii.mapping_sources(c, root=d)
# (the generator writes contig 2 in front of contig 1; a stream cannot go back, so every stream's records are put in column order)
offsets = sii.contig_offsets(v)
def in_column_order(text):
    head, recs = sii.split_text(text)
    return head + b"".join(sorted(recs, key=lambda l: sii.column_of(l, offsets)))
sources = [(n_, in_column_order(t)) for n_, t in sources]
texts = dict(sources)
print("streams", len(sources), "text bytes", sum(len(t) for t in texts.values()))
out = {}
for rep in range(3):
    st = {}
    t0 = time.perf_counter()
    whole, n = gdb.import_cells(v, c, file_root=d, device=0, streams=texts, stats=st)
    dt = time.perf_counter() - t0
    out["whole"] = {"wall_s": dt, "cells": n, "cells_per_s": n / dt, "ms_index": st["ms_index"], "ms_measure": st["ms_measure"], "ms_write": st["ms_write"], "ms_sort_gather": st["ms_sort_gather"]}
    for cap in (64 << 10, 16 << 20):
        heads, recs = {}, {}
        for name, text in sources:
            heads[name], recs[name] = sii.split_text(text)
        t0 = time.perf_counter()
        imp = gdb.StreamImporter(sii.loader_json(v, c))
        names = [n_ for n_, _ in sources]
        for n_ in names:
            imp.add_buffer_stream(n_, False, cap, heads[n_])
        imp.setup()
        pos = {n_: 0 for n_ in names}
        def piece(n_):
            r = recs[n_]; i = pos[n_]; size = 0; j = i
            while j < len(r) and (j == i or size + len(r[j]) <= cap):
                size += len(r[j]); j += 1
            pos[n_] = j
            return b"".join(r[i:j])
        for k, n_ in enumerate(names):
            imp.write(k, piece(n_))
        got = []
        while not imp.done:
            cells, ex = imp.import_batch()
            got.append(cells)
            for k, _ in ex:
                imp.write(k, piece(names[k]))
        s = imp.stats()
        imp.finish(); imp.close()
        dt = time.perf_counter() - t0
        assert b"".join(got) == whole
        out["stream_%d" % cap] = dict(s, wall_s=dt, cells_per_s=s["num_cells"] / dt)
print(json.dumps(out, indent=1))
