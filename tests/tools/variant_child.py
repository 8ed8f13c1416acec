"""One fresh process for the knobs that gdb_pipeline.hip / gdb_bgzf.hip read once per process (GDBAMD_RES_LAYOUT, GDBAMD_SLOT_REGROUP,
GDBAMD_SITE_ORDER, GDBAMD_BGZF_BLOCK, GDBAMD_BGZF_WAVES, GDBAMD_BGZF_TEXT).  The parent (tests/test_gpu_kernel_variants.py) sets
the knobs in this process's environment, names the work and an output directory, and does all the judging; this script only runs the
device code and writes what it produced:

  variant_child.py pipeline OUTDIR SHAPE   the named shape of variant_shapes.py through CombineEngine.run_interval, once per entry of
                                           runs.json in OUTDIR ([{"arena_bytes": .., "env": {..}}]; env: per-interval knobs);
                                           -> run<i>.bin (the bytes) and results.json (record count, pages, page_kernel, ...)
  variant_child.py bgzf OUTDIR GOLDEN      the hostile inputs of tests/test_bgzf.py through gdb.bgzf_compress with vcf_text False and True
                                           -> hbytes<i>.bgzf / htext<i>.bgzf (HOSTILE_INPUTS, i: position in the dictionary) and
                                           tbytes<i>.bgzf / ttext<i>.bgzf (HOSTILE_TEXT_INPUTS), and the golden case GOLDEN as a "z"
                                           stream -> golden.z
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (TESTS, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def run_pipeline(outdir, shape_name):
    import genomicsdb_amd as gdb
    import variant_shapes as vs
    N, begin, end, cells, q = vs.inputs(shape_name, outdir)
    with open(os.path.join(outdir, "runs.json")) as f:
        runs = json.load(f)
    eng = gdb.CombineEngine(q)
    eng.stage_cells(cells)
    eng.set_reference(begin, vs.reference_bases(begin, end))
    results = []
    for i, run in enumerate(runs):
        for k, v in run.get("env", {}).items():
            os.environ[k] = v
        got, st = eng.run_interval(begin, end, arena_bytes=run["arena_bytes"])
        for k in run.get("env", {}):
            del os.environ[k]
        with open(os.path.join(outdir, "run%d.bin" % i), "wb") as f:
            f.write(got)
        results.append({"num_records": st.num_records, "pages": st.pages, "page_kernel": st.page_kernel,
                        "resolved_entry_bytes": st.resolved_entry_bytes, "bytes_out": st.bytes_out})
    eng.close()
    with open(os.path.join(outdir, "results.json"), "w") as f:
        json.dump(results, f)


def run_bgzf(outdir, golden_name):
    import genomicsdb_amd as gdb
    import helpers
    import test_bgzf
    from golden_cases import CASES
    for i, data in enumerate(test_bgzf.HOSTILE_INPUTS.values()):
        for mode, vcf_text in (("bytes", False), ("text", True)):
            comp, _ = gdb.bgzf_compress(data, vcf_text=vcf_text)
            with open(os.path.join(outdir, "h%s%d.bgzf" % (mode, i)), "wb") as f:
                f.write(comp)
    for i, data in enumerate(test_bgzf.HOSTILE_TEXT_INPUTS.values()):
        for mode, vcf_text in (("bytes", False), ("text", True)):
            comp, _ = gdb.bgzf_compress(data, vcf_text=vcf_text)
            with open(os.path.join(outdir, "t%s%d.bgzf" % (mode, i)), "wb") as f:
                f.write(comp)
    _, callsets, vid, ov, _, mode = [c for c in CASES if c[0] == golden_name][0]
    q, _ = helpers.query_json(callsets, vid, ov, mode)
    s = gdb.GenomicsDBQueryStream(query_json=q, cells=helpers.cells_for(callsets, vid), buffer_capacity=1 << 20, output_format="z")
    z = s.read()
    s.close()
    with open(os.path.join(outdir, "golden.z"), "wb") as f:
        f.write(z)


if __name__ == "__main__":
    kind, outdir, what = sys.argv[1:4]
    {"pipeline": run_pipeline, "bgzf": run_bgzf}[kind](outdir, what)
    with open(os.path.join(outdir, "done"), "w") as f:
        f.write("ok\n")
