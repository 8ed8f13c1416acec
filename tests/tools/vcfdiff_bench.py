"""vcfdiff_bench.py - first measurement of the device vcfdiff (profiles/device_vcfdiff.md): a combined VCF of 1 000 samples from the
tests' generator (tests/vcfdiff_inputs.py), BGZF, against itself and against a copy whose ALTs are permuted with the fields remapped.
Wall clock of the call, HIP-event time of keys, compare, index and inflate, and the plain-Python model's time beside them.
  python tests/tools/vcfdiff_bench.py [--samples 1000] [--lines 300] [--alleles 4] [--runs 3] [--out FILE.json]"""
import argparse
import copy
import json
import os
import random
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import vcfdiff_inputs as vi  # noqa: E402
import vcfdiff_model as vm   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--lines", type=int, default=300)
    ap.add_argument("--alleles", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    import genomicsdb_amd
    d = tempfile.mkdtemp(prefix="vcfdiff_bench_")
    gold = vi.make_base(1, a.samples, a.alleles, a.lines)
    perm = copy.deepcopy(gold)
    vi.permute_alts(perm, random.Random(2))
    gtext, ptext = gold.text(), perm.text()
    import bgzf_write
    paths = {}
    for name, text in (("gold", gtext), ("permuted", ptext)):
        paths[name] = os.path.join(d, name + ".vcf.gz")
        bgzf_write.write_file(paths[name], text.encode())
    result = {"samples": a.samples, "record_lines": len(gold.recs), "alleles": a.alleles, "text_bytes": len(gtext), "bgzf_bytes": os.path.getsize(paths["gold"]), "cases": {}}
    print("generated %d bytes of text per file" % len(gtext), flush=True)
    for case, test in (("against_itself", "gold"), ("alts_permuted", "permuted")):
        genomicsdb_amd.vcfdiff(paths["gold"], paths[test])      # warm-up: module load, first allocations
        runs = []
        for _ in range(a.runs):
            st = {}
            t0 = time.perf_counter()
            rep = genomicsdb_amd.vcfdiff(paths["gold"], paths[test], stats=st)
            st["wall_s"] = time.perf_counter() - t0
            runs.append(st)
        entry = {"events": len(rep["events"]), "compared": rep["compared"], "runs": runs}
        if not a.no_model:
            t0 = time.perf_counter()
            want = vm.model(paths["gold"], paths[test])
            entry["model_s"] = time.perf_counter() - t0
            entry["equals_model"] = want == rep
        result["cases"][case] = entry
        print(case, json.dumps(entry)[:600], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
