"""Seeded writer of synthetic (g)VCF text for the importers (host/vcf_importer.cc against kernels/gdb_import.hip): single-sample
gVCFs plus, optionally, one multi-sample VCF, with a vid and a callset mapping next to them.

What the text holds on purpose: two contigs written in an order other than their column offsets, reference blocks (END=) of
random length - so that some cross any column cut -, SNPs, insertions, deletions (intervals with treat_deletions_as_intervals)
with a record inside the deleted range (overlap on one row), two records at one position (sort ties), '.' elements, missing
FORMAT values, sum-like INFO fields (divided among the samples of the multi-sample file) and a few numeric tokens outside the
device's fast path (deferred to the host parser).

    python tests/tools/synth_gvcf_text.py OUTDIR --files 6 --lines 2000 --multi 3
"""
import argparse
import json
import os
import random

CONTIGS = [("1", 0, 5000000), ("2", 5000000, 5000000)]      # name, column offset, length
WRITE_ORDER = ["2", "1"]                                      # not the order of the offsets

VID_FIELDS = {
    "PASS": {"type": "int"}, "LowQual": {"type": "int"},
    "END": {"vcf_field_class": ["INFO"], "type": "int"},
    "BaseQRankSum": {"vcf_field_class": ["INFO"], "type": "float"},
    "MQ": {"vcf_field_class": ["INFO"], "type": "float"},
    "RAW_MQ": {"vcf_field_class": ["INFO"], "type": "float", "VCF_field_combine_operation": "sum"},
    "MLEAC": {"vcf_field_class": ["INFO"], "type": "int", "length": "A", "VCF_field_combine_operation": "element_wise_sum"},
    "DP": {"vcf_field_class": ["INFO", "FORMAT"], "type": "int"},
    "GT": {"vcf_field_class": ["FORMAT"], "type": "int", "length": "PP"},
    "AD": {"vcf_field_class": ["FORMAT"], "type": "int", "length": "R"},
    "GQ": {"vcf_field_class": ["FORMAT"], "type": "int"},
    "MIN_DP": {"vcf_field_class": ["FORMAT"], "type": "int"},
    "PL": {"vcf_field_class": ["FORMAT"], "type": "int", "length": "G"},
    "SB": {"vcf_field_class": ["FORMAT"], "type": "int", "length": 4},
    "PID": {"vcf_field_class": ["FORMAT"], "type": "char", "length": "VAR"},
}
BASES = "ACGT"


def _sample_block(rng):
    dp = rng.randrange(0, 60)
    return "0/0:%d:%d:%d:0,%d,%d" % (dp, rng.randrange(0, 99), max(dp - 3, 0), rng.randrange(0, 90), rng.randrange(90, 900))


def _sample_variant(rng, n_alt):
    n_all = n_alt + 1
    gt = "%d%s%d" % (rng.randrange(n_all), rng.choice("/|"), rng.randrange(n_all))
    if rng.random() < 0.03:
        gt = rng.choice([".", "./.", "1"])
    ad = ",".join(str(rng.randrange(0, 50)) if rng.random() > 0.02 else "." for _ in range(n_all))
    pl = ",".join(str(rng.randrange(0, 2000)) for _ in range(n_all * (n_all + 1) // 2))
    sb = ",".join(str(rng.randrange(0, 30)) for _ in range(4)) if rng.random() > 0.05 else "."
    return "%s:%s:%d:%d:%s:%s:%d_x" % (gt, ad, rng.randrange(1, 90), rng.randrange(0, 99), pl, sb, rng.randrange(1, 10 ** 6))


def _float(rng):
    r = rng.random()
    if r < 0.002:
        return "%.17g" % rng.uniform(-50, 50)          # more digits than the fast path takes
    if r < 0.004:
        return rng.choice(["1e-30", "2.5e+30"])
    if r < 0.3:
        return "%.2e" % rng.uniform(-1, 1)
    return "%.3f" % rng.uniform(-60, 60)


def write_vcf(path, sample_names, n_lines, rng):
    ns = len(sample_names)
    out = ["##fileformat=VCFv4.2", "##source=synth_gvcf_text", "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + sample_names)]
    per_contig = [n_lines // 2, n_lines - n_lines // 2]
    for name, n in zip(WRITE_ORDER, per_contig):
        length = [c for c in CONTIGS if c[0] == name][0][2]
        step = max(8, (length - 1000) // max(n, 1))
        pos = 1 + rng.randrange(0, 50)
        written = 0
        while written < n:
            r = rng.random()
            if r < 0.6:      # reference block
                end = pos + rng.randrange(0, 2 * step)
                out.append("\t".join([name, str(pos), ".", rng.choice(BASES), "<NON_REF>", ".", ".", "END=%d" % end, "GT:DP:GQ:MIN_DP:PL"] + [_sample_block(rng) for _ in range(ns)]))
                written += 1
                pos = end + 1 if rng.random() > 0.1 else pos + 1      # sometimes the next record overlaps the block
                continue
            if r < 0.8:
                ref, alts = rng.choice(BASES), [rng.choice(BASES)]
            elif r < 0.9:
                ref = "".join(rng.choice(BASES) for _ in range(rng.randrange(2, 9)))
                alts = [ref[0] if rng.random() < 0.7 else ref[0].lower()]            # deletion
            else:
                ref = rng.choice(BASES)
                alts = [ref + "".join(rng.choice(BASES) for _ in range(rng.randrange(1, 6)))]   # insertion
            if rng.random() < 0.2:
                alts.append(rng.choice(BASES) + "T")
            alts.append("<NON_REF>")
            info = ["BaseQRankSum=%s" % _float(rng), "DP=%d" % rng.randrange(0, 200), "MQ=%s" % _float(rng), "RAW_MQ=%s" % _float(rng),
                    "MLEAC=%s" % ",".join(str(rng.randrange(0, 7)) for _ in alts)]
            if rng.random() < 0.1:
                info.append("DP=%d" % rng.randrange(0, 200))       # a repeated key: the last one counts
            qual = "%.2f" % rng.uniform(0, 3000) if rng.random() > 0.05 else "."
            flt = rng.choice([".", "PASS", "LowQual", "PASS;LowQual"])
            rec = "\t".join([name, str(pos), "." if rng.random() > 0.1 else "rs%d" % rng.randrange(10 ** 6), ref, ",".join(alts), qual, flt, ";".join(info),
                             "GT:AD:DP:GQ:PL:SB:PID"] + [_sample_variant(rng, len(alts)) for _ in range(ns)])
            out.append(rec)
            written += 1
            if rng.random() < 0.05 and written < n:                # a second record at the same position
                out.append(rec.replace("\t" + qual + "\t", "\t.\t", 1))
                written += 1
            pos += 1 if len(ref) > 1 and rng.random() < 0.5 else rng.randrange(1, step)      # inside the deleted range, or onwards
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def write_inputs(outdir, n_files=6, n_lines=2000, multi=3, seed=20240518):
    """-> (vid path, callsets path); rows in file order, the samples of the multi-sample file last"""
    os.makedirs(outdir, exist_ok=True)
    rng = random.Random(seed)
    callsets, row = {}, 0
    for i in range(n_files):
        fn = "s%04d.g.vcf" % i
        write_vcf(os.path.join(outdir, fn), ["S%04d" % i], n_lines, rng)
        callsets["S%04d" % i] = {"row_idx": row, "idx_in_file": 0, "filename": fn}
        row += 1
    if multi:
        names = ["M%d" % k for k in range(multi)]
        write_vcf(os.path.join(outdir, "multi.vcf"), names, n_lines, rng)
        for k, nm in enumerate(names):
            callsets[nm] = {"row_idx": row, "idx_in_file": k, "filename": "multi.vcf"}
            row += 1
    vid = {"fields": VID_FIELDS, "contigs": {c[0]: {"length": c[2], "tiledb_column_offset": c[1]} for c in CONTIGS}}
    vp, cp = os.path.join(outdir, "vid.json"), os.path.join(outdir, "callsets.json")
    with open(vp, "w") as f:
        json.dump(vid, f)
    with open(cp, "w") as f:
        json.dump({"callsets": callsets}, f)
    return vp, cp


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--files", type=int, default=6)
    ap.add_argument("--lines", type=int, default=2000)
    ap.add_argument("--multi", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20240518)
    a = ap.parse_args()
    print(*write_inputs(a.outdir, a.files, a.lines, a.multi, a.seed))
