"""vcfdiff_inputs.py - seeded generator of small VCF pairs with a known verdict for the vcfdiff tests: a base file (gold) plus one
transformed copy (test).  NEUTRAL transforms must give no event at all (every pair COMPARED and clean); each of SINGLE must raise exactly
the one bit or event it names.  Genotype orders are enumerated here (itertools), not taken from the model or the product."""
import copy
import gzip
import itertools
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))

CONTIGS = ["1", "10", "2", "X"]      # (byte order differs from this order)
HEADER_INFO = [("END", "1", "Integer"), ("DP", "1", "Integer"), ("AF", "A", "Float"), ("MLEAC", "A", "Integer"), ("MQ", "1", "Float"), ("DB", "0", "Flag"),
               ("BaseQRankSum", "1", "Float"), ("XS", "1", "String"), ("RAW", ".", "Float")]
HEADER_FMT = [("GT", "1", "String"), ("AD", "R", "Integer"), ("DP", "1", "Integer"), ("GQ", "1", "Integer"), ("PL", "G", "Integer"), ("SB", "4", "Integer"),
              ("PGT", "1", "String"), ("XF", "A", "Float")]
BASES = "ACGT"


def genotypes(n_alleles, ploidy):
    """the genotypes of a ploidy in VCF order: ascending by the last allele, then the one before it, ..."""
    return sorted(itertools.combinations_with_replacement(range(n_alleles), ploidy), key=lambda g: g[::-1])


class Rec:
    def __init__(self):
        self.chrom, self.pos, self.id, self.ref, self.alts, self.qual, self.filter = "1", 1, ".", "A", [], ".", "."
        self.info = []          # [(key, [tokens] or None for a Flag)]
        self.keys = []          # FORMAT keys
        self.samples = []       # per sample {key: [tokens]}; GT is one token

    def text(self, sample_order=None):
        info = ";".join(k if v is None else "%s=%s" % (k, ",".join(v)) for k, v in self.info) or "."
        cols = [self.chrom, str(self.pos), self.id, self.ref, ",".join(self.alts) or ".", self.qual, self.filter, info]
        if self.keys:
            cols.append(":".join(self.keys))
            order = sample_order if sample_order is not None else range(len(self.samples))
            for s in order:
                sub = [",".join(self.samples[s].get(k, ["."])) for k in self.keys]
                if self.samples[s].get("_drop"):       # trailing subfields that hold nothing are not written
                    while len(sub) > 1 and set(sub[-1]) <= set(".,"):
                        sub.pop()
                cols.append(":".join(sub))
        return "\t".join(cols)


class File:
    def __init__(self, n_samples):
        self.contigs = list(CONTIGS)
        self.info, self.fmt = list(HEADER_INFO), list(HEADER_FMT)
        self.sample_names = ["S%d" % i for i in range(n_samples)]
        self.sample_order = list(range(n_samples))
        self.recs = []

    def text(self):
        out = ["##fileformat=VCFv4.2", '##FILTER=<ID=LowQual,Description="Low quality">', '##FILTER=<ID=q10,Description="q, 10">']
        out += ['##INFO=<ID=%s,Number=%s,Type=%s,Description="%s, generated">' % (i + (i[0],)) for i in self.info]
        out += ['##FORMAT=<ID=%s,Number=%s,Type=%s,Description="x">' % f for f in self.fmt]
        out += ["##contig=<ID=%s,length=100000>" % c for c in self.contigs]
        out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + [self.sample_names[s] for s in self.sample_order]))
        out += [r.text(self.sample_order) for r in self.recs]
        return "\n".join(out) + "\n"


def make_base(seed, n_samples, n_alleles, n_lines=60, exponent_floats=False):
    """ref blocks and variant lines of n_alleles alleles (REF included; the last ALT is <NON_REF>), ploidy 1, 2 and 3 among the samples"""
    rng = random.Random(seed)
    f = File(n_samples)
    for chrom in ("1", "2", "10"):
        pos = 100
        for _ in range(n_lines // 3):
            r = Rec()
            r.chrom, r.pos = chrom, pos
            r.ref = rng.choice(BASES)
            variant = rng.random() < 0.5
            r.keys = ["GT", "AD", "DP", "GQ", "PL", "SB", "PGT", "XF"] if variant else ["GT", "DP", "GQ", "PL"]
            if variant:
                if rng.random() < 0.3:
                    r.ref += "".join(rng.choice(BASES) for _ in range(rng.randint(1, 4)))
                alts = set()
                while len(alts) < n_alleles - 2:
                    a = "".join(rng.choice(BASES) for _ in range(rng.randint(1, 3)))
                    if a != r.ref:
                        alts.add(a)
                r.alts = sorted(alts) + ["<NON_REF>"]
                r.id = rng.choice([".", "rs%d" % rng.randint(1, 999), "rs%d;rs%d" % (rng.randint(1, 99), rng.randint(100, 199))])
                r.qual = rng.choice([".", "%.2f" % (rng.random() * 1000), "50"])
                r.filter = rng.choice([".", "PASS", "LowQual", "LowQual;q10"])
                na = len(r.alts)
                r.info = [("DP", [str(rng.randint(1, 500))]), ("AF", ["%.4f" % rng.random() for _ in range(na)]), ("MLEAC", [str(rng.randint(0, 9)) for _ in range(na)]),
                          ("MQ", ["%.2f" % (rng.random() * 60)]), ("DB", None), ("BaseQRankSum", [rng.choice(["-1.25", ".", "0.000", "1.5e30" if exponent_floats else "2.5"])]),
                          ("XS", [rng.choice(["abc", "."])]), ("RAW", ["%.3f" % (rng.random() * 10) for _ in range(rng.randint(1, 3))])]
                pos += len(r.ref)
            else:
                r.alts = ["<NON_REF>"]
                length = rng.randint(1, 50)
                r.info = [("END", [str(pos + length - 1)])]
                pos += length
            pos += rng.randint(0, 20)
            n = 1 + len(r.alts)
            for s in range(n_samples):
                ploidy = (1, 2, 2, 3)[(s + rng.randint(0, 3)) % 4] if n_samples > 1 else rng.choice((1, 2, 3))
                d = {"GT": [rng.choice(["/", "|"]).join(rng.choice(["0", "."]) for _ in range(ploidy))], "DP": [str(rng.randint(0, 99))], "GQ": [str(rng.randint(0, 99))],
                     "PL": [str(rng.randint(0, 255)) for _ in genotypes(n, ploidy)]}
                if rng.random() < 0.1:
                    d["GT"], d["PL"] = ["./."], ["."]
                if variant:
                    d["AD"] = [str(rng.randint(0, 40)) for _ in range(n)]
                    d["SB"] = [str(rng.randint(0, 20)) for _ in range(4)]
                    d["PGT"] = [rng.choice(["0|1", "."])]
                    d["XF"] = [rng.choice(["%.3f" % rng.random(), "."]) for _ in range(n - 1)]
                r.samples.append(d)
            f.recs.append(r)
    return f


def _ploidy(d):
    return d["GT"][0].count("/") + d["GT"][0].count("|") + 1


# ---- neutral transforms: no event other than a clean COMPARED -----------------------------------------------------------------
def permute_alts(f, rng):
    for r in f.recs:
        na = len(r.alts)
        if na < 2:
            continue
        perm = list(range(1, na + 1))
        rng.shuffle(perm)
        new_of = [0] + perm                              # old allele index -> new allele index
        alts = [None] * na
        for old in range(1, na + 1):
            alts[new_of[old] - 1] = r.alts[old - 1]
        r.alts = alts

        def remap_r(v):
            out = [None] * len(v)
            for old, x in enumerate(v):
                out[new_of[old]] = x
            return out

        def remap_a(v):
            out = [None] * len(v)
            for old, x in enumerate(v):
                out[new_of[old + 1] - 1] = x
            return out
        r.info = [(k, remap_a(v) if k in ("AF", "MLEAC") else v) for k, v in r.info]
        for d in r.samples:
            if "AD" in d:
                d["AD"] = remap_r(d["AD"])
            if "XF" in d:
                d["XF"] = remap_a(d["XF"])
            if len(d["PL"]) > 1:
                gts = genotypes(na + 1, _ploidy(d))
                where = {g: i for i, g in enumerate(gts)}
                out = [None] * len(gts)
                for i, g in enumerate(gts):
                    out[where[tuple(sorted(new_of[a] for a in g))]] = d["PL"][i]
                d["PL"] = out


def shuffle_orders(f, rng):
    rng.shuffle(f.sample_order)
    rng.shuffle(f.info)
    rng.shuffle(f.fmt)
    for r in f.recs:
        rng.shuffle(r.info)
        rng.shuffle(r.keys)


def float_noise(f, rng):
    for r in f.recs:
        r.info = [(k, ["%.9f" % (float(x) * (1 + 2e-7)) if k in ("AF", "MQ") and x != "." else x for x in v] if v else v) for k, v in r.info]
        r.info = [(k, [x.replace("e", "0e") for x in v] if k == "BaseQRankSum" else v) for k, v in r.info]      # 1.5e30 -> 1.50e30: the same value, not the same bytes
        if r.qual not in (".",):
            r.qual = "%.7f" % (float(r.qual) * (1 - 2e-7))


def drop_trailing(f, rng):
    for r in f.recs:
        for d in r.samples:
            d["_drop"] = True


def dot_gt(f, rng):
    for r in f.recs:
        for d in r.samples:
            if set(d["GT"][0]) <= set("./|") and len(d["GT"][0]) > 1:
                d["GT"] = ["."]


NEUTRAL = {"permute_alts": permute_alts, "shuffle_orders": shuffle_orders, "float_noise": float_noise, "drop_trailing": drop_trailing, "dot_gt": dot_gt}


# ---- transforms that raise exactly one bit or event: -> what the report must hold ------------------------------------------------
def _variant(f, rng, need=lambda r: True):
    c = [i for i, r in enumerate(f.recs) if "AD" in r.keys and need(r)]
    return c[rng.randrange(len(c))]


def _expect(f, i, **kw):
    e = {"kind": "COMPARED", "rec": i, "flags": [], "info": {}, "format": {}}
    e.update(kw)
    return [e]


def change_pl(f, rng):
    i = _variant(f, rng, lambda r: any(len(d["PL"]) > 1 for d in r.samples))
    d = rng.choice([d for d in f.recs[i].samples if len(d["PL"]) > 1])
    k = rng.randrange(len(d["PL"]))
    d["PL"][k] = str(int(d["PL"][k]) + 1)
    return _expect(f, i, format={"DIFFERS": ["PL"]})


def permuted_change_pl(f, rng):
    """one PL element changed behind a permutation of the ALTs: the change must be found through the genotype map"""
    permute_alts(f, rng)
    return change_pl(f, rng)


def rename_alt(f, rng):
    i = _variant(f, rng)
    f.recs[i].alts[0] = f.recs[i].alts[0] + "N"
    r = f.recs[i]
    mapped = [k for k, _, _ in HEADER_INFO if k in ("AF", "MLEAC")]
    fm = [k for k, _, _ in HEADER_FMT if k in ("AD", "PL", "XF") and k in r.keys]
    return _expect(f, i, flags=["ALLELES"], info={"DIFFERS": mapped}, format={"DIFFERS": fm})


def drop_id(f, rng):
    i = _variant(f, rng, lambda r: ";" in r.id)
    f.recs[i].id = f.recs[i].id.split(";")[0]
    return _expect(f, i, flags=["ID"])


def add_filter(f, rng):
    i = _variant(f, rng, lambda r: r.filter == "LowQual")
    f.recs[i].filter = "LowQual;q10"
    return _expect(f, i, flags=["FILTER"])


def remove_info(f, rng):
    i = _variant(f, rng)
    f.recs[i].info = [(k, v) for k, v in f.recs[i].info if k != "DP"]
    return _expect(f, i, info={"MISSING_IN_TEST": ["DP"]})


def remove_flag(f, rng):
    i = _variant(f, rng)
    f.recs[i].info = [(k, v) for k, v in f.recs[i].info if k != "DB"]
    return []


def float_beyond(f, rng):
    i = _variant(f, rng)
    f.recs[i].info = [(k, ["%.2f" % (float(v[0]) + 1.5)] if k == "MQ" else v) for k, v in f.recs[i].info]
    return _expect(f, i, info={"DIFFERS": ["MQ"]})


def float_vs_dot(f, rng):
    i = _variant(f, rng)
    f.recs[i].info = [(k, ["."] if k == "MQ" else v) for k, v in f.recs[i].info]
    return []


def cut_ref_block(f, rng):
    c = [i for i, r in enumerate(f.recs) if r.alts == ["<NON_REF>"] and int(r.info[0][1][0]) - r.pos >= 3]
    i = c[rng.randrange(len(c))]
    r = f.recs[i]
    end = int(r.info[0][1][0])
    mid = r.pos + (end - r.pos) // 2
    second = copy.deepcopy(r)
    r.info = [("END", [str(mid)])]
    second.pos = mid + 1
    f.recs.insert(i + 1, second)
    return [{"kind": "REF_BLOCKS_OVERLAP", "rec": i, "test_rec": i}, {"kind": "REF_BLOCKS_OVERLAP", "rec": i, "test_rec": i + 1}]


def delete_line(f, rng):
    i = rng.randrange(1, len(f.recs) // 3 - 1)      # inside the first contig, not its last record
    del f.recs[i]
    return [{"kind": "DIFFERENT_POSITIONS", "rec": i, "test_rec": i}]


def extra_contig(f, rng):
    r = Rec()
    r.chrom, r.pos, r.ref, r.alts = "X", 5, "A", ["<NON_REF>"]
    r.info = [("END", ["9"])]
    r.keys = ["GT", "DP", "GQ", "PL"]
    r.samples = [{"GT": ["0/0"], "DP": ["1"], "GQ": ["2"], "PL": ["0", "1", "2"]} for _ in f.sample_names]
    f.contigs.append("Y")
    r2 = copy.deepcopy(r)
    r2.chrom = "Y"
    f.recs += [r, r2]
    return [{"kind": "EXTRA_LINES", "test_rec": len(f.recs) - 2}, {"kind": "EXTRA_LINES", "test_rec": len(f.recs) - 1}]


SINGLE = {"change_pl": change_pl, "permuted_change_pl": permuted_change_pl, "rename_alt": rename_alt, "drop_id": drop_id, "add_filter": add_filter, "remove_info": remove_info, "remove_flag": remove_flag,
          "float_beyond": float_beyond, "float_vs_dot": float_vs_dot, "cut_ref_block": cut_ref_block, "delete_line": delete_line, "extra_contig": extra_contig}


def make_pair(seed, n_samples, n_alleles, transform, n_lines=60, exponent_floats=False):
    """-> (gold text, test text, expected): expected is [] for a neutral transform, else the events the report must list, each with the
    kind, the gold / test line numbers and, for a compared pair, the flag names and the non-empty masks"""
    gold = make_base(seed, n_samples, n_alleles, n_lines, exponent_floats)
    test = copy.deepcopy(gold)
    rng = random.Random(seed * 7919 + 13)
    if transform == "all_neutral":
        for t in NEUTRAL.values():
            t(test, rng)
        expected = []
    elif transform in NEUTRAL:
        NEUTRAL[transform](test, rng)
        expected = []
    elif transform == "deletion_vs_star":
        # both files have a 3-base deletion; only test has the '*' line that it spans: the walk steps over that line as a misplaced one
        d = Rec()
        d.chrom, d.pos, d.ref, d.alts = "X", 50, "ACG", ["A", "<NON_REF>"]
        d.keys = ["GT", "DP"]
        d.samples = [{"GT": ["0/0"], "DP": ["3"]} for _ in gold.sample_names]
        star = copy.deepcopy(d)
        star.pos, star.ref, star.alts = 51, "C", ["*", "<NON_REF>"]
        after = copy.deepcopy(star)
        after.pos, after.ref, after.alts = 60, "T", ["G", "<NON_REF>"]
        gold.recs += [d, after]
        test.recs += [copy.deepcopy(d), star, copy.deepcopy(after)]
        n = len(gold.recs)
        expected = [{"kind": "DIFFERENT_POSITIONS", "rec": n - 1, "test_rec": n - 1}]
    else:
        expected = SINGLE[transform](test, rng)
    hdr = gold.text().count("\n") - len(gold.recs)
    out = []
    for e in expected:
        e = dict(e)
        g, t = e.pop("rec", None), e.pop("test_rec", None)
        if e["kind"] == "COMPARED":
            t = g
        e["gold_line"] = hdr + g + 1 if g is not None else 0
        e["test_line"] = hdr + t + 1 if t is not None else 0
        out.append(e)
    thdr = test.text().count("\n") - len(test.recs)
    for e in out:
        if e["test_line"]:
            e["test_line"] += thdr - hdr
    return gold.text(), test.text(), out


def write_as(path, text, how):
    """how: "plain" | "gzip" | "bgzf" (small blocks, so that lines cross members)"""
    data = text.encode()
    if how == "plain":
        raw = data
    elif how == "gzip":
        raw = gzip.compress(data)
    else:
        import bgzf_write
        raw = bgzf_write.bgzf(data, 700)
    with open(path, "wb") as f:
        f.write(raw)
    return path


def summarize(report):
    """a report in the generator's terms: kind, line numbers, flags and the non-empty masks"""
    out = []
    for e in report["events"]:
        s = {"kind": e["kind"], "gold_line": e["gold_line"], "test_line": e["test_line"]}
        if e["kind"] == "COMPARED":
            s["flags"] = e["flags"]
            s["info"] = {k: v for k, v in e["info"].items() if v}
            s["format"] = {k: v for k, v in e["format"].items() if v}
        out.append(s)
    return out


def swap_first_two_alts(text):
    """a VCF text with the first two ALTs of every record line that has at least two swapped, and AD, PL and the Number=A INFO fields
    MLEAC / MLEAF / AF / AC remapped; GT indices 1 and 2 are exchanged (they are left alone where the GT is missing)"""
    out = []
    for line in text.split("\n"):
        cols = line.split("\t")
        if line.startswith("#") or len(cols) < 8 or cols[4].count(",") < 1:
            out.append(line)
            continue
        alts = cols[4].split(",")
        n = len(alts) + 1
        new_of = [0, 2, 1] + list(range(3, n))
        alts[0], alts[1] = alts[1], alts[0]
        cols[4] = ",".join(alts)

        def remap(v, shift):
            res = list(v)
            for old, x in enumerate(v):
                res[new_of[old + shift] - shift] = x
            return res
        info = []
        for kv in cols[7].split(";"):
            k, eq, v = kv.partition("=")
            if k in ("MLEAC", "MLEAF", "AF", "AC") and v.count(",") == n - 2:
                v = ",".join(remap(v.split(","), 1))
            info.append(k + eq + v)
        cols[7] = ";".join(info)
        if len(cols) > 9:
            keys = cols[8].split(":")
            for c in range(9, len(cols)):
                sub = cols[c].split(":")
                ploidy = (sub[0].count("/") + sub[0].count("|") + 1) if keys[0] == "GT" else 2
                for i, k in enumerate(keys):
                    if i >= len(sub):
                        break
                    v = sub[i].split(",")
                    if k == "AD" and len(v) == n:
                        sub[i] = ",".join(remap(v, 0))
                    elif k == "PL" and len(v) == len(genotypes(n, ploidy)):
                        gts = genotypes(n, ploidy)
                        where = {g: j for j, g in enumerate(gts)}
                        res = list(v)
                        for j, g in enumerate(gts):
                            res[where[tuple(sorted(new_of[a] for a in g))]] = v[j]
                        sub[i] = ",".join(res)
                    elif k == "GT":
                        sub[i] = "".join({"1": "2", "2": "1"}.get(ch, ch) for ch in sub[i]) if all(len(t) <= 1 for t in sub[i].replace("|", "/").split("/")) else sub[i]
                cols[c] = ":".join(sub)
        out.append("\t".join(cols))
    return "\n".join(out)


# the shapes of the tests: (samples, alleles with REF, record lines).  Samples 1, 3, 64, 65 and 257: one lane, a partial wavefront, a full one, one
# more than a wavefront, one more than a workgroup; alleles 2 and 3 stay on the light path, 4 and 7 take the cooperative one (G = 10 and 28 diploid, 84 triploid)
SHAPES = [(1, 2, 60), (3, 3, 60), (3, 7, 60), (1, 4, 60), (64, 4, 30), (65, 7, 24), (257, 4, 18), (257, 2, 18)]
PERMUTING = ("all_neutral", "permute_alts", "permuted_change_pl")
ALL_TRANSFORMS = ["all_neutral"] + list(NEUTRAL) + list(SINGLE) + ["deletion_vs_star"]


def pair_cases():
    """(samples, alleles, lines, transform): every transform on a light and on a cooperative shape, the permuting ones on every shape"""
    cases = []
    for shape in SHAPES:
        for t in ALL_TRANSFORMS if shape in ((3, 3, 60), (3, 7, 60)) else PERMUTING:
            cases.append(shape + (t,))
    return cases


def seed_of(ns, na, transform):
    return 1000 * ns + 10 * na + ALL_TRANSFORMS.index(transform)
