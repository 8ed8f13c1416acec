"""vcfdiff_model.py - the rule of the device vcfdiff ("Comparing two VCFs") in plain Python: header tables, line keys, the
walk and the compare, written from the rule's text and the reference's lines it cites (tools/src/vcfdiff.cc, tools/include/vcfdiff.h).
It shares no code with the product; tests compare the product's report with model(...) for equality.

report = {"compared": pairs compared, "events": [event, ...]}; an event is listed when it is not COMPARED or when a bit is set:
  {"kind", "gold_line", "test_line" (1-based, 0: none), "gold_text", "test_text", "flags": [names],
   "info": {mask name: [field names]}, "format": {...}}      (flags / info / format only where a compare ran)
"""
import gzip
import re

import numpy as np

FLAG_NAMES = ("ID", "ALLELES", "QUAL", "FILTER")
MASK_NAMES = ("MISSING_IN_TEST", "ADDED_IN_TEST", "TYPE_DIFFERS", "DIFFERS")
KNOWN = ("END REF ALT QUAL FILTER BaseQRankSum ClippingRankSum MQRankSum ReadPosRankSum DP MQ RAW_MQ MQ0 DP_FORMAT MIN_DP GQ SB AD PL AF AN AC "
         "GT PS PGT PID ExcessHet ID").split()      # known_field_info.cc:42-71
KNOWN_CLASS = {"AF": "A", "AC": "A", "AD": "R", "PL": "G", "GT": "GT"}      # :239-283; every other known name: identity
MAX_FIELDS = 64
MAX_ALLELES = 255
MAX_KEYS = 64


class VcfDiffError(Exception):
    pass


def read_text(path):
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:4] == b"BCF\x02":
        raise VcfDiffError("%s is BCF2: vcfdiff reads VCF text only" % path)
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
        if raw[:4] == b"BCF\x02":
            raise VcfDiffError("%s is BCF2: vcfdiff reads VCF text only" % path)
    return raw.decode("latin-1")


# ---- headers --------------------------------------------------------------------------------------------------------------------
def _attrs(body):
    """ID=..,Number=..,Type=..,Description="..." -> dict (quotes respected)"""
    out, key, val, in_q, on_val = {}, "", "", False, False
    for c in body + ",":
        if c == '"':
            in_q = not in_q
            val += c
        elif c == "," and not in_q:
            if key:
                out[key] = val
            key, val, on_val = "", "", False
        elif c == "=" and not on_val and not in_q:
            on_val = True
        elif on_val:
            val += c
        else:
            key += c
    return out


class Header:
    def __init__(self, text):
        self.contigs, self.info, self.fmt, self.filters, self.samples = [], {}, {}, [], []
        self.info_order, self.fmt_order = [], []
        self.lines_before = 0
        pos = 0
        while pos < len(text):
            eol = text.find("\n", pos)
            if eol < 0:
                eol = len(text)
            line = text[pos:eol].rstrip("\r")
            if line and not line.startswith("#"):
                break
            self.lines_before += 1
            pos = eol + 1
            m = re.match(r"##(contig|INFO|FORMAT|FILTER)=<(.*)>\s*$", line)
            if m:
                a = _attrs(m.group(2))
                if "ID" not in a:
                    continue
                if m.group(1) == "contig":
                    if a["ID"] not in self.contigs:
                        self.contigs.append(a["ID"])
                elif m.group(1) == "FILTER":
                    self.filters.append(a["ID"])
                else:
                    d, order = (self.info, self.info_order) if m.group(1) == "INFO" else (self.fmt, self.fmt_order)
                    if a["ID"] not in d:
                        order.append(a["ID"])
                    d[a["ID"]] = (a.get("Number", "."), a.get("Type", "String"))
            elif line.startswith("#CHROM"):
                self.samples = line.split("\t")[9:]
        self.record_begin = min(pos, len(text))


def field_table(gold_defs, gold_order, test_defs, test_order, what):
    """the union of the names, gold's header order then the names only test has: [(name, type, class, in_gold, in_test, type_differs, number_differs)]"""
    names = list(gold_order) + [n for n in test_order if n not in gold_defs]
    if len(names) > MAX_FIELDS:
        raise VcfDiffError("more than 64 distinct %s names in the two headers (%d): the result masks are 64 bits wide" % (what, len(names)))
    table = []
    for n in names:
        g, t = gold_defs.get(n), test_defs.get(n)
        number, typ = g if g else t
        both = g is not None and t is not None
        if n in KNOWN:
            cls, ndiff = KNOWN_CLASS.get(n, "I"), False
        else:
            cls = number if number in ("A", "R", "G") else "I"
            ndiff = both and g[0] != t[0]
        kind = {"Integer": "INT", "Float": "FLOAT", "Flag": "FLAG"}.get(typ, "STR")
        table.append(dict(name=n, type=kind, cls=cls, in_gold=g is not None, in_test=t is not None, type_differs=both and g[1] != t[1], number_differs=ndiff))
    return table


# ---- values ---------------------------------------------------------------------------------------------------------------------
_INT = re.compile(r"[+-]?[0-9]+\Z")
_FLOAT_PREFIX = re.compile(r"\s*([+-]?(?:(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|inf(?:inity)?|nan))", re.I)


def plain_int(tok):
    if not _INT.match(tok):
        return None
    v = int(tok)
    return v if -2**63 <= v < 2**63 else None


def is_missing(tok):
    return tok == "" or tok == "."


def all_missing(toks):
    return all(is_missing(t) for t in toks)


def to_float32(tok):
    """(float)strtod(tok): the longest numeric prefix, 0 when there is none; '.' is missing (NaN)"""
    if is_missing(tok):
        return np.float32("nan")
    m = _FLOAT_PREFIX.match(tok)
    with np.errstate(all="ignore"):
        return np.float32(float(m.group(1))) if m else np.float32(0.0)


def float_differs(a_tok, b_tok, threshold):
    """compare_unequal<float> (:366-376): a decides the relative difference"""
    if is_missing(a_tok) and is_missing(b_tok):
        return False
    if a_tok == b_tok:
        return False
    a, b = to_float32(a_tok), to_float32(b_tok)
    with np.errstate(all="ignore"):
        diff = np.abs(np.float32(a - b))
        rel = np.abs(np.float32(diff / a)) if a != 0 else np.float32(0.0)
    return bool(float(diff) > threshold and float(rel) > threshold)


def int_differs(a, b):
    if is_missing(a) and is_missing(b):
        return False
    if is_missing(a) or is_missing(b):
        return True
    if a == b:
        return False
    x, y = plain_int(a), plain_int(b)
    return x is None or y is None or x != y


def elem_differs(typ, g, t, threshold):
    if typ == "FLOAT":
        return float_differs(g, t, threshold)      # in fields a is gold
    if typ == "INT":
        return int_differs(g, t)
    return not ((is_missing(g) and is_missing(t)) or g == t)


# ---- genotype index maps (vcfdiff.h:57-100) -------------------------------------------------------------------------------------
def _binom(n, k):
    if k < 0 or k > n:
        return 0
    r = 1
    for i in range(1, k + 1):
        r = r * (n - k + i) // i
    return r


def genotype_of(k, ploidy, n_alleles):
    """the ascending allele list of genotype index k, None when k is beyond the genotypes of n_alleles"""
    if k >= _binom(n_alleles + ploidy - 1, ploidy):
        return None
    out = []
    for m in range(ploidy, 0, -1):
        a = 0
        while _binom(a + 1 + m - 1, m) <= k:
            a += 1
        k -= _binom(a + m - 1, m)
        out.append(a)
    return out[::-1]


def genotype_index(alleles):
    return sum(_binom(a + m, m + 1) for m, a in enumerate(sorted(alleles)))


def map_index(cls, k, amap, ploidy):
    n = len(amap)
    if cls == "A":
        return amap[k + 1] - 1 if k + 1 < n else k
    if cls == "R":
        return amap[k] if k < n else k
    if cls == "G":
        if ploidy < 1 or ploidy > 8:
            return k
        g = genotype_of(k, ploidy, n)
        if g is None:
            return k
        return genotype_index([amap[a] for a in g])
    return k


def split_gt(tok):
    """-> (allele tokens, separators in front of the 2nd and later alleles)"""
    return re.split(r"[/|]", tok), re.findall(r"[/|]", tok)


def gt_differs(g, t):
    ga, gs = split_gt(g)
    ta, ts = split_gt(t)
    n = max(len(ga), len(ta))
    ga += ["."] * (n - len(ga))
    ta += ["."] * (n - len(ta))
    if any(int_differs(x, y) for x, y in zip(ga, ta)):
        return True
    return any(x != y for x, y in zip(gs, ts))


def vector_differs(fd, gtoks, ttoks, amap, alleles_flag, ploidy, threshold):
    cls, typ = fd["cls"], fd["type"]
    if cls == "GT":
        return gt_differs(",".join(gtoks), ",".join(ttoks))
    if cls in ("A", "R", "G"):
        if alleles_flag:
            return True
        if len(gtoks) != len(ttoks):
            return not (all_missing(gtoks) and all_missing(ttoks))
        for k, g in enumerate(gtoks):
            m = map_index(cls, k, amap, ploidy)
            if m < 0 or m >= len(ttoks) or elem_differs(typ, g, ttoks[m], threshold):
                return True
        return False
    n = min(len(gtoks), len(ttoks))
    if any(elem_differs(typ, gtoks[k], ttoks[k], threshold) for k in range(n)):
        return True
    return not all_missing(gtoks[n:]) or not all_missing(ttoks[n:])


# ---- lines ----------------------------------------------------------------------------------------------------------------------
class Record:
    __slots__ = ("line_no", "text", "cols", "contig", "pos", "end", "refblock", "long_ref")


def info_pairs(col):
    """[(key, value)] of an INFO column; a later duplicate of a key replaces the earlier value in place"""
    if col == ".":
        return []
    out, at = [], {}
    for kv in col.split(";"):
        k, _, v = kv.partition("=")
        if k in at:
            out[at[k]] = (k, v)
        else:
            at[k] = len(out)
            out.append((k, v))
    return out


def parse_records(path, text, hdr):
    """every record line of a file with its keys; the first offending line speaks"""
    recs, seen, cur = [], set(), None
    line_no = hdr.lines_before
    for raw in text[hdr.record_begin:].split("\n"):
        line_no += 1
        line = raw.rstrip("\r") if raw.endswith("\r") else raw
        if not line or line.startswith("#"):
            continue
        where = "%s line %d" % (path, line_no)
        cols = line.split("\t")
        if len(cols) < 8:
            raise VcfDiffError("short record line in " + where)
        if cols[0] not in hdr.contigs:
            raise VcfDiffError("contig %s is not in the header of its file (%s)" % (cols[0], where))
        pos = plain_int(cols[1])
        info = info_pairs(cols[7])
        endv = [v for k, v in info if k == "END"]
        end = plain_int(endv[-1]) if endv else 0
        if pos is None or end is None:
            raise VcfDiffError("POS / END not in plain decimal form (%s)" % where)
        for k, _ in info:
            if k != "END" and k not in hdr.info:
                raise VcfDiffError("INFO key %s is not declared in the header (%s)" % (k, where))
        if len(cols) > 8:
            keys = cols[8].split(":")
            if len(keys) > MAX_KEYS:
                raise VcfDiffError("more than 64 FORMAT keys on a line (%s)" % where)
            for k in keys:
                if k not in hdr.fmt:
                    raise VcfDiffError("FORMAT key %s is not declared in the header (%s)" % (k, where))
        if (1 if cols[4] == "." else 1 + len(cols[4].split(","))) > MAX_ALLELES:
            raise VcfDiffError("more than 255 alleles on a line (%s)" % where)
        r = Record()
        r.line_no, r.text, r.cols, r.contig, r.pos = line_no, line, cols, cols[0], pos - 1
        r.end = end - 1 if endv else r.pos + len(cols[3]) - 1
        r.refblock, r.long_ref = cols[4] == "<NON_REF>", len(cols[3]) > 1
        if cur is None or r.contig != cur.contig:
            if r.contig in seen:
                raise VcfDiffError("the records of contig %s are not contiguous (%s)" % (r.contig, where))
            seen.add(r.contig)
        elif r.pos < cur.pos:
            raise VcfDiffError("POS goes back within contig %s (%s)" % (r.contig, where))
        cur = r
        recs.append(r)
    return recs


def parse_regions(regions):
    """chr | chr:pos | chr:from-to | chr:from- , comma separated; the first entry per contig counts (:807-848) -> {contig: (lo, hi)} 0-based, inclusive"""
    out = {}
    for entry in (regions or "").split(","):
        if not entry:
            continue
        name, lo, hi = entry, 0, 2**62
        i = entry.rfind(":")
        m = re.match(r"([0-9]+)(-([0-9]*))?\Z", entry[i + 1:]) if i > 0 else None
        if m:
            name = entry[:i]
            lo = int(m.group(1)) - 1
            hi = lo if m.group(2) is None else (int(m.group(3)) - 1 if m.group(3) else 2**62)
        if name not in out:
            out[name] = (lo, hi)
    return out


# ---- compare --------------------------------------------------------------------------------------------------------------------
def compare(g, t, T):
    """compare_line (:659-758) -> (flags, info masks, format masks) as sets of names"""
    flags = set()
    thr = T["threshold"]
    if set(re.split(r"[;,]", g.cols[2])) != set(re.split(r"[;,]", t.cols[2])):
        flags.add("ID")
    galts = [] if g.cols[4] == "." else g.cols[4].split(",")
    talts = [] if t.cols[4] == "." else t.cols[4].split(",")
    amap = [0]
    if len(galts) != len(talts) or (g.pos == t.pos and g.cols[3] != t.cols[3]) or any(a not in galts for a in talts) or any(a not in talts for a in galts):
        flags.add("ALLELES")
    else:
        amap += [1 + talts.index(a) for a in galts]
    if float_differs(t.cols[5], g.cols[5], thr):      # a is test here (:714)
        flags.add("QUAL")
    gf = [] if g.cols[6] == "." else g.cols[6].split(";")
    tf = [] if t.cols[6] == "." else t.cols[6].split(";")
    if len(gf) != len(tf) or any(f not in gf for f in tf):
        flags.add("FILTER")
    alleles_flag = "ALLELES" in flags
    info = {m: set() for m in MASK_NAMES}
    fmt = {m: set() for m in MASK_NAMES}

    def both(fd, masks, gtoks, ttoks, ploidy):
        if fd["type_differs"]:
            masks["TYPE_DIFFERS"].add(fd["name"])
        elif fd["type"] == "FLAG":
            pass
        elif fd["number_differs"] or vector_differs(fd, gtoks, ttoks, amap, alleles_flag, ploidy, thr):
            masks["DIFFERS"].add(fd["name"])

    def one(fd, masks, which, toks):
        if fd["type"] != "FLAG" and not all_missing(toks):
            masks[which].add(fd["name"])

    gi = [(k, v) for k, v in info_pairs(g.cols[7]) if k != "END"]
    ti = [(k, v) for k, v in info_pairs(t.cols[7]) if k != "END"]
    tid, gid = dict(ti), dict(gi)
    for k, v in gi:
        fd = T["info"][k]
        if k in tid:
            both(fd, info, v.split(","), tid[k].split(","), 0)
        else:
            one(fd, info, "MISSING_IN_TEST", v.split(","))
    for k, v in ti:
        if k not in gid:
            one(T["info"][k], info, "ADDED_IN_TEST", v.split(","))

    if len(g.cols) > 8 and len(t.cols) > 8:
        gk, tk = g.cols[8].split(":"), t.cols[8].split(":")
        for j, tj in enumerate(T["sample_map"]):
            gs = (g.cols[9 + j] if 9 + j < len(g.cols) else "").split(":")
            ts = (t.cols[9 + tj] if 9 + tj < len(t.cols) else "").split(":")
            gv = lambda i: gs[i].split(",") if i < len(gs) else ["."]
            tv = lambda i: ts[i].split(",") if i < len(ts) else ["."]
            ploidy = len(split_gt(gs[0])[0]) if gk[0] == "GT" else 0
            for i, k in enumerate(gk):
                if gk.index(k) != i:
                    continue       # a repeated key: its first subfield counts
                fd = T["fmt"][k]
                if k in tk:
                    both(fd, fmt, gv(i), tv(tk.index(k)), ploidy)
                else:
                    one(fd, fmt, "MISSING_IN_TEST", gv(i))
            for i, k in enumerate(tk):
                if k not in gk and tk.index(k) == i:
                    one(T["fmt"][k], fmt, "ADDED_IN_TEST", tv(i))
    return flags, info, fmt


# ---- the walk -------------------------------------------------------------------------------------------------------------------
def walk(gold, test, gold_contigs, test_contigs):
    """-> [(kind, gold record or None, test record or None)] over records grouped by contig"""
    def by_contig(recs):
        d = {}
        for r in recs:
            d.setdefault(r.contig, []).append(r)
        return d
    G, T = by_contig(gold), by_contig(test)
    common = sorted((c for c in gold_contigs if c in test_contigs), key=lambda s: s.encode("latin-1"))
    events = []
    for c in common:
        gl, tl = G.get(c, []), T.get(c, [])
        i = j = 0
        while i < len(gl) and j < len(tl):
            g, t = gl[i], tl[j]
            overlap = g.pos <= t.end and t.pos <= g.end
            if g.pos == t.pos and g.end == t.end:
                events.append(("COMPARED", g, t))
                i += 1
                j += 1
            elif g.refblock and t.refblock and overlap:
                events.append(("REF_BLOCKS_OVERLAP", g, t))
                if g.end <= t.end:
                    i += 1
                if t.end <= g.end:
                    j += 1
            else:
                events.append(("DIFFERENT_POSITIONS", g, t))
                if not overlap:
                    if g.pos < t.pos:
                        while i < len(gl) and gl[i].end < t.pos:
                            i += 1
                    else:
                        while j < len(tl) and tl[j].end < g.pos:
                            j += 1
                elif t.end > g.end:
                    if t.long_ref and t.pos <= g.pos:
                        j += 1
                    else:
                        i += 1
                elif g.end > t.end:
                    if g.long_ref and g.pos <= t.pos:
                        i += 1
                    else:
                        j += 1
                else:
                    i += 1
                    j += 1
        if i < len(gl):
            events.append(("EXTRA_LINES", gl[i], None))
        elif j < len(tl):
            events.append(("EXTRA_LINES", None, tl[j]))
    for c in gold_contigs:
        if c not in test_contigs and G.get(c):
            events.append(("EXTRA_LINES", G[c][0], None))
    for c in test_contigs:
        if c not in gold_contigs and T.get(c):
            events.append(("EXTRA_LINES", None, T[c][0]))
    return events


def model(gold_path, test_path, threshold=1e-5, regions=""):
    gtext, ttext = read_text(gold_path), read_text(test_path)
    gh, th = Header(gtext), Header(ttext)
    for h in (gh, th):
        if len(set(h.samples)) != len(h.samples):
            raise VcfDiffError("duplicate sample name in a file header")
    if set(gh.samples) != set(th.samples):
        raise VcfDiffError("Sample names in the 2 file headers are different - cannot perform any further comparisons")
    info = field_table(gh.info, gh.info_order, th.info, th.info_order, "INFO")
    fmt = field_table(gh.fmt, gh.fmt_order, th.fmt, th.fmt_order, "FORMAT")
    T = dict(threshold=threshold, info={f["name"]: f for f in info}, fmt={f["name"]: f for f in fmt}, sample_map=[th.samples.index(s) for s in gh.samples])
    gold, test = parse_records(gold_path, gtext, gh), parse_records(test_path, ttext, th)
    if regions:
        R = parse_regions(regions)
        keep = lambda r: r.contig in R and r.pos <= R[r.contig][1] and r.end >= R[r.contig][0]
        gold, test = [r for r in gold if keep(r)], [r for r in test if keep(r)]
    report = {"compared": 0, "events": []}
    for kind, g, t in walk(gold, test, gh.contigs, th.contigs):
        ev = {"kind": kind, "gold_line": g.line_no if g else 0, "test_line": t.line_no if t else 0, "gold_text": g.text if g else "", "test_text": t.text if t else ""}
        if kind in ("COMPARED", "REF_BLOCKS_OVERLAP"):
            report["compared"] += 1
            flags, im, fm = compare(g, t, T)
            ev["flags"] = [n for n in FLAG_NAMES if n in flags]
            ev["info"] = {m: [f["name"] for f in info if f["name"] in im[m]] for m in MASK_NAMES}
            ev["format"] = {m: [f["name"] for f in fmt if f["name"] in fm[m]] for m in MASK_NAMES}
            if kind == "COMPARED" and not flags and not any(im.values()) and not any(fm.values()):
                continue
        report["events"].append(ev)
    return report
