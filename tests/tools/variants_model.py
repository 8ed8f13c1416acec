"""A plain-Python model of the variants query (gt_mpi_gather without a mode flag), built ON TOP of the `--print-calls` document of the
oracle (oracle_print_cells mode 0, pinned by the reference's "calls" goldens).  It shares no code with the product.

The calls document lists, per query interval, the calls in the reference's order (first the intervals that reach the interval's begin,
then the cells that begin inside).  The model
  1. groups them by (begin, end, REF, set of ALT) in order of first appearance (GA4GHCallInfoToVariantIdx::find_or_insert, variant.cc:26-71);
     without REF or ALT among the attributes every call is a variant of its own,
  2. for variants of more than one call merges the alleles (merge_alt_alleles, variant_operations.cc:134-228: first appearance decides an
     ALT's place, <NON_REF> goes last) and, unless the result is a plain reference block, rewrites GT (remap_GT_field, :233-263) and every
     field whose vid length is R, A or G (remap_data_based_on_alleles / _genotype, variant_field_handler.cc:41-398) in merged order,
  3. returns the structure json.loads gives for the reference's document (every numeric field a list, strings as they are).
"""
import json

NON_REF = "<NON_REF>"
BCF_INT32_MISSING = -2147483648
MAX_ALT_FOR_G = 50


def vid_lengths(vid_path):
    """field name -> 'R' / 'A' / 'G' / 'PP' / ... as the vid mapping file spells it (only string lengths matter here)"""
    d = json.load(open(vid_path))
    fields = d["fields"]
    items = fields.items() if isinstance(fields, dict) else [(f["name"], f) for f in fields]
    out = {}
    for name, f in items:
        ln = f.get("length")
        if isinstance(ln, str):
            out[name] = ln
    return out


def genotypes(ploidy, nalleles):
    """allele tuples (non-decreasing) in VCF order"""
    if ploidy == 1:
        return [(a,) for a in range(nalleles)]
    out = []
    for a in range(nalleles):
        for g in genotypes(ploidy - 1, a + 1):
            out.append(g + (a,))
    return out


def _aslist(v):
    return v if isinstance(v, (list, str)) else [v]


def _remap_call(fields, merged_alt, lengths):
    alt = fields["ALT"]
    non_ref = NON_REF in merged_alt
    merged = [None] + merged_alt                      # index 0 = REF
    own = [None] + alt
    m2i = [0] + [max(i for i in range(1, len(own)) if own[i] == a) if a in alt else None for a in merged_alt]
    i2m = [0] + [merged.index(a, 1) for a in alt]
    nm = len(merged)
    out = dict(fields)
    ploidy = 0
    if "GT" in fields:
        gt = fields["GT"]
        step = 2 if lengths.get("GT") in ("PP", "Phased_Ploidy", "PHASED_PLOIDY") else 1
        ploidy = (len(gt) + 1) // 2 if step == 2 else len(gt)
        new = list(gt)
        for i in range(0, len(gt), step):
            v = gt[i]
            if v in (-1, BCF_INT32_MISSING, 2147483647):
                continue
            new[i] = i2m[v] if 0 <= v < len(i2m) else (nm - 1 if non_ref else -1)
        out["GT"] = new
    for name, val in fields.items():
        ln = lengths.get(name)
        if name in ("GT", "REF", "ALT") or ln not in ("R", "A", "G") or isinstance(val, str):
            continue
        get = lambda idx: val[idx] if idx is not None and idx < len(val) else BCF_INT32_MISSING
        if ln == "R":
            out[name] = [get(m2i[j]) for j in range(nm)]
        elif ln == "A":
            out[name] = [get(None if m2i[j] is None else m2i[j] - 1) for j in range(1, nm)]
        else:
            if nm - 1 > MAX_ALT_FOR_G:
                continue
            if ploidy == 0:
                out[name] = [val[0] if val else 0]
                continue
            in_index = {g: k for k, g in enumerate(genotypes(ploidy, len(own)))}
            res = []
            for g in genotypes(ploidy, nm):
                src = [m2i[a] for a in g]
                res.append(BCF_INT32_MISSING if any(s is None for s in src) else get(in_index[tuple(sorted(src))]))
            out[name] = res
    return out


def variants_from_calls(calls_doc, attributes, lengths):
    """calls_doc: the parsed --print-calls document; attributes: the query's attribute names (the calls themselves show which attributes are
    queried in effect: this project's query configuration always adds REF and ALT); lengths: vid_lengths()"""
    variants = []
    for block in calls_doc["variant_calls"]:
        index = {}
        for call in block["variant_calls"]:
            fields = {k: _aslist(v) for k, v in call["fields"].items()}
            c = {"row": call["row"], "interval": call["interval"], "fields": fields}
            if "genomic_interval" in call:
                c["genomic_interval"] = call["genomic_interval"]
            grouped = "REF" in fields and "ALT" in fields
            key = (call["interval"][0], call["interval"][1], fields["REF"], frozenset(fields["ALT"])) if grouped else ("single", len(index))
            if key not in index:
                index[key] = len(variants)
                variants.append([])
            variants[index[key]].append(c)
    out = []
    for calls in variants:
        v = {"interval": calls[-1]["interval"], "common_fields": {}, "variant_calls": calls}
        if "genomic_interval" in calls[-1]:
            v["genomic_interval"] = calls[-1]["genomic_interval"]
        if len(calls) > 1:
            merged_alt = []
            for c in calls:
                for a in c["fields"]["ALT"]:
                    if a != NON_REF and a not in merged_alt:
                        merged_alt.append(a)
            if any(NON_REF in c["fields"]["ALT"] for c in calls):
                merged_alt.append(NON_REF)
            ref = max((c["fields"]["REF"] for c in calls), key=len)
            v["common_fields"] = {"REF": ref, "ALT": merged_alt}
            if not (len(ref) == 1 and merged_alt == [NON_REF]):
                for c in calls:
                    c["fields"] = _remap_call(c["fields"], merged_alt, lengths)
        out.append(v)
    return {"variants": out}


def round6(x):
    """floats to 6 significant digits (the calls document carries "%g" text), everything else as it is"""
    if isinstance(x, float):
        return float("%.6g" % x)
    if isinstance(x, list):
        return [round6(v) for v in x]
    if isinstance(x, dict):
        return {k: round6(v) for k, v in x.items()}
    return x
