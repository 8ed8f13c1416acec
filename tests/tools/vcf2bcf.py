"""VCF text -> BCF2 (VCFv4.2/BCFv2.2 specification, section 6), typed the way htslib's vcf_parse types a record: the test inputs
of the device importer's BCF2 path.

TEST infrastructure, written next to - not from - the decoder tests/tools/bcf2text.py.  What it follows:
  * one dictionary for FILTER / INFO / FORMAT ids, PASS = 0, else order of first appearance in the header or the IDX= key;
    one contig dictionary (bcf_hdr_parse / bcf_hdr_sync);
  * an integer vector takes the narrowest of int8 / int16 / int32 that holds all its values outside the reserved codes;
    '.' elements are the type's missing value; FORMAT vectors are padded to the longest sample with vector_end;
  * GT is (allele + 1) << 1 | phased, a '.' allele 0 | phased; strings are char vectors (FORMAT: padded with NUL);
  * rlen = END - POS + 1 when INFO has END, else the length of REF.
Ids that the text uses without declaring them (the importers never needed the ## lines) are declared in the written header:
typed by the vid mapping when one is given, else as htslib assumes (String / Number=.).

encode(text, ...) -> (stream, report); report counts the vectors of each type, missing values and vector_end paddings.

    python tests/tools/vcf2bcf.py IN.vcf OUT.bcf [--vid VID.json] [--no-idx | --shuffle-idx SEED] [--no-pass] [--bgzf]
"""
import argparse
import gzip
import json
import random
import re
import struct

INT_MISSING = {1: -128, 2: -32768, 3: -2147483648}
INT_VEND = {1: -127, 2: -32767, 3: -2147483647}
INT_MIN_OK = {1: -120, 2: -32760, 3: -2147483640}     # htslib keeps 8 codes of each width reserved
INT_MAX = {1: 127, 2: 32767, 3: 2147483647}
INT_FMT = {1: "<b", 2: "<h", 3: "<i"}
FLOAT_MISSING, FLOAT_VEND = 0x7F800001, 0x7F800002
BT_INT8, BT_INT16, BT_INT32, BT_FLOAT, BT_CHAR = 1, 2, 3, 5, 7
MISSING, VEND = object(), object()


def new_report():
    return {"int8": 0, "int16": 0, "int32": 0, "float": 0, "char": 0, "flag": 0, "missing": 0, "vector_end": 0, "missing_inside_longer_vector": 0}


def _desc(n, t):
    if n < 15:
        return bytes([(n << 4) | t])
    return bytes([0xF0 | t]) + _typed_int(n)


def _int_type(values):
    vals = [v for v in values if v is not MISSING and v is not VEND]
    for t in (1, 2, 3):
        if all(INT_MIN_OK[t] <= v <= INT_MAX[t] for v in vals):
            return t
    raise ValueError("integer outside int32: %r" % vals)


def _typed_int(v):
    t = _int_type([v])
    return bytes([0x10 | t]) + struct.pack(INT_FMT[t], v)


def _pack_ints(values, t):
    return b"".join(struct.pack(INT_FMT[t], INT_MISSING[t] if v is MISSING else INT_VEND[t] if v is VEND else v) for v in values)


def _pack_floats(values):
    out = []
    for v in values:
        out.append(struct.pack("<I", FLOAT_MISSING) if v is MISSING else struct.pack("<I", FLOAT_VEND) if v is VEND else struct.pack("<f", v))
    return b"".join(out)


def _count(report, values, kind):
    report[kind] += 1
    nm = sum(1 for v in values if v is MISSING)
    report["missing"] += nm
    report["vector_end"] += sum(1 for v in values if v is VEND)
    if nm and len([v for v in values if v is not VEND]) > 1:
        report["missing_inside_longer_vector"] += 1


def _typed_string(s, report=None):
    if report is not None:
        report["char"] += 1
    b = s.encode()
    return _desc(len(b), BT_CHAR) + b


def _typed_int_vector(values, report):
    if not values:
        return b"\x00"
    t = _int_type(values)
    _count(report, values, {1: "int8", 2: "int16", 3: "int32"}[t])
    return _desc(len(values), t) + _pack_ints(values, t)


def _parse_float(s):
    return float(s)       # Python rounds the decimal string to a double as strtod does; struct 'f' rounds that to float32


_TYPE_OF_VID = {"int": "Integer", "integer": "Integer", "float": "Float", "char": "String", "string": "String", "flag": "Flag", "bool": "Flag", "boolean": "Flag"}


def _vid_types(vid):
    """vcf name -> {'INFO': Type, 'FORMAT': Type}, plus contig names, from a vid mapping (dict)"""
    out = {}
    fields = vid.get("fields", {})
    items = fields.items() if isinstance(fields, dict) else [(f["name"], f) for f in fields]
    for name, f in items:
        t = f.get("type")
        if isinstance(t, list):
            t = t[0]
        ty = _TYPE_OF_VID.get(str(t).lower(), "String")
        vname = f.get("vcf_name", name)
        for cls in f.get("vcf_field_class", []):
            out.setdefault(vname, {})[cls] = ty
    return out


def _split_header(text):
    lines = text.decode().split("\n")
    meta, chrom, recs = [], None, []
    for ln in lines:
        if ln.endswith("\r"):
            ln = ln[:-1]
        if not ln:
            continue
        if ln.startswith("##"):
            meta.append(ln)
        elif ln.startswith("#CHROM"):
            chrom = ln
        elif not ln.startswith("#"):
            recs.append(ln)
    if chrom is None:
        raise ValueError("no #CHROM line")
    return meta, chrom, recs


_STRUCT = re.compile(r"##(FILTER|INFO|FORMAT|contig)=<(.*)>$")


def _line_id(body):
    return re.match(r"ID=([^,>]+)", body).group(1)


def encode(text, vid=None, idx="keep", pass_line=True, seed=0, report=None):
    """idx: 'keep' - write IDX= keys, ids in order of appearance; 'none' - no IDX keys; 'shuffle' - IDX= keys with permuted ids"""
    report = new_report() if report is None else report
    meta, chrom, recs = _split_header(text)
    vt = _vid_types(vid) if vid else {}
    declared = {"FILTER": {}, "INFO": {}, "FORMAT": {}, "contig": {}}
    for ln in meta:
        m = _STRUCT.match(ln)
        if m:
            ty = re.search(r"[,<]Type=([A-Za-z]+)", "<" + m.group(2))
            declared[m.group(1)].setdefault(_line_id(m.group(2)), ty.group(1) if ty else None)
    # ids the records use without a declaration
    extra = []
    for ln in recs:
        c = ln.split("\t")
        if c[0] not in declared["contig"]:
            declared["contig"][c[0]] = None
            extra.append("##contig=<ID=%s>" % c[0])
        if c[6] != ".":
            for f in c[6].split(";"):
                if f != "PASS" and f not in declared["FILTER"]:
                    declared["FILTER"][f] = None
                    extra.append('##FILTER=<ID=%s,Description="undeclared">' % f)
        if c[7] != ".":
            for kv in c[7].split(";"):
                k = kv.split("=", 1)[0]
                if k not in declared["INFO"]:
                    ty = vt.get(k, {}).get("INFO") or ("Flag" if "=" not in kv else "String")
                    declared["INFO"][k] = ty
                    extra.append('##INFO=<ID=%s,Number=%s,Type=%s,Description="undeclared">' % (k, "0" if ty == "Flag" else ".", ty))
        if len(c) > 8:
            for k in c[8].split(":"):
                if k not in declared["FORMAT"]:
                    ty = vt.get(k, {}).get("FORMAT") or ("Integer" if k == "GT" else "String")
                    if k == "GT":
                        ty = "String"       # htslib declares GT a String and encodes it specially
                    declared["FORMAT"][k] = ty
                    extra.append('##FORMAT=<ID=%s,Number=%s,Type=%s,Description="undeclared">' % (k, "1" if k == "GT" else ".", ty))
    # the written header: fileformat, PASS, the text's own lines, the added declarations
    lines = [ln for ln in meta if ln.startswith("##fileformat")] or ["##fileformat=VCFv4.2"]
    if pass_line:
        lines.append('##FILTER=<ID=PASS,Description="All filters passed">')
    lines += [ln for ln in meta if not ln.startswith("##fileformat") and not re.match(r"##FILTER=<ID=PASS[,>]", ln)] + extra
    ids, contigs = {"PASS": 0}, {}
    order = []
    for ln in lines:
        m = _STRUCT.match(ln)
        if not m:
            continue
        name = _line_id(m.group(2))
        if m.group(1) == "contig":
            contigs.setdefault(name, len(contigs))
        elif name not in ids:
            ids[name] = len(ids)
            order.append(name)
    if idx == "shuffle":
        rng = random.Random(seed)
        perm = list(range(1, len(ids)))
        rng.shuffle(perm)
        for name, i in zip(order, perm):
            ids[name] = i
        cperm = list(range(len(contigs)))
        rng.shuffle(cperm)
        contigs = {name: cperm[i] for name, i in contigs.items()}
    if idx in ("keep", "shuffle"):
        def with_idx(ln):
            m = _STRUCT.match(ln)
            if not m:
                return ln
            name = _line_id(m.group(2))
            body = re.sub(r",IDX=\d+", "", m.group(2))
            return "##%s=<%s,IDX=%d>" % (m.group(1), body, contigs[name] if m.group(1) == "contig" else ids[name])
        lines = [with_idx(ln) for ln in lines]
    else:
        lines = [re.sub(r",IDX=\d+>$", ">", ln) for ln in lines]
    header = ("\n".join(lines + [chrom]) + "\n").encode() + b"\x00"
    n_sample = max(len(chrom.split("\t")) - 9, 0)
    out = [b"BCF\x02\x02", struct.pack("<I", len(header)), header]
    for ln in recs:
        out.append(_record(ln.split("\t"), ids, contigs, declared, n_sample, report))
    return b"".join(out), report


def _info_value(ty, val, report):
    if ty == "Flag" or val is None:
        report["flag"] += 1
        return b"\x00"
    if ty == "Integer":
        return _typed_int_vector([MISSING if x == "." else int(x) for x in val.split(",")], report)
    if ty == "Float":
        vals = [MISSING if x == "." else _parse_float(x) for x in val.split(",")]
        _count(report, vals, "float")
        return _desc(len(vals), BT_FLOAT) + _pack_floats(vals)
    return _typed_string(val, report)


def _gt_values(s):
    if s == ".":
        return [0]
    vals, phased, tok = [], 0, ""
    for ch in s + "\0":
        if ch in "/|\0":
            vals.append(phased if tok == "." else ((int(tok) + 1) << 1) | phased)
            phased, tok = (1 if ch == "|" else 0), ""
        else:
            tok += ch
    return vals


def _record(c, ids, contigs, declared, n_sample, report):
    pos = int(c[1]) - 1
    alleles = [c[3]] + ([] if c[4] == "." else c[4].split(","))
    info = [] if c[7] == "." else [kv.split("=", 1) for kv in c[7].split(";")]
    end = None
    for kv in info:
        if kv[0] == "END" and len(kv) > 1:
            end = int(kv[1])
    rlen = (end - pos) if end is not None else len(c[3])
    qual = struct.pack("<I", FLOAT_MISSING) if c[5] == "." else struct.pack("<f", _parse_float(c[5]))
    keys = c[8].split(":") if len(c) > 8 and n_sample else []
    shared = [struct.pack("<iii", contigs[c[0]], pos, rlen), qual, struct.pack("<II", (len(alleles) << 16) | len(info), (len(keys) << 24) | n_sample)]
    shared.append(_typed_string("" if c[2] == "." else c[2]))
    shared += [_typed_string(a) for a in alleles]
    shared.append(_typed_int_vector([] if c[6] == "." else [ids[f] for f in c[6].split(";")], new_report()))
    for kv in info:
        shared.append(_typed_int(ids[kv[0]]))
        shared.append(_info_value(declared["INFO"][kv[0]], kv[1] if len(kv) > 1 else None, report))
    indiv = []
    samples = [s.split(":") for s in c[9:9 + n_sample]]
    for k, key in enumerate(keys):
        raw = [s[k] if k < len(s) else "." for s in samples]
        ty = declared["FORMAT"][key]
        indiv.append(_typed_int(ids[key]))
        if key == "GT":
            per = [_gt_values(x) for x in raw]
            kind = "int"
        elif ty == "Integer":
            per = [[MISSING if x == "." else int(x) for x in v.split(",")] for v in raw]
            kind = "int"
        elif ty == "Float":
            per = [[MISSING if x == "." else _parse_float(x) for x in v.split(",")] for v in raw]
            kind = "float"
        else:
            width = max(len(v.encode()) for v in raw)
            report["char"] += 1
            indiv.append(_desc(width, BT_CHAR) + b"".join(v.encode().ljust(width, b"\x00") for v in raw))
            continue
        width = max(len(v) for v in per)
        per = [v + [VEND] * (width - len(v)) for v in per]
        flat = [x for v in per for x in v]
        if kind == "int":
            t = _int_type(flat)
            for v in per:
                _count(report, v, {1: "int8", 2: "int16", 3: "int32"}[t])
            indiv.append(_desc(width, t) + _pack_ints(flat, t))
        else:
            for v in per:
                _count(report, v, "float")
            indiv.append(_desc(width, BT_FLOAT) + _pack_floats(flat))
    sh, ind = b"".join(shared), b"".join(indiv)
    return struct.pack("<II", len(sh), len(ind)) + sh + ind


def read_text(path):
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def encode_file(src, dst, vid=None, bgzf=False, **kw):
    """src (plain or gzip VCF) -> dst; bgzf: a BGZF .bcf through tests/tools/bgzf_write.py, else the plain stream"""
    data, report = encode(read_text(src), vid=vid, **kw)
    if bgzf:
        import bgzf_write
        bgzf_write.write_file(dst, data)
    else:
        with open(dst, "wb") as f:
            f.write(data)
    return data, report


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--vid")
    ap.add_argument("--no-idx", action="store_true")
    ap.add_argument("--shuffle-idx", type=int)
    ap.add_argument("--no-pass", action="store_true")
    ap.add_argument("--bgzf", action="store_true")
    a = ap.parse_args()
    _, rep = encode_file(a.src, a.dst, vid=json.load(open(a.vid)) if a.vid else None, bgzf=a.bgzf,
                         idx="none" if a.no_idx else "shuffle" if a.shuffle_idx is not None else "keep", pass_line=not a.no_pass, seed=a.shuffle_idx or 0)
    print(json.dumps(rep))
