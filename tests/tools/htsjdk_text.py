"""BCF2 ("bu") -> VCF text the way htsjdk prints it: what a GATK caller sees of the stream GenomicsDBFeatureReader opens (is_bcf,
use_missing_values_only_not_vector_end, no IDX keys), so that the stream can be compared byte for byte with the reference's *java_vcf*
goldens (tests/golden/outputs/java_* and *_java_*), which are htsjdk's VCFWriter over BCF2Codec's decoding of that stream.

TEST infrastructure.  It shares the low-level readers of tests/tools/bcf2text.py (parse_stream, the typed descriptor, the value
reader, Header); the printing rules are htsjdk's, as far as the goldens pin them:
  header   ##fileformat=VCFv4.2 first, whatever the stream says; every other ## line once, sorted by its text, the ##contig lines in
           dictionary order as one block where "##contig" sorts; no ',IDX=' keys; then #CHROM
  FILTER   '.' when the record has none
  INFO     keys sorted by code point, a flag is its bare key, floats (QUAL too) through formatVCFDouble, strings verbatim
  FORMAT   GT first, the other keys sorted
  sample   a vector ends at its first vector_end; trailing missing elements are padding and are dropped, a missing element before a
           present one is '.'; nothing left is '.'; a string is the bytes before the first NUL, '.' when empty or the lone 0x07;
           trailing '.' fields of a sample are trimmed (never the first), so an absent sample is a single '.'
  GT       alleles = the elements that are neither missing nor vector_end; '.' when (v >> 1) == 0, else (v >> 1) - 1; ALL joined
           with '|' when the FIRST allele's phase bit is set, else with '/' (the goldens pin: the reference's .|./. and ./.|. both
           print ././., 0|1/0 prints 0/1/0)

decode_record() gives the raw values (integers, float bit patterns) for tests that compare two streams element by element.
"""
import bisect
import decimal
import re
import struct

from bcf2text import (BT_CHAR, BT_FLOAT, BT_INT8, BT_INT16, BT_INT32, BT_NULL, FLOAT_MISSING, _FMT, BCFError, Header,  # noqa: F401
                      _missing_vend, _typed_descriptor, _typed_int, _values, parse_stream)


# ---- numbers ------------------------------------------------------------------------------------------------------------------------
def _fixed(d, places):
    return str(decimal.Decimal(d).quantize(decimal.Decimal(1).scaleb(-places), rounding=decimal.ROUND_HALF_UP))


def _scientific(d, places):
    x = decimal.Decimal(d)
    e = x.adjusted()
    m = x.scaleb(-e).quantize(decimal.Decimal(1).scaleb(-places), rounding=decimal.ROUND_HALF_UP)
    if abs(m) >= 10:      # 9.9996 -> 10.000: one digit before the point again
        e += 1
        m = x.scaleb(-e).quantize(decimal.Decimal(1).scaleb(-places), rounding=decimal.ROUND_HALF_UP)
    return "%se%s%02d" % (m, "-" if e < 0 else "+", abs(e))


def format_vcf_double(d):
    """htsjdk VCFEncoder.formatVCFDouble: d < 0.01 -> %.3e (0.00 when |d| < 1e-20), 0.01 <= d < 1 -> %.3f, d >= 1 -> %.2f; every
    negative number is therefore printed with %.3e.
    java.util.Formatter documents "rounded using the round half up algorithm"; here that is done on the exact value of the double
    (decimal, ROUND_HALF_UP), not with Python's %, which rounds half to even.  No golden holds an exact tie: the tie rule rests on
    that documentation alone (tests/test_htsjdk_text.py has one tie, 2.125, that is exact in binary)."""
    d = float(d)
    if d < 1:
        if d < 0.01:
            return _scientific(d, 3) if abs(d) >= 1e-20 else "0.00"
        return _fixed(d, 3)
    return _fixed(d, 2)


def _float_of(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]      # (Python widens the float to a double, as Java does)


# ---- header -------------------------------------------------------------------------------------------------------------------------
def header_lines(text):
    """the header lines htsjdk writes for a header text (str, with or without IDX keys)"""
    meta, contigs, chrom = set(), [], None
    for ln in text.split("\n"):
        ln = re.sub(r",IDX=\d+>$", ">", ln)
        if ln.startswith("##contig"):
            if ln not in contigs:
                contigs.append(ln)
        elif ln.startswith("##"):
            if not ln.startswith("##fileformat="):
                meta.add(ln)
        elif ln.startswith("#CHROM"):
            chrom = ln
    if chrom is None:
        raise BCFError("no #CHROM line")
    meta = sorted(meta)
    at = bisect.bisect_left(meta, "##contig")
    return ["##fileformat=VCFv4.2"] + meta[:at] + contigs + meta[at:] + [chrom]


# ---- records ------------------------------------------------------------------------------------------------------------------------
class Record:
    """one decoded record: raw values, nothing interpreted.  shared = the bytes of the shared block; info = [(name, type, values)];
    fmt = [(name, type, per-sample length, [values of sample 0, ...])]"""
    __slots__ = ("shared", "rid", "pos", "rlen", "qual_bits", "id", "alleles", "filters", "info", "n_sample", "fmt")


def decode_record(hdr, rec):
    l_shared, l_indiv = struct.unpack_from("<II", rec, 0)
    if len(rec) != 8 + l_shared + l_indiv:
        raise BCFError("record of %d bytes, lengths say %d" % (len(rec), 8 + l_shared + l_indiv))
    r = Record()
    r.shared = bytes(rec[8:8 + l_shared])
    at = 8
    r.rid, r.pos, r.rlen, r.qual_bits, n_allele_info, n_fmt_sample = struct.unpack_from("<iiiIII", rec, at)
    at += 24
    n_info, n_allele = n_allele_info & 0xFFFF, n_allele_info >> 16
    r.n_sample, n_fmt = n_fmt_sample & 0xFFFFFF, n_fmt_sample >> 24
    n, t, at = _typed_descriptor(rec, at)
    vals, at = _values(rec, at, t, n)
    r.id = bytes(vals).decode()
    r.alleles = []
    for _ in range(n_allele):
        n, t, at = _typed_descriptor(rec, at)
        vals, at = _values(rec, at, t, n)
        r.alleles.append(bytes(vals).decode())
    n, t, at = _typed_descriptor(rec, at)
    r.filters, at = _values(rec, at, t, n)
    r.info = []
    for _ in range(n_info):
        key, at = _typed_int(rec, at)
        n, t, at = _typed_descriptor(rec, at)
        vals, at = _values(rec, at, t, n)
        r.info.append((hdr.ids[key], t, vals))
    if at != 8 + l_shared:
        raise BCFError("shared block length: parsed %d, l_shared %d" % (at - 8, l_shared))
    r.fmt = []
    for _ in range(n_fmt):
        key, at = _typed_int(rec, at)
        n, t, at = _typed_descriptor(rec, at)
        w = _FMT[t][1] if t != BT_NULL else 0
        if w and n:       # (one unpack for the field: the synthetic shapes have millions of elements)
            flat = struct.unpack_from("<%d%s" % (r.n_sample * n, _FMT[t][0].lstrip("<")), rec, at)
            per = [list(flat[s * n:(s + 1) * n]) for s in range(r.n_sample)]
        else:
            per = [[] for _ in range(r.n_sample)]
        at += r.n_sample * n * w
        r.fmt.append((hdr.ids[key], t, n, per))
    if at != len(rec):
        raise BCFError("individual block length: parsed %d, record %d" % (at, len(rec)))
    return r


def split_records(body):
    """the records of a stream's body (no header): [bytes, ...]"""
    at, recs = 0, []
    while at < len(body):
        l_shared, l_indiv = struct.unpack_from("<II", body, at)
        recs.append(body[at:at + 8 + l_shared + l_indiv])
        if len(recs[-1]) != 8 + l_shared + l_indiv:
            raise BCFError("truncated record at %d" % at)
        at += 8 + l_shared + l_indiv
    return recs


def expected_flagged(r):
    """the FORMAT fields of record r of the DEFAULT stream as use_missing_values_only_not_vector_end writes them (reference
    variant_field_handler.cc:846-866; the flag reaches nothing but collect_and_extend_fields, so the shared block stays):
      int, float  every vector_end becomes the type's missing value
      GT          a vector that begins with vector_end (no call at all) becomes [0 = no-call allele, missing, ...]; every other
                  vector_end becomes missing
      char        [0x07, NUL, ...] (an absent string) becomes all NUL; anything else stays
    same keys, order, type and per-sample length: [(name, type, n, per-sample values)]"""
    out = []
    for name, t, n, per in r.fmt:
        if t == BT_CHAR:
            new = [[0] * n if v and v[0] == 7 and not any(v[1:]) else list(v) for v in per]
        elif t == BT_NULL:
            new = [list(v) for v in per]
        else:
            missing, vend = _missing_vend(t)
            new = []
            for v in per:
                if name == "GT" and v and v[0] == vend:
                    new.append([0] + [missing] * (n - 1))
                else:
                    new.append([missing if x == vend else x for x in v])
        out.append((name, t, n, new))
    return out


def flag_rule_mismatch(d, f):
    """d: a record of the default stream, f: the same record of the flagged stream (both decoded).  None when f is exactly what the
    flag makes of d - shared block byte for byte, FORMAT fields by expected_flagged() as raw integers / float bit patterns - else a
    description of the first difference"""
    if f.shared != d.shared:
        return "shared block differs at POS %d" % (d.pos + 1)
    if f.n_sample != d.n_sample:
        return "n_sample %d, default stream %d, at POS %d" % (f.n_sample, d.n_sample, d.pos + 1)
    want = expected_flagged(d)
    if [x[:3] for x in f.fmt] != [x[:3] for x in want]:
        return "FORMAT keys / types / lengths %r, expected %r, at POS %d" % ([x[:3] for x in f.fmt], [x[:3] for x in want], d.pos + 1)
    for (name, t, n, got), (_, _, _, exp) in zip(f.fmt, want):
        if got != exp:
            s = [i for i in range(len(exp)) if got[i] != exp[i]][0]
            return "POS %d field %s (type %d) sample %d: %r, expected %r" % (d.pos + 1, name, t, s, got[s], exp[s])
    return None


def _number(t, v, float_bits=None):
    if t != BT_FLOAT:
        return str(v)
    return format_vcf_double(_float_of(float_bits(v) if float_bits else v))


def string_text(vals):
    b = bytes(vals).split(b"\x00", 1)[0]
    return "." if b in (b"", b"\x07") else b.decode()


def vector_text(t, vals, float_bits=None):
    """an INFO value or one sample's FORMAT value that is not GT"""
    if t == BT_CHAR:
        return string_text(vals)
    if t == BT_NULL or not vals:
        return "."
    missing, vend = _missing_vend(t)
    if vend in vals:
        vals = vals[:vals.index(vend)]
    while vals and vals[-1] == missing:
        vals = vals[:-1]
    return ",".join("." if v == missing else _number(t, v, float_bits) for v in vals) if vals else "."


def gt_text(t, vals):
    missing, vend = _missing_vend(t)
    alleles = [v for v in vals if v != missing and v != vend]
    if not alleles:
        return "."
    sep = "|" if alleles[0] & 1 else "/"
    return sep.join("." if (v >> 1) == 0 else str((v >> 1) - 1) for v in alleles)


def record_line(hdr, rec, float_bits=None):
    """float_bits: a function on float bit patterns applied to every float before it is printed (for a comparison with a stream
    that was made from text, which holds fewer digits than a float)"""
    r = rec if isinstance(rec, Record) else decode_record(hdr, rec)
    cols = [hdr.contigs[r.rid], str(r.pos + 1), r.id or ".", r.alleles[0], ",".join(r.alleles[1:]) if len(r.alleles) > 1 else ".",
            "." if r.qual_bits == FLOAT_MISSING else _number(BT_FLOAT, r.qual_bits, float_bits),
            ";".join(sorted(hdr.ids[i] for i in r.filters)) if r.filters else "."]
    info = []
    for name, t, vals in sorted(r.info, key=lambda x: x[0]):
        info.append(name if t == BT_NULL or not vals else name + "=" + vector_text(t, vals, float_bits))
    cols.append(";".join(info) if info else ".")
    if r.fmt:
        if r.n_sample != len(hdr.samples):
            raise BCFError("n_sample %d, header has %d samples" % (r.n_sample, len(hdr.samples)))
        fields = sorted(r.fmt, key=lambda f: (f[0] != "GT", f[0]))
        cols.append(":".join(f[0] for f in fields))
        for s in range(r.n_sample):
            parts = [gt_text(t, per[s]) if name == "GT" else vector_text(t, per[s], float_bits) for name, t, _, per in fields]
            while len(parts) > 1 and parts[-1] == ".":
                parts.pop()
            cols.append(":".join(parts))
    return "\t".join(cols)


def record_lines(data):
    """the record lines of a "bu" stream"""
    hdr, recs = parse_stream(data)
    return [record_line(hdr, r) for r in recs]


def stream_to_text(data):
    """a "bu" stream -> the VCF file htsjdk writes from it (bytes)"""
    hdr, recs = parse_stream(data)
    return ("\n".join(header_lines(hdr.text) + [record_line(hdr, r) for r in recs]) + "\n").encode()
