"""Shared by the BCF2 import tests (CPU harness and device): a callset mapping of VCF text files -> the same mapping over BCF2
encodings of them (tests/tools/vcf2bcf.py), and a BCF2 stream -> the mapping over its text as the independent decoder
tests/tools/bcf2text.py prints it.  Not a test module."""
import json
import os
import struct

import bcf2text
import vcf2bcf


def fmt9(v):
    """9 significant digits identify a float32 and survive (float)strtod"""
    return "%.9g" % v


def _entries(cs):
    c = cs["callsets"]
    return list(c.values()) if isinstance(c, dict) else c


def rewrite_callsets(src_callsets, dst_callsets, rename):
    """the mapping with every "filename" f replaced by rename(f); -> the file names in mapping order, old -> new"""
    cs = json.load(open(src_callsets))
    names = {}
    for e in _entries(cs):
        if e["filename"] not in names:
            names[e["filename"]] = rename(e["filename"], len(names))
        e["filename"] = names[e["filename"]]
    with open(dst_callsets, "w") as f:
        json.dump(cs, f)
    return names


def encode_mapping(vid_path, callsets_path, root, outdir, bgzf=False, **kw):
    """-> (new callsets path, {new file name: plain BCF2 stream}, summed encoder report); the files are written to outdir, as plain
    BCF2 or as BGZF .bcf"""
    os.makedirs(outdir, exist_ok=True)
    vid = json.load(open(vid_path))
    new_cs = os.path.join(outdir, "callsets.json")
    names = rewrite_callsets(callsets_path, new_cs, lambda f, k: "f%d.bcf" % k)
    streams, report = {}, vcf2bcf.new_report()
    for old, new in names.items():
        src = old if os.path.isabs(old) else os.path.join(root, old)
        data, _ = vcf2bcf.encode_file(src, os.path.join(outdir, new), vid=vid, bgzf=bgzf, report=report, **kw)
        streams[new] = data
    return new_cs, streams, report


def decode_mapping(callsets_path, streams, outdir):
    """the mapping `callsets_path` (file names = keys of streams) over the streams' text by bcf2text, %.9g floats -> new callsets path"""
    os.makedirs(outdir, exist_ok=True)
    new_cs = os.path.join(outdir, "callsets.json")
    names = rewrite_callsets(callsets_path, new_cs, lambda f, k: os.path.splitext(f)[0] + ".vcf")
    for old, new in names.items():
        with open(os.path.join(outdir, new), "wb") as f:
            f.write(bcf2text.stream_to_vcf_text(streams[old], fmt9))
    return new_cs


def hostile_streams(data):
    """three malformed variants of a valid plain stream with at least two records -> {kind: (stream, 1-based record number it names)}:
    the last record truncated, an unknown type code (4) in the ID descriptor of record 2, and a FILTER dictionary id of 127 in record 2"""
    hdr, recs = bcf2text.parse_stream(data)
    begin = len(data) - sum(len(r) for r in recs)
    at = begin + len(recs[0])
    r = bytearray(recs[1])
    p = 8 + 24
    bad_type = bytearray(data)
    bad_type[at + p] = (r[p] & 0xF0) | 4
    n_allele = struct.unpack_from("<I", r, 8 + 16)[0] >> 16
    for _ in range(1 + n_allele):       # ID and the alleles
        n, t, p = bcf2text._typed_descriptor(r, p)
        p += n
    n, t, p = bcf2text._typed_descriptor(r, p)
    if n < 1 or t != bcf2text.BT_INT8:
        raise ValueError("record 2 needs a FILTER of int8 ids")
    bad_dict = bytearray(data)
    bad_dict[at + p + n - 1] = 127
    return {"truncated": (bytes(data[:-5]), len(recs)), "type_code": (bytes(bad_type), 2), "dictionary_id": (bytes(bad_dict), 2)}
