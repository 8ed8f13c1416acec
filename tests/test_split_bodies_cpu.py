"""The bodies of the device splitter (csrc/core/gdb_split.hpp; vcf2tiledb --split-files) on the CPU, through the stand-alone program
tests/hostsim_split (built with the address and undefined-behaviour sanitizers, run as a subprocess), against the plain-Python model
tests/tools/split_model.py, which never calls the code under test:
  check 1  bodies == model on (a) t0,t1,t2 at 0 / 12200 / 17385, (b) t6,t7,t8 at 0 / 8029500 / 8029501, (c) a hand-made file;
  check 2  round trip through the HOST importer with the model's split text: importing the split files of partition p for partition
           p gives the cells of importing the originals for p, byte for byte, wherever the precondition of the round trip holds -
           it holds on (a) and (b); t0_overlapping at 12202 is the reference's own counter-example and falls the other way;
  check 3  a line error names file and line; check 4 "split_files_paths"; check 5 malformed variants of the hand-made file.
Host code only - no device."""
import gzip
import json
import os
import subprocess

import pytest

import helpers
import split_inputs as si
from split_inputs import split_model


@pytest.fixture(scope="module")
def gdb():
    from genomicsdb_amd import build as b
    b.build_native()
    import genomicsdb_amd
    return genomicsdb_amd


@pytest.fixture(scope="module")
def prog():
    from genomicsdb_amd import build as b
    return b.build_hostsim_split()


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return si.input_sets(tmp_path_factory.mktemp("split_sets"))


def run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.decode()


def sim_split(prog, out_dir, vid, callsets, root, parts, extra=()):
    os.makedirs(out_dir, exist_ok=True)
    return run(prog, "split", vid, callsets, root or "-", out_dir, ",".join(str(b) for b, _ in parts), ",".join(str(e) for _, e in parts), *extra)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_bodies_equal_the_model(prog, sets, tmp_path, name):
    vid, callsets, root, names, begins = sets[name]
    model, parts = si.model_of(vid, root, names, begins)
    si.assert_model_is_interesting(model, names, len(parts))
    out = sim_split(prog, str(tmp_path), vid, callsets, root, parts)
    assert "error" not in out, out
    for i, fn in enumerate(names):
        for p in range(len(parts)):
            got = open(os.path.join(str(tmp_path), "f%d_p%d.txt" % (i, p)), "rb").read()
            assert got == model[(fn, p)], (fn, p)


def test_the_hand_made_file_holds_every_case(sets):
    vid, callsets, root, names, begins = sets["c"]
    model, parts = si.model_of(vid, root, names, begins)
    lines = [ln for ln in si.HAND_LINES if not ln.startswith("#")]
    where = {i: [p for p in range(5) if (ln.encode() + b"\n") in model[(names[0], p)]] for i, ln in enumerate(lines)}
    assert [where[i] for i in range(len(lines))] == [[4], [0, 1, 2], [0], [0, 1], [0, 1], [1], [1, 2], [1], [1], [2], [2]]
    assert model[(names[0], 1)].count(b"\r\n") == 1 and model[(names[0], 2)].endswith(b"DP=11\t" + si._FMT.encode() + b"\t0/0:3:9:3:0,9,90\t0/0:5:12:4:0,12,120\n")
    assert not si.hand_text().endswith(b"\n") and si.is_header_only(model[(names[0], 3)])


def _write_split_set(dirname, model, names, p, callsets):
    """the model's text of partition p as files, and a callset mapping that names them -> its path"""
    os.makedirs(dirname, exist_ok=True)
    cs = json.load(open(callsets))
    for i, fn in enumerate(names):
        with gzip.open(os.path.join(dirname, "p%d_f%d.vcf.gz" % (p, i)), "wb") as f:
            f.write(model[(fn, p)])
    for v in cs["callsets"].values():
        v["filename"] = "p%d_f%d.vcf.gz" % (p, names.index(v["filename"]))
    path = os.path.join(dirname, "callsets_p%d.json" % p)
    with open(path, "w") as f:
        json.dump(cs, f)
    return path


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_round_trip_through_the_host_importer(gdb, sets, tmp_path, name):
    vid, callsets, root, names, begins = sets[name]
    model, parts = si.model_of(vid, root, names, begins)
    offsets = split_model.contig_offsets(vid)
    checked = 0
    for p, part in enumerate(parts):
        holds = all(split_model.round_trip_precondition(split_model.read_text(os.path.join(root, fn)), offsets, part) for fn in names)
        if name in ("a", "b"):
            assert holds, (name, p)
        if not holds:
            continue
        cp = _write_split_set(str(tmp_path), model, names, p, callsets)
        want = gdb.import_cells(vid, callsets, file_root=root, column_begin=part[0], column_end=part[1])
        got = gdb.import_cells(vid, cp, file_root=str(tmp_path), column_begin=part[0], column_end=part[1])
        assert got[1] == want[1] and got[0] == want[0], (name, p)
        checked += 1
    assert checked >= 2


def test_t0_overlapping_at_12202_falls_the_other_way(gdb, tmp_path):
    """The reference's own t0_overlapping_at_12202 run: t0_overlapping.vcf.gz holds a record nested inside a longer one of the same
    sample.  The model says which way the round trip falls (split_model.replay_differs), the host importer's two results must agree."""
    vid, callsets, root, names = si.golden_set("t0_overlapping.json")
    part = (12202, si.LAST_END)
    offsets = split_model.contig_offsets(vid)
    texts = [split_model.read_text(os.path.join(root, fn)) for fn in names]
    holds = all(split_model.round_trip_precondition(t, offsets, part) for t in texts)
    differs = any(split_model.replay_differs(t, offsets, part) for t in texts)
    model = {(fn, 0): split_model.split_text(t, offsets, [part])[0] for fn, t in zip(names, texts)}
    cp = _write_split_set(str(tmp_path), model, names, 0, callsets)
    want = gdb.import_cells(vid, callsets, file_root=root, column_begin=part[0], column_end=part[1])
    got = gdb.import_cells(vid, cp, file_root=str(tmp_path), column_begin=part[0], column_end=part[1])
    print("t0_overlapping at 12202: precondition holds = %s, model says differs = %s, cells %d (originals) / %d (split)" % (holds, differs, want[1], got[1]))
    assert (got[0] != want[0]) == differs


BAD = [("unknown contig", lambda cols: ["chrUn"] + cols[1:], "contig chrUn is not in the vid mapping"),
       ("POS = x", lambda cols: cols[:1] + ["x"] + cols[2:], "POS"),
       ("7 columns", lambda cols: cols[:7], "short record line")]


@pytest.mark.parametrize("what,change,words", BAD, ids=[b[0] for b in BAD])
def test_errors_name_file_and_line(prog, tmp_path, what, change, words):
    lines = list(si.HAND_LINES)
    lines[7] = "\t".join(change(lines[7].split("\t")))        # physical line 8
    vid, callsets, root, names = si.write_hand(str(tmp_path / "in"), "\n".join(lines).encode())
    out = sim_split(prog, str(tmp_path / "out"), vid, callsets, root, split_model.derive_partitions(si.HAND_BEGINS, si.LAST_END))
    assert out.startswith("error: "), out
    assert words in out and "hand_split.vcf line 8" in out, out
    assert not os.listdir(str(tmp_path / "out"))


def test_split_files_paths(prog, tmp_path):
    cs = {"callsets": {"A": {"row_idx": 0, "idx_in_file": 0, "filename": "/data/in/a.vcf.gz"}, "B": {"row_idx": 1, "idx_in_file": 0, "filename": "b.vcf.gz"},
                       "C": {"row_idx": 2, "idx_in_file": 0, "filename": "sub/c.vcf.gz"}},
          "split_files_paths": {"/data/in/a.vcf.gz": ["/x/a0.vcf.gz", "/x/a1.vcf.gz"], "b.vcf.gz": "/y/only_b.vcf.gz"}}
    cp = str(tmp_path / "cs.json")
    json.dump(cs, open(cp, "w"))
    assert run(prog, "paths", cp, "/data/in/a.vcf.gz", "-", 1) == "/x/a1.vcf.gz\n"
    assert run(prog, "paths", cp, "/data/in/a.vcf.gz", "/res", 0) == "/x/a0.vcf.gz\n"
    out = run(prog, "paths", cp, "/data/in/a.vcf.gz", "-", 2)
    assert out.startswith("error: ") and "had 2 entries" in out and "index 2" in out
    assert run(prog, "paths", cp, "b.vcf.gz", "/res", 5) == "/y/only_b.vcf.gz\n"
    assert run(prog, "paths", cp, "sub/c.vcf.gz", "-", 3) == "sub/partition_3_c.vcf.gz\n"
    assert run(prog, "paths", cp, "sub/c.vcf.gz", "/res", 3) == "/res/partition_3_c.vcf.gz\n"
    assert run(prog, "paths", cp, "plain.vcf", "-", 0) == "./partition_0_plain.vcf\n"
    cs["split_files_paths"] = ["not", "a", "dictionary"]
    json.dump(cs, open(cp, "w"))
    assert run(prog, "paths", cp, "b.vcf.gz", "-", 0).startswith("error: ")


def test_malformed_variants_end_with_a_split_or_a_named_error(prog, tmp_path):
    """the sanitized program on the hand-made file, on truncations of it and on garbled copies: status 0 (run() asserts it), and
    either every output or a named error"""
    whole = si.hand_text()
    parts = split_model.derive_partitions(si.HAND_BEGINS, si.LAST_END)
    variants = [whole] + [whole[:n] for n in (0, 1, 57, 200, 330, 331, 400, 555, len(whole) - 1)]
    for k in range(12):
        g = bytearray(whole)
        for j in range(1 + k):
            at = (7919 * (k + 1) * (j + 3)) % len(g)
            g[at] = b"\t\n;=\rE\x00\xff9-"[(k + j) % 10]
        variants.append(bytes(g))
    splits = errors = 0
    for i, text in enumerate(variants):
        vid, callsets, root, names = si.write_hand(str(tmp_path / ("in%d" % i)), text)
        out = sim_split(prog, str(tmp_path / ("out%d" % i)), vid, callsets, root, parts)
        if out.startswith("error: "):
            errors += 1
            assert "hand_split.vcf" in out or "idx_in_file" in out, out
        else:
            splits += 1
            assert sorted(os.listdir(str(tmp_path / ("out%d" % i)))) == ["f0_p%d.txt" % p for p in range(5)]
    assert splits >= 2 and errors >= 2
