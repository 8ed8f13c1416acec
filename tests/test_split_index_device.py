"""split_files(..., index_on_device=True): every output's .tbi is built on the GPU while the output is written (kernels/gdb_index.hip), from
the packed text that is still in device memory and the blocks the deflate just made.  The outputs equal those of index_on_device=False
byte for byte, and every .tbi equals what the host builder writes for that output - on the hand-made file and on one seeded synthetic
set, read as plain text and as BGZF, for all partitions and for one, with one flush per output and with many.  Then the command line."""
import json
import os
import subprocess
import sys

import pytest

import helpers
import split_inputs as si

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bgzf_write  # noqa: E402
import synth_gvcf_text  # noqa: E402

pytestmark = pytest.mark.gpu

SYNTH_BEGINS = [0, 1800000, 6801064]      # as in test_split_device.py: a record of every file spans each cut


@pytest.fixture(scope="module")
def gdb():
    import genomicsdb_amd
    return genomicsdb_amd


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """-> {(set, form): (vid, callsets, file root, partitions)}"""
    base = tmp_path_factory.mktemp("split_index")
    out = {}
    vid, callsets, root, names = si.write_hand(str(base / "hand"))
    out[("hand", "plain")] = (vid, callsets, root, si.split_model.derive_partitions(si.HAND_BEGINS, si.LAST_END))
    plain = str(base / "synth_plain")
    vid, callsets = synth_gvcf_text.write_inputs(plain, n_files=2, n_lines=2000, multi=1)
    parts = si.split_model.derive_partitions(SYNTH_BEGINS, si.LAST_END)
    out[("synth", "plain")] = (vid, callsets, plain, parts)
    bg = str(base / "synth_bgzf")
    os.makedirs(bg)
    for fn in ("s0000.g.vcf", "s0001.g.vcf", "multi.vcf"):
        bgzf_write.write_file(os.path.join(bg, fn), open(os.path.join(plain, fn), "rb").read(), member_size=700, level=1)
    out[("synth", "bgzf")] = (vid, callsets, bg, parts)
    return out


def host_tbi(path, scratch):
    """the host builder's file for a copy of the output"""
    from genomicsdb_amd import _lib
    copy = os.path.join(scratch, "copy_" + os.path.basename(path))
    with open(copy, "wb") as f:
        f.write(open(path, "rb").read())
    assert _lib.lib().gdbamd_build_output_index(os.fsencode(copy), 0) == 0, _lib.last_error()
    return open(copy + ".tbi", "rb").read()


@pytest.mark.parametrize("budget", [0, 4096], ids=["one_flush", "many_flushes"])
@pytest.mark.parametrize("produce", [None, 1], ids=["all_partitions", "partition_1"])
@pytest.mark.parametrize("which", [("hand", "plain"), ("synth", "plain"), ("synth", "bgzf")], ids=["hand", "synth_plain", "synth_bgzf"])
def test_outputs_and_indexes_equal_the_host_paths(gdb, inputs, tmp_path, which, produce, budget):
    vid, callsets, root, parts = inputs[which]
    res = {}
    stats = {}
    for on in (False, True):
        d = str(tmp_path / ("device" if on else "host"))
        os.makedirs(d)
        stats[on] = {}
        res[on] = gdb.split_files(vid, callsets, parts, results_directory=d, file_root=root, produce=produce, text_budget_bytes=budget, stats=stats[on],
                                  index_on_device=on)
    assert sorted(res[True]) == sorted(res[False]) and len(res[True]) >= 1
    scratch = str(tmp_path / "scratch")
    os.makedirs(scratch)
    for key, path in res[True].items():
        other = res[False][key]
        assert open(path, "rb").read() == open(other, "rb").read(), key
        tbi = open(path + ".tbi", "rb").read()
        assert tbi == host_tbi(path, scratch), key
        assert tbi == open(other + ".tbi", "rb").read(), key
    assert sorted(os.listdir(str(tmp_path / "device"))) == sorted(os.listdir(str(tmp_path / "host")))      # no temporary file is left
    print(which, produce, budget, {k: stats[True][k] for k in ("s_index_build", "ms_index_kernels", "s_total")}, stats[False]["s_index_build"])
    for k in ("num_files", "num_record_lines", "num_lines_written", "text_bytes_out", "compressed_bytes_out", "num_batches"):
        assert stats[True][k] == stats[False][k], k
    assert stats[False]["ms_index_kernels"] == 0 and stats[False]["s_index_build"] > 0
    assert stats[True]["s_index_build"] > 0
    if stats[True]["num_lines_written"]:
        assert stats[True]["ms_index_kernels"] > 0


def test_command_line_flag(gdb, inputs, tmp_path):
    vid, callsets, root, parts = inputs[("synth", "bgzf")]
    loader = {"row_based_partitioning": False, "column_partitions": [{"begin": b, "workspace": str(tmp_path / "ws"), "array": "a%d" % i} for i, b in enumerate(SYNTH_BEGINS)],
              "callset_mapping_file": callsets, "vid_mapping_file": vid}
    lj = tmp_path / "loader.json"
    lj.write_text(json.dumps(loader))
    tool = os.path.join(os.path.dirname(gdb.__file__), "vcf2tiledb")
    dirs = {}
    for on in (False, True):
        d = tmp_path / ("device" if on else "host")
        d.mkdir()
        dirs[on] = d
        cmd = [tool, "--split-files", "--split-all-partitions", "--split-files-results-directory", str(d)] + (["--split-index-on-device"] if on else []) + [str(lj)]
        r = subprocess.run(cmd, cwd=root, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        timer = [ln for ln in r.stderr.decode().splitlines() if ",split_files," in ln]
        assert len(timer) == 1 and ",index_kernels_ms," in timer[0]
        assert (float(timer[0].rsplit(",", 1)[1]) > 0) == on
    names = sorted(os.listdir(str(dirs[True])))
    assert names == sorted(os.listdir(str(dirs[False]))) and len(names) == 2 * 3 * 3
    for n in names:
        assert (dirs[True] / n).read_bytes() == (dirs[False] / n).read_bytes(), n
