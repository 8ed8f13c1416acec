"""The bodies of the device tabix builder (csrc/core/gdb_index.hpp) on the CPU, no GPU needed: tests/hostsim_index runs them serially
over a file, batch by batch, and writes the .tbi through the serialiser the host builder uses.  For every input of tests/index_inputs.py
the file must equal what gdbamd_build_output_index writes for a copy of the same file, byte for byte, whatever the batch size; the
sanitized stand-alone program runs clean over all inputs.  Also the interface: symbols, header, signature."""
import ctypes
import inspect
import os
import subprocess

import pytest

import helpers
import index_inputs

HOSTSIM_DIR = os.path.join(helpers.ROOT, "tests", "hostsim_index")
STAT_NAMES = ("members", "batches", "lines", "records", "contigs", "bins", "chunks", "windows", "atomics")
CASES = index_inputs.cases()
BATCH_BYTES = (0, 1, 700, 5000)      # one batch; one line per batch; a few lines; a few dozen


@pytest.fixture(scope="module")
def sim():
    from genomicsdb_amd import build
    lib_path, prog = build.build_hostsim_index()
    lib = ctypes.CDLL(lib_path)
    lib.hostsim_index_build.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p, ctypes.c_uint64]
    return lib, prog


def host_tbi(tmp_path, data, name="host.vcf.gz"):
    """the yardstick: the host builder's file for a copy of the same file"""
    from genomicsdb_amd import _lib
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    L = _lib.lib()
    rc = L.gdbamd_build_output_index(os.fsencode(p), 0)
    assert rc == 0, _lib.last_error()
    with open(p + ".tbi", "rb") as f:
        return f.read()


def run_sim(lib, path, out, batch_bytes):
    st = (ctypes.c_uint64 * len(STAT_NAMES))()
    err = ctypes.create_string_buffer(2048)
    rc = lib.hostsim_index_build(os.fsencode(path), os.fsencode(out), batch_bytes, st, err, len(err))
    return rc, dict(zip(STAT_NAMES, (int(v) for v in st))), err.value.decode()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hostsim_writes_the_host_builders_bytes_whatever_the_batch_size(sim, tmp_path, name):
    lib, _ = sim
    want = host_tbi(tmp_path, CASES[name])
    p = str(tmp_path / "sim.vcf.gz")
    with open(p, "wb") as f:
        f.write(CASES[name])
    batches = set()
    for bb in BATCH_BYTES:
        out = str(tmp_path / ("sim_%d.tbi" % bb))
        rc, st, err = run_sim(lib, p, out, bb)
        assert rc == 0, err
        with open(out, "rb") as f:
            assert f.read() == want, (name, bb, st)
        batches.add(st["batches"])
    if name in ("runs", "batches", "windows", "info", "contigs"):
        assert max(batches) >= 3 and min(batches) == 1


def test_counts_of_the_run_and_contig_inputs(sim, tmp_path):
    lib, _ = sim
    # contigs: "a" 1 bin and, the interruption aside, 1 chunk; "b" 2 bins; "c" 2 bins (POS 5 * 16384 is the last base of window 4)
    for name, want in (("runs", dict(records=493, contigs=1, bins=5, chunks=5)), ("contigs", dict(records=16, contigs=3, bins=5, chunks=5))):
        p = str(tmp_path / (name + ".vcf.gz"))
        with open(p, "wb") as f:
            f.write(CASES[name])
        for bb in (0, 900):
            rc, st, err = run_sim(lib, p, p + ".tbi", bb)
            assert rc == 0, err
            assert {k: st[k] for k in want} == want, (name, bb, st)


def test_300_records_of_one_window_issue_few_atomics(sim, tmp_path):
    lib, _ = sim
    p = str(tmp_path / "w.vcf.gz")
    with open(p, "wb") as f:
        f.write(CASES["windows"])
    rc, st, err = run_sim(lib, p, p + ".tbi", 0)
    assert rc == 0, err
    # 305 records; the reference block alone covers 70 windows.  One atomic per (window, wavefront of 64 neighbours) that touches it
    assert st["records"] == 305 and st["atomics"] < 100, st


@pytest.mark.parametrize("name", sorted(index_inputs.refusals()))
def test_refusals_name_the_place_and_leave_nothing(sim, tmp_path, name):
    lib, _ = sim
    data, words, line = index_inputs.refusals()[name]
    p = str(tmp_path / "bad.vcf.gz")
    with open(p, "wb") as f:
        f.write(data)
    rc, _, err = run_sim(lib, p, p + ".tbi", 0)
    assert rc != 0 and words in err, err
    if line is not None:
        assert err.endswith("(%s line %d)" % (p, line)), err
    assert not os.path.exists(p + ".tbi")


def test_sanitized_program_runs_clean_over_all_inputs(sim, tmp_path):
    _, prog = sim
    inputs = dict(CASES)
    inputs["one_line_members"] = index_inputs.one_line_members()
    for k, (data, _, _) in index_inputs.refusals().items():
        inputs["refused_" + k] = data
    for name, data in sorted(inputs.items()):
        p = str(tmp_path / (name + ".vcf.gz"))
        with open(p, "wb") as f:
            f.write(data)
        for bb in (0, 1, 900):
            r = subprocess.run([prog, p, p + ".tbi", str(bb)], capture_output=True, timeout=120)
            assert r.returncode == 0 and not r.stderr, (name, bb, r.stderr.decode()[-2000:])
            assert r.stdout.startswith(b"stats " if not name.startswith("refused_") else b"error: "), (name, r.stdout)


def test_interface_symbols_header_and_signature():
    import genomicsdb_amd
    from genomicsdb_amd import _lib, api
    L = _lib.lib()
    for name in ("gdbamd_index_vcf_device", "gdbamd_split_files_device_index"):
        assert name in _lib.SYMBOLS and getattr(L, name)
    header = open(os.path.join(helpers.ROOT, "include", "genomicsdb_amd.h")).read()
    assert "int gdbamd_index_vcf_device(const char* path, int device, uint64_t text_budget_bytes, gdbamd_index_stats* stats);" in header
    assert "} gdbamd_index_stats;" in header and "int gdbamd_split_files_device_index(" in header
    assert str(inspect.signature(genomicsdb_amd.index_vcf)) == "(path, device=0, text_budget_bytes=0, stats=None)"
    assert inspect.signature(api.split_files).parameters["index_on_device"].default is False
    assert api.INDEX_STAT_NAMES == tuple(n for n, _ in _lib.IndexStats._fields_)
    for k in ("members", "batches", "lines", "records", "contigs", "bins", "chunks", "linear_windows", "text_bytes", "atomics", "ms_inflate", "ms_index",
              "ms_records", "ms_chunks", "ms_linear", "s_read", "s_serialize_write", "s_total"):
        assert k in api.INDEX_STAT_NAMES
    assert api.SPLIT_STAT_NAMES[-1] == "ms_index_kernels" and api.SPLIT_STAT_NAMES[14] == "s_index_build"
