"""In-tree build of libgenomicsdb_amd.so (HIP kernels for gfx950 + host layer + C ABI) with hipcc.

hipcc cross-compiles gfx950 without a GPU; the .so lands next to this file so that it travels with the
repo snapshot to the GPU box.  Also builds the test oracle (oracle/Makefile) and the hostsim harness.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
OBJ = os.path.join(ROOT, "build", "obj")
LIB = os.path.join(PKG, "libgenomicsdb_amd.so")
TOOL = os.path.join(PKG, "gt_mpi_gather")
TOOLS = {"gt_mpi_gather": TOOL, "vcf2tiledb": os.path.join(PKG, "vcf2tiledb"), "test_genomicsdb_importer": os.path.join(PKG, "test_genomicsdb_importer"),
         "vcf_histogram": os.path.join(PKG, "vcf_histogram"), "vcfdiff": os.path.join(PKG, "vcfdiff")}

SOURCES = [
    "kernels/gdb_pipeline.hip",
    "kernels/gdb_bgzf.hip",
    "kernels/gdb_import.hip",
    "kernels/gdb_import_stream.hip",
    "kernels/gdb_inflate.hip",
    "kernels/gdb_merge.hip",
    "kernels/gdb_split.hip",
    "kernels/gdb_histogram.hip",
    "kernels/gdb_index.hip",
    "kernels/gdb_output_index.hip",
    "kernels/gdb_vcfdiff.hip",
    "kernels/gdb_columns.hip",
    "host/vid_mapper.cc",
    "host/variant_query_config.cc",
    "host/combine_plan.cc",
    "host/fragment.cc",
    "host/reference_genome.cc",
    "host/vcf_importer.cc",
    "host/vcf_index.cc",
    "host/bgzf_host.cc",
    "api/genomicsdb_bcf_generator.cc",
    "api/genomicsdb_operators.cc",
    "api/genomicsdb_importer.cc",
    "api/loader_outputs.cc",
    "api/capi.cc",
]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-gline-tables-only", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


def _headers():
    out = []
    for d, _, fs in os.walk(CSRC):
        out += [os.path.join(d, f) for f in fs if f.endswith((".h", ".hpp", ".inc"))]
    out.append(os.path.join(ROOT, "include", "genomicsdb_amd.h"))
    return out


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_native(verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    hdrs = _headers()
    objs, stale = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(OBJ, s.replace("/", "_") + ".o")
        objs.append(obj)
        if _newer(obj, [src] + hdrs):
            stale.append([HIPCC] + FLAGS + (["-x", "hip"] if s.endswith(".hip") else []) + ["-c", src, "-o", obj])

    def compile_one(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    # the translation units are independent: a few at a time (MAX_JOBS, else up to 8, never more than the machine has)
    jobs = max(1, min(int(os.environ.get("MAX_JOBS", "8")), os.cpu_count() or 1, len(stale) or 1))
    with ThreadPoolExecutor(jobs) as pool:
        list(pool.map(compile_one, stale))
    if _newer(LIB, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-lz"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    # command lines of the reference's query tool (--produce-Broad-GVCF mode) and import tool, linked against the library
    for name, exe in TOOLS.items():
        tool_src = os.path.join(CSRC, "tools", name + ".cc")
        if _newer(exe, [tool_src, LIB] + hdrs):
            cmd = [HIPCC, "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", tool_src, "-o", exe, "-L" + PKG, "-lgenomicsdb_amd", "-Wl,-rpath,$ORIGIN", "-lz"]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
    build_jni(verbose)
    return LIB


def build_jni(verbose=False):
    """libtiledbgenomicsdb.so (the name the reference's Java loader asks for) = the GenomicsDBQueryStream natives, the
    GenomicsDBImporter natives (jni_importer.cc) and the one-time initialiser over the C ABI.  Compiled against a JDK's jni.h when $JAVA_HOME has one, else against the minimal
    stand-in csrc/jni/stub/jni.h (specification function-table indices only), so the glue is built and symbol-checked always."""
    jh = os.environ.get("JAVA_HOME", "")
    inc = os.path.join(jh, "include") if jh else ""
    if inc and os.path.exists(os.path.join(inc, "jni.h")):
        incs = ["-I" + inc, "-I" + os.path.join(inc, "linux")]
    else:
        incs = ["-I" + os.path.join(CSRC, "jni", "stub")]
    out = os.path.join(PKG, "libtiledbgenomicsdb.so")
    srcs = [os.path.join(CSRC, "jni", "jni_query_stream.cc"), os.path.join(CSRC, "jni", "jni_importer.cc")]
    if _newer(out, srcs + [LIB, os.path.join(CSRC, "jni", "stub", "jni.h"), os.path.join(ROOT, "include", "genomicsdb_amd.h")]):
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall"] + incs + srcs + ["-o", out, "-L" + PKG, "-lgenomicsdb_amd", "-Wl,-rpath,$ORIGIN"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return out


def build_oracle():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    return os.path.join(ROOT, "oracle", "liboracle_gvcf.so")


def build_hostsim():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostsim")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "jni_harness")])   # JVM-less driver of the JNI glue (tests only)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "compat")])        # reference-shaped C++ caller (tests only)


def build_hostsim_variants():
    """CPU harness around the bodies of the variants query (core/gdb_variants.hpp; tests only)"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostsim_variants")])
    return os.path.join(ROOT, "tests", "hostsim_variants", "libhostsim_variants.so")


def build_hostsim_import():
    """CPU harness around the bodies of the device importer (core/gdb_import.hpp; tests only)"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostsim_import")])
    return os.path.join(ROOT, "tests", "hostsim_import", "libhostsim_import.so")


def build_hostsim_import_bcf():
    """CPU harness around the bodies of the device importer's BCF2 path (core/gdb_import_bcf.hpp) and the stand-alone
    malformed-input program built with the address and undefined-behaviour sanitizers (tests only); -> (library, program)"""
    d = os.path.join(ROOT, "tests", "hostsim_import_bcf")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "libhostsim_import_bcf.so"), os.path.join(d, "malformed_bcf")


def build_hostsim_import_csv():
    """CPU harness around the bodies of the device importer's CSV path (core/gdb_import_csv.hpp) and the same source as a
    stand-alone program built with the address and undefined-behaviour sanitizers (tests only); -> (library, program)"""
    d = os.path.join(ROOT, "tests", "hostsim_import_csv")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "libhostsim_import_csv.so"), os.path.join(d, "hostsim_import_csv_main")


def build_hostsim_import_stream():
    """CPU harness around the bodies of the streaming importer (core/gdb_import_stream.hpp) and the same source as a stand-alone
    program built with the address and undefined-behaviour sanitizers (tests only); -> (library, program)"""
    d = os.path.join(ROOT, "tests", "hostsim_import_stream")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "libhostsim_import_stream.so"), os.path.join(d, "hostsim_import_stream_main")


def build_jni_importer_harness():
    """JVM-less driver of the GenomicsDBImporter natives in libtiledbgenomicsdb.so (tests only); -> program"""
    d = os.path.join(ROOT, "tests", "jni_importer_harness")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "jni_importer_harness")


def build_hostsim_merge():
    """CPU harness around the bodies of the cell-stream merge (core/gdb_merge.hpp) and the same source as a stand-alone program
    built with the address and undefined-behaviour sanitizers (tests only); -> (library, program)"""
    d = os.path.join(ROOT, "tests", "hostsim_merge")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "libhostsim_merge.so"), os.path.join(d, "hostsim_merge_main")


def build_hostsim_merge_files():
    """CPU harness of the windowed merge (host/merge_files_common.hpp's planner and round loop over pools in host memory, the bodies
    of core/gdb_merge.hpp) and the same source as a stand-alone program built with the address and undefined-behaviour sanitizers
    (tests only); -> (library, program)"""
    d = os.path.join(ROOT, "tests", "hostsim_merge_files")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "libhostsim_merge_files.so"), os.path.join(d, "hostsim_merge_files_main")


def build_hostsim_split():
    """The bodies of the device splitter (core/gdb_split.hpp) as a stand-alone program built with the address and
    undefined-behaviour sanitizers (tests only); -> program"""
    d = os.path.join(ROOT, "tests", "hostsim_split")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "hostsim_split")


def build_hostsim_histogram():
    """The bodies of the input histogram (core/gdb_histogram.hpp) as a stand-alone program built with the address and
    undefined-behaviour sanitizers (tests only); -> program"""
    d = os.path.join(ROOT, "tests", "hostsim_histogram")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "hostsim_histogram")


def build_hostsim_index():
    """CPU harness around the bodies of the device tabix builder (core/gdb_index.hpp) with the shared serialiser, and the same source
    as a stand-alone program built with the address and undefined-behaviour sanitizers (tests only); -> (library, program)"""
    d = os.path.join(ROOT, "tests", "hostsim_index")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "libhostsim_index.so"), os.path.join(d, "hostsim_index")


def build_hostsim_output_index():
    """CPU harness around the bodies of the device builder of the output's index (core/gdb_output_index.hpp) with the shared page
    merger and serialisers, and the same source as a stand-alone program built with the address and undefined-behaviour sanitizers
    (tests only); -> (library, program)"""
    d = os.path.join(ROOT, "tests", "hostsim_output_index")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "libhostsim_output_index.so"), os.path.join(d, "hostsim_output_index")


def build_hostsim_vcfdiff():
    """The bodies of the device vcfdiff (core/gdb_vcfdiff.hpp) as a stand-alone program built with the address and
    undefined-behaviour sanitizers (tests only); -> program"""
    d = os.path.join(ROOT, "tests", "hostsim_vcfdiff")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "hostsim_vcfdiff")


def build_hostsim_columns():
    """CPU harness around the bodies of the column decoder (core/gdb_columns.hpp) and the same source as a stand-alone program
    built with the address and undefined-behaviour sanitizers (tests only); -> (library, program)"""
    d = os.path.join(ROOT, "tests", "hostsim_columns")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "libhostsim_columns.so"), os.path.join(d, "hostsim_columns_main")


def build_hostsim_numtext():
    """CPU harness around the number-text bodies, the ALT token iterator (core/gdb_core.hpp) and the first-cell table of the site pass
    (core/gdb_stages.hpp), and the same source as a stand-alone program built with the address and undefined-behaviour sanitizers
    (tests only); -> (library, program)"""
    d = os.path.join(ROOT, "tests", "hostsim_numtext")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "libhostsim_numtext.so"), os.path.join(d, "hostsim_numtext_main")


def build_hostsim_inflate():
    """CPU harness around the bodies of the BGZF inflater (core/gdb_inflate.hpp; tests only)"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostsim_inflate")])
    return os.path.join(ROOT, "tests", "hostsim_inflate", "libhostsim_inflate.so")


def build_hostsim_tile_inflate():
    """CPU harness around the body of the tile inflater of compressed fragment files (core/gdb_tile_inflate.hpp) and a stand-alone
    driver of the same body built with the address and undefined-behaviour sanitizers (tests only); -> (library, program)"""
    d = os.path.join(ROOT, "tests", "hostsim_tile_inflate")
    subprocess.check_call(["make", "-s", "-C", d])
    return os.path.join(d, "libhostsim_tile_inflate.so"), os.path.join(d, "tile_inflate_fuzz")


def build_hostsim_dispatch():
    """CPU harness around the choice of an interval's sizing and page kernels (kernels/gdb_assembly_choice.hpp; tests only)"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostsim_dispatch")])
    return os.path.join(ROOT, "tests", "hostsim_dispatch", "libhostsim_dispatch.so")


if __name__ == "__main__":
    print(build_native(verbose=True))
    print(build_oracle())
