// hostsim_import_bcf.cc - C entry of the CPU harness of the device importer's BCF2 path (hostsim_import_bcf.hpp), for the tests.
#include "hostsim_import_bcf.hpp"

#include "../../genomicsdb_amd/csrc/common/gz_text.hpp"
#include "../../genomicsdb_amd/csrc/common/mini_json.hpp"

using namespace genomicsdb_amd;

namespace {
thread_local std::string g_error;
}

extern "C" {

const char* hsb_last_error(void) { return g_error.c_str(); }

// the files of the callset mapping are BCF2 (plain, gzip or BGZF); stats: files, records, cells, spanning cells, batches
int hsb_import(const char* vid_file, const char* callsets_file, const char* file_root, int treat_deletions_as_intervals, int64_t column_begin, int64_t column_end,
               uint64_t budget, uint8_t** cells, uint64_t* nbytes, int64_t* stats) {
  try {
    VidMapper vid;
    vid.parse_vid_json(mini_json::parse_file(vid_file));
    vid.parse_callsets_json(mini_json::parse_file(callsets_file));
    ImportOptions opt;
    opt.treat_deletions_as_intervals = treat_deletions_as_intervals != 0;
    opt.column_begin = column_begin; opt.column_end = column_end;
    if (file_root) opt.file_root = file_root;
    hostsim_bcf::Stats st;
    const std::vector<uint8_t> out = hostsim_bcf::run(vid, opt, budget ? budget : (uint64_t)64 << 20, [](const ImportFile& f) {
      try { return gz_text::read_all(f.path); } catch (const std::exception& e) { throw VCF2BinaryException(e.what()); }
    }, &st);
    *cells = (uint8_t*)malloc(out.size() ? out.size() : 1);
    if (!out.empty()) memcpy(*cells, out.data(), out.size());
    *nbytes = out.size();
    if (stats) { stats[0] = st.files; stats[1] = st.records; stats[2] = st.cells; stats[3] = st.spanning; stats[4] = st.batches; }
    g_error.clear();
    return 0;
  } catch (const std::exception& e) { g_error = e.what(); return -1; }
}
void hsb_free(void* p) { free(p); }

}  // extern "C"
