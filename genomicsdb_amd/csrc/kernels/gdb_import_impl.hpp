// gdb_import_impl.hpp - the state of a DeviceImporter and the launches of its finish() kernels, for the two translation units that
// drive it: kernels/gdb_import.hip (whole files and streams, one sort in finish()) and kernels/gdb_import_stream.hip (buffer streams
// batch by batch).  The member functions and the kernels are defined in gdb_import.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <functional>
#include <string>
#include <vector>

#include "../host/import_bcf.hpp"
#include "../host/import_common.hpp"
#include "gdb_import.h"
#include "gdb_import_device.hpp"
#include "gdb_inflate.h"

namespace genomicsdb_amd {

struct DeviceImporter::Impl {
  int device = 0;
  ImportOptions opt;
  uint64_t budget = 0;
  ImportTablesHost H;
  std::vector<ImportFile> files;
  std::vector<std::string> skipped_files;      // "filename"s whose callsets all lie outside the row bounds: never opened
  ImportStats st;
  hipStream_t stream = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  // tables, uploaded once
  impdev::DBuf<char> d_names; impdev::DBuf<gdbimp::ImpName> d_contigs, d_fields; impdev::DBuf<gdbimp::ImpAttr> d_info, d_fmt;
  impdev::DBuf<unsigned long long> d_row_best, d_counters;
  impdev::DBuf<uint32_t> d_err, d_ndef;
  bool spanning = false; int seq_bits = 64; uint64_t line_seq = 0;
  bool spanning_slots = false;       // a batch whose slots take part in the partition-begin rule was queued (never a CSV batch)
  ImportTextTap tap; bool tapped = false;      // tapped: text batches go to tap.on_batch once indexed, no cell is made
  bool stage_in_lds = true;          // the A/B of profiles/device_import.md: -7.5 % on the write kernel; GDBAMD_IMPORT_STAGE_LDS=0|1 overrides
  // per batch, reused
  impdev::DBuf<char> d_text, d_tmp;
  impdev::DBuf<uint64_t> d_tile, d_tile_scan, d_size, d_off, d_patch_at;
  impdev::DBuf<uint32_t> d_nl, d_first_tab, d_tab, d_patch_val;
  impdev::DBuf<int64_t> d_col, d_end, d_samp_row;
  impdev::DBuf<int32_t> d_samp_idx;
  impdev::DBuf<uint8_t> d_kind;
  impdev::DBuf<gdbimp::ImpDeferred> d_def;
  // what stays until finish()
  struct Batch { uint64_t n_slots = 0, cells_bytes = 0; uint64_t* key = nullptr; uint64_t* src = nullptr; uint32_t* size = nullptr; uint64_t* tag = nullptr; uint8_t* cells = nullptr; };
  std::vector<Batch> batches;
  uint64_t total_slots = 0, total_cells = 0;
  bool finished = false;
  // the streaming importer's hook: called when a batch's cells are written and checked, while d_col and the batch's index are still
  // those of the batch (n_lines lines or records, per_line slots each; text: the batch is text with a newline index)
  std::function<void(uint32_t n_lines, uint32_t per_line, bool text)> after_batch;
  // BGZF input
  int inflate_mode = DeviceImporter::kInflateAuto;
  BgzfDeviceInflater inflater;
  impdev::DBuf<char> d_win[2];               // the window and the one the carried partial line moves to
  impdev::DBuf<unsigned long long> d_find;
  // BCF2 input: the file's tables, and per batch the record offsets and the index pass's tables
  impdev::DBuf<int32_t> d_dict_info, d_dict_fmt, d_dict_filter;
  impdev::DBuf<int64_t> d_contig_off;
  impdev::DBuf<uint32_t> d_rec_off;
  impdev::DBuf<gdbimp::ImpBcfRec> d_rec;
  impdev::DBuf<gdbimp::ImpBcfField> d_fld;

  gdbimp::ImpTables tables(int n_samples) const {
    gdbimp::ImpTables T = H.view(opt, n_samples);
    T.names = d_names.p; T.contigs = d_contigs.p; T.fields = d_fields.p; T.info = d_info.p; T.fmt = d_fmt.p;
    return T;
  }
  template <class T> void scan(const T* in, T* out, size_t n) {
    size_t bytes = 0;
    IMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, out, T(0), n, rocprim::plus<T>(), stream));
    d_tmp.ensure(std::max<size_t>(bytes, 16));
    IMP_HIP_CHECK(rocprim::exclusive_scan((void*)d_tmp.p, bytes, in, out, T(0), n, rocprim::plus<T>(), stream));
  }
  void free_batches() {
    for (Batch& b : batches) { if (b.key) (void)hipFree(b.key); if (b.src) (void)hipFree(b.src); if (b.size) (void)hipFree(b.size); if (b.tag) (void)hipFree(b.tag); if (b.cells) (void)hipFree(b.cells); }
    batches.clear();
  }
  // text: host text to upload, or null when the batch is already in d_text; -> lines of the batch
  // n_csv_rows >= 0: the lines are those of a CSV cell file, and d_samp_row holds that many rows of the file, ascending
  uint32_t batch(const ImportFile& file, const ImportHeader& hdr, const char* text, size_t n, bool add_newline, int64_t lines_before, int n_imp, int n_csv_rows = -1);
  int upload_samples(const ImportHeader& hdr);                              // -> imported samples of the file
  void append_vcf_path(const ImportFile& file, double t0);                  // a file of VCF text: BGZF to the device as it is, else inflated here
  void append_text(const ImportFile& file, const std::string& text);        // inflated text of a whole file, on the host
  void append_bgzf(const ImportFile& file, const std::string& raw, const std::vector<BgzfMember>& mem);
  void append_bcf(const ImportFile& file, const char* data, size_t n);      // a whole BCF2 stream, inflated
  // the tables of a BCF2 header, uploaded (they stay the file's until the next call); then the records data[offs[k] .. offs[k+1]),
  // cut into batches; records_before: records of the file in front of offs[0], for messages
  gdbimp::ImpBcfTables upload_bcf_tables(const BcfHeaderHost& hdr);
  void bcf_batches(const ImportFile& file, const BcfHeaderHost& hdr, const gdbimp::ImpBcfTables& BT, int n_imp, const char* data, const std::vector<uint64_t>& offs,
                   uint64_t records_before);
  void append_csv(const ImportFile& file, const char* data, size_t n);      // a whole CSV cell file
  const ImportFile& file_named(const std::string& filename) const;
  // measure, layout and write of the n_lines x max(n_imp, 1) slots of a batch whose index pass is queued (ev[0], ev[1] recorded).
  // host_text: the batch's text for the deferred tokens; describe(bit, line) / where(line): the words of an error
  struct BatchWords {
    std::function<const char*()> host_text; size_t n_text = 0;
    std::function<std::string(uint32_t, uint32_t)> describe;
    std::function<std::string(uint32_t)> where;
  };
  template <class Src> void cells_of_batch(const Src& src, const gdbimp::ImpTables& T, uint32_t n_lines, int n_imp, const BatchWords& words, bool text);
  void find_newlines(const char* text, uint64_t lo, uint64_t mid, uint64_t hi, uint64_t* last_below, uint64_t* first_above);
};

namespace impdev {
// the kernels finish() ends with, for the streaming importer's emit step (defined in gdb_import.hip)
void launch_iota(uint32_t* v, uint64_t n, hipStream_t s);
void launch_sorted_sizes(const uint32_t* idx, const uint32_t* size, uint64_t kept, uint64_t* out /* kept + 1 */, hipStream_t s);
void launch_gather(const uint32_t* idx, const uint64_t* src, const uint32_t* size, const uint64_t* off, uint64_t kept, uint8_t* out, uint64_t out_bytes, hipStream_t s);
}  // namespace impdev

}  // namespace genomicsdb_amd
