// loader_outputs.cc - see loader_outputs.h
#include "loader_outputs.h"

#include <sys/stat.h>

#include <chrono>
#include <cstdio>
#include <iostream>

#include "../host/vcf_importer.h"
#include "genomicsdb_bcf_generator.h"

namespace genomicsdb_amd {

namespace {
void mkdir_p(const std::string& path) {
  for (size_t i = 1; i <= path.size(); ++i)
    if (i == path.size() || path[i] == '/') mkdir(path.substr(0, i).c_str(), 0755);
}
bool wants(const mini_json::Value& doc, const char* key) { return doc.HasMember(key) && doc[key].GetBool(); }
bool merges(const GenomicsDBImportConfig& loader, const std::string& array_file, struct stat* have) {
  return loader.m_has_delete_and_create_tiledb_array && !loader.m_delete_and_create_tiledb_array && ::stat(array_file.c_str(), have) == 0;
}
double since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); }
}  // namespace

std::string loader_array_directory(const GenomicsDBImportConfig& loader, int rank) {
  const std::string dir = loader.get_workspace(rank) + "/" + loader.get_array_name(rank);
  mkdir_p(dir);
  return dir;
}

bool loader_outputs_need_cells(const mini_json::Value& doc, const GenomicsDBImportConfig& loader, int rank) {
  if (loader.m_produce_combined_vcf) return true;
  if (!wants(doc, "produce_tiledb_array")) return false;
  struct stat have;
  return wants(doc, "compress_tiledb_array") || merges(loader, loader.get_workspace(rank) + "/" + loader.get_array_name(rank) + "/cells.bin", &have);
}

void produce_loader_outputs(const LoaderOutputs& out, const mini_json::Value& doc, const GenomicsDBImportConfig& loader, const std::vector<uint8_t>* cells_or_null) {
  const int rank = out.rank, device = out.device;
  const std::string& loader_text = out.loader_text;
  const ColumnRange part = loader.get_column_partition(rank);
  static const std::vector<uint8_t> none;
  if (!cells_or_null && (out.spooled_cells_file.empty() || loader_outputs_need_cells(doc, loader, rank)))
    throw GenomicsDBConfigException("the loader's outputs need the cells of the import in memory");
  const std::vector<uint8_t>& cells = cells_or_null ? *cells_or_null : none;
  if (wants(doc, "produce_tiledb_array")) {
    const std::string dir = loader_array_directory(loader, rank);
    const std::string array_file = dir + "/cells.bin";
    struct stat have;
    const bool merge = merges(loader, array_file, &have);
    std::vector<uint8_t> merged;
    bool windowed = merge && out.merge_windowed;
    if (merge && !windowed) {      // the batch joins the cells the array holds: on the device, or not at all
      const auto tm = std::chrono::steady_clock::now();
      std::vector<uint8_t> old((size_t)have.st_size);
      FILE* in = fopen(array_file.c_str(), "rb");
      if (!in) throw GenomicsDBConfigException("cannot read " + array_file);
      const size_t got = old.empty() ? 0 : fread(old.data(), 1, old.size(), in);
      fclose(in);
      if (got != old.size()) throw GenomicsDBConfigException("short read from " + array_file);
      MergeStats ms;
      std::vector<CellStream> streams(2);
      streams[0].data = old.data(); streams[0].nbytes = old.size();
      streams[1].data = cells.data(); streams[1].nbytes = cells.size();
      try {
        merged = merge_cell_streams_device(streams, device, &ms);
        std::cerr << "GENOMICSDB_TIMER,Rank," << rank << ",merge_tiledb_array,Wall-clock time(s)," << since(tm)
                  << ",streams," << ms.num_streams << ",cells_in," << ms.cells_in << ",cells_out," << ms.cells_out << ",bytes_out," << ms.bytes_out << ",tile," << ms.tile
                  << ",keys_ms," << ms.ms_keys << ",rank_ms," << ms.ms_rank << ",scan_ms," << ms.ms_scan << ",gather_ms," << ms.ms_gather << ",h2d_s," << ms.s_h2d
                  << ",d2h_s," << ms.s_d2h << ",merge_s," << ms.s_total << "\n";
      } catch (const VCF2BinaryException& e) {      // the sizes do not fit the device together: window by window, then
        if (std::string(e.what()).find("arrays larger than device memory are not merged") == std::string::npos) throw;
        std::cerr << out.tool << ": " << e.what() << "; merging window by window instead (--merge-window-bytes)\n";
        windowed = true;
      }
    }
    if (windowed) {      // cells.bin is read as a file, window by window, and never whole; the merge writes the new file itself
      const auto tm = std::chrono::steady_clock::now();
      std::vector<CellSource> sources(2);
      sources[0].path = array_file;
      sources[1].data = cells.data(); sources[1].nbytes = cells.size();
      MergeFilesOptions mo;
      mo.device = device; mo.window_bytes = out.merge_window_bytes;
      MergeFilesStats ms;
      merge_cell_files_device(sources, array_file, mo, &ms);
      std::cerr << "GENOMICSDB_TIMER,Rank," << rank << ",merge_tiledb_array_windowed,Wall-clock time(s)," << since(tm)
                << ",streams," << ms.num_streams << ",cells_in," << ms.cells_in << ",cells_out," << ms.cells_out << ",bytes_out," << ms.bytes_out << ",tile," << ms.tile
                << ",rounds," << ms.rounds << ",carried_cells," << ms.carried_cells << ",grown," << ms.grown << ",window_bytes," << ms.window_bytes
                << ",device_bytes_peak," << ms.device_bytes_peak << ",pinned_bytes," << ms.pinned_bytes << ",keys_ms," << ms.ms_keys << ",rank_ms," << ms.ms_rank
                << ",scan_ms," << ms.ms_scan << ",gather_ms," << ms.ms_gather << ",read_s," << ms.s_read << ",write_s," << ms.s_write << ",wait_device_s," << ms.s_wait_device
                << ",merge_s," << ms.s_total << "\n";
      if (!out.spooled_cells_file.empty()) remove(out.spooled_cells_file.c_str());
      if (wants(doc, "compress_tiledb_array")) {      // (the columnar file is built from the merged cells staged whole)
        struct stat now;
        FILE* in = fopen(array_file.c_str(), "rb");
        if (!in || ::stat(array_file.c_str(), &now) != 0) { if (in) fclose(in); throw GenomicsDBConfigException("cannot read " + array_file); }
        merged.resize((size_t)now.st_size);
        const size_t got = merged.empty() ? 0 : fread(merged.data(), 1, merged.size(), in);
        fclose(in);
        if (got != merged.size()) throw GenomicsDBConfigException("short read from " + array_file);
      }
    }
    const std::vector<uint8_t>& array_cells = merge ? merged : cells;
    if (windowed) {      // (written above)
    } else if (!merge && !out.spooled_cells_file.empty()) {      // the import wrote these very bytes batch by batch
      if (rename(out.spooled_cells_file.c_str(), array_file.c_str()) != 0) throw GenomicsDBConfigException("cannot rename " + out.spooled_cells_file + " to " + array_file);
    } else {
      const std::string write_to = merge ? array_file + ".merge.tmp" : array_file;
      FILE* f = fopen(write_to.c_str(), "wb");
      if (!f) throw GenomicsDBConfigException("cannot write " + write_to);
      if (!array_cells.empty() && fwrite(array_cells.data(), 1, array_cells.size(), f) != array_cells.size()) {
        fclose(f);
        if (merge) remove(write_to.c_str());
        throw GenomicsDBConfigException("short write to " + write_to);
      }
      if (fclose(f) != 0) throw GenomicsDBConfigException("cannot write " + write_to);
      if (merge && rename(write_to.c_str(), array_file.c_str()) != 0) { remove(write_to.c_str()); throw GenomicsDBConfigException("cannot rename " + write_to + " to " + array_file); }
      if (!out.spooled_cells_file.empty()) remove(out.spooled_cells_file.c_str());
    }
    remove((dir + "/fragment.gdbamd").c_str());   // a columnar copy of older cells must not shadow the new array
    // "compress_tiledb_array" (the reference's loader gzips the attribute tiles of the array it writes): the columnar fragment file with
    // its data sections as DEFLATE tiles goes next to cells.bin; queries read it window by window and inflate the tiles on the device
    if (wants(doc, "compress_tiledb_array") && !array_cells.empty()) {
      const auto tc = std::chrono::steady_clock::now();
      const size_t close_at = loader_text.rfind('}');
      if (close_at == std::string::npos) throw GenomicsDBConfigException("loader JSON is not an object");
      const std::string all_text = loader_text.substr(0, close_at) + ", \"query_column_ranges\": [[[" + std::to_string(part.first) + ", " + std::to_string(part.second) + "]]]" +
                                   loader_text.substr(close_at);
      try {
        CombineEngine eng(mini_json::parse(all_text), 0, nullptr, rank, "", false);
        eng.stage_cells(array_cells.data(), array_cells.size());
        eng.save_fragment(dir + "/fragment.gdbamd", true);
        struct stat fs;
        const long long zbytes = ::stat((dir + "/fragment.gdbamd").c_str(), &fs) == 0 ? (long long)fs.st_size : -1;
        std::cerr << "GENOMICSDB_TIMER,Rank," << rank << ",compress_tiledb_array,Wall-clock time(s)," << since(tc)
                  << ",cells_bytes," << array_cells.size() << ",fragment_bytes," << zbytes << "\n";
      } catch (const GenomicsDBDeviceException& e) {
        // (the columnar file is built from columns staged in HBM: without a device the array stays as cells.bin, which every reader accepts)
        std::cerr << out.tool << ": compress_tiledb_array skipped: " << e.what() << "\n";
      }
    }
  }
  if (loader.m_produce_combined_vcf) {
    // the loader JSON doubles as the query JSON of the in-line combine: every attribute, the whole column partition
    const auto tv = std::chrono::steady_clock::now();
    const size_t close = loader_text.rfind('}');
    if (close == std::string::npos) throw GenomicsDBConfigException("loader JSON is not an object");
    const std::string query_text = loader_text.substr(0, close) + ", \"query_column_ranges\": [[[" + std::to_string(part.first) + ", " + std::to_string(part.second) +
                                   "]]]" + loader_text.substr(close);
    const size_t capacity = (size_t)64u << 20;
    GenomicsDBBCFGenerator gen(query_text, cells.data(), cells.size(), capacity, false);
    std::vector<uint8_t> buf(capacity);
    size_t total = 0;
    while (!gen.end()) {
      const size_t n = gen.read_and_advance(buf.data(), 0, buf.size());
      if (n == 0) break;
      if (fwrite(buf.data(), 1, n, stdout) != n) throw GenomicsDBConfigException("short write of the combined VCF");
      total += n;
    }
    fflush(stdout);
    std::cerr << "GENOMICSDB_TIMER,Rank," << rank << ",produce_combined_vcf,Wall-clock time(s)," << since(tv) << ",bytes," << total << "\n";
  }
}

}  // namespace genomicsdb_amd
