// genomicsdb_importer.cc - see genomicsdb_importer.h
#include "genomicsdb_importer.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <unordered_set>

#include "../common/mini_json.hpp"
#include "../host/variant_query_config.h"
#include "../kernels/gdb_import_stream.h"
#include "loader_outputs.h"

namespace genomicsdb_amd {

namespace {
std::string loader_text_of(const std::string& path_or_json) {      // (a string that begins with '{' is the JSON itself)
  const size_t first = path_or_json.find_first_not_of(" \t\r\n");
  return first != std::string::npos && path_or_json[first] == '{' ? path_or_json : mini_json::read_text_file(path_or_json);
}
}  // namespace

std::string chromosome_intervals_for_column_partition(const std::string& loader_config_file, int rank) {
  const mini_json::Value doc = mini_json::parse(loader_text_of(loader_config_file));
  GenomicsDBImportConfig loader;
  loader.read_from_json(doc, rank);
  if (loader.m_vid_mapping_file.empty()) throw GenomicsDBConfigException("loader JSON needs vid_mapping_file");
  VidMapper vid;
  vid.parse_vid_json(mini_json::parse_file(loader.m_vid_mapping_file));
  const ColumnRange part = loader.get_column_partition(rank);
  std::vector<ContigInfo> contigs;
  for (unsigned i = 0; i < vid.get_num_contigs(); ++i) contigs.push_back(vid.get_contig_info(i));
  std::sort(contigs.begin(), contigs.end(), [](const ContigInfo& a, const ContigInfo& b) { return a.m_tiledb_column_offset < b.m_tiledb_column_offset; });
  std::string out = "{\"contigs\":[";
  bool any = false;
  for (const ContigInfo& c : contigs) {
    const int64_t off = c.m_tiledb_column_offset;
    int64_t begin;
    if (off <= part.first && part.first < off + c.m_length) begin = part.first - off + 1;      // the contig the partition begins in
    else if (off > part.first && off <= part.second) begin = 1;
    else continue;
    const int64_t end = off + c.m_length > part.second ? part.second - off + 1 : c.m_length;
    out += std::string(any ? "," : "") + "{\"" + c.m_name + "\":[" + std::to_string(begin) + "," + std::to_string(end) + "]}";
    any = true;
  }
  return out + "]}";
}

void import_files_of_loader(const std::string& loader_config_file, int rank, int device) {
  LoaderOutputs out;
  out.loader_text = loader_text_of(loader_config_file); out.rank = rank; out.tool = "GenomicsDBImporter";
  const mini_json::Value doc = mini_json::parse(out.loader_text);
  GenomicsDBImportConfig loader;
  loader.read_from_json(doc, rank);
  if (loader.m_vid_mapping_file.empty() || loader.m_callset_mapping_file.empty()) throw GenomicsDBConfigException("loader JSON needs vid_mapping_file and callset_mapping_file");
  VidMapper vid;
  vid.parse_vid_json(mini_json::parse_file(loader.m_vid_mapping_file));
  vid.parse_callsets_json(mini_json::parse_file(loader.m_callset_mapping_file));
  const ColumnRange part = loader.get_column_partition(rank);
  ImportOptions opt;
  opt.treat_deletions_as_intervals = loader.m_treat_deletions_as_intervals;
  opt.column_begin = part.first;
  opt.column_end = part.second;
  opt.row_begin = loader.m_lb_callset_row_idx;
  opt.row_end = loader.m_ub_callset_row_idx;
  if (device >= 0) out.device = device;
  else if (const char* e = getenv("GDBAMD_DEVICE")) out.device = atoi(e);
  else if (const char* e2 = getenv("LOCAL_RANK")) out.device = atoi(e2);
  const std::vector<uint8_t> cells = import_callsets_to_cells_device(vid, opt, out.device, 0);
  produce_loader_outputs(out, doc, loader, &cells);
}

struct GenomicsDBImporter::Impl {
  std::string loader_text;
  mini_json::Value doc;
  GenomicsDBImportConfig loader;
  int rank = 0, device = 0;
  bool is_loader_setup = false, finished = false;
  std::vector<BufferStreamDecl> decls;
  std::unordered_set<std::string> names;
  DeviceStreamImporter* dev = nullptr;
  std::vector<uint8_t> batch_cells, all_cells;
  std::vector<BufferStreamIdentifier> exhausted;
  bool produce_array = false, keep_cells = false;
  std::string spool_path;
  FILE* spool = nullptr;
  ~Impl() {
    delete dev;
    if (spool) fclose(spool);
    if (!spool_path.empty() && !finished) remove(spool_path.c_str());      // an import that did not finish leaves no file behind
  }
};

GenomicsDBImporter::GenomicsDBImporter(const std::string& loader_config_file, int rank, int device) : m_(new Impl) {
  try {
    m_->loader_text = loader_text_of(loader_config_file);
    m_->doc = mini_json::parse(m_->loader_text);
    m_->loader.read_from_json(m_->doc, rank);
    if (m_->loader.m_vid_mapping_file.empty()) throw GenomicsDBConfigException("loader JSON needs vid_mapping_file");
    m_->rank = rank;
    if (device >= 0) m_->device = device;
    else if (const char* e = getenv("GDBAMD_DEVICE")) m_->device = atoi(e);
    else if (const char* e2 = getenv("LOCAL_RANK")) m_->device = atoi(e2);
  } catch (...) { delete m_; m_ = nullptr; throw; }
}
GenomicsDBImporter::GenomicsDBImporter(GenomicsDBImporter&& other) : m_(other.m_) { other.m_ = nullptr; }
GenomicsDBImporter::~GenomicsDBImporter() { delete m_; }

void GenomicsDBImporter::add_buffer_stream(const std::string& name, VidFileTypeEnum type, size_t capacity, const uint8_t* init, size_t n) {
  if (m_->is_loader_setup) throw GenomicsDBImporterException("Cannot add buffer stream once setup_loader() has been called for a given GenomicsDBImporter object");
  if (m_->names.count(name)) throw GenomicsDBImporterException("Duplicate buffer stream name " + name);
  m_->names.insert(name);
  BufferStreamDecl d;
  d.name = name; d.is_bcf = type == BCF_BUFFER_STREAM_TYPE; d.capacity = capacity;
  if (init && n) d.init.assign(init, init + n);
  m_->decls.push_back(d);
}

void GenomicsDBImporter::setup_loader(const std::string& callsets_json) {
  if (m_->is_loader_setup) throw GenomicsDBImporterException("setup_loader() has already been called for this GenomicsDBImporter object");
  VidMapper vid;
  vid.parse_vid_json(mini_json::parse_file(m_->loader.m_vid_mapping_file));
  // the callsets of the string join those of the file (reference tiledb_loader.cc:502-505)
  if (!m_->loader.m_callset_mapping_file.empty()) vid.parse_callsets_json(mini_json::parse_file(m_->loader.m_callset_mapping_file));
  if (callsets_json.find_first_not_of(" \t\r\n") != std::string::npos) vid.parse_callsets_json(mini_json::parse(callsets_json));
  const ColumnRange part = m_->loader.get_column_partition(m_->rank);
  ImportOptions opt;
  opt.treat_deletions_as_intervals = m_->loader.m_treat_deletions_as_intervals;
  opt.column_begin = part.first;
  opt.column_end = part.second;
  opt.row_begin = m_->loader.m_lb_callset_row_idx;
  opt.row_end = m_->loader.m_ub_callset_row_idx;
  m_->dev = new DeviceStreamImporter(m_->device, vid, opt, m_->decls);
  m_->produce_array = m_->doc.HasMember("produce_tiledb_array") && m_->doc["produce_tiledb_array"].GetBool();
  m_->keep_cells = loader_outputs_need_cells(m_->doc, m_->loader, m_->rank);
  m_->is_loader_setup = true;
}

static void need_setup(bool is_setup, const char* what) {
  if (!is_setup) throw GenomicsDBImporterException(std::string("Cannot ") + what + " in the GenomicsDBImporter without calling setup_loader() first");
}
const std::vector<int64_t>& GenomicsDBImporter::get_buffer_stream_idx_to_global_file_idx_vec() const {
  need_setup(m_->is_loader_setup, "ask for the file indices of the buffer streams");
  return m_->dev->stream_file_idx();
}
size_t GenomicsDBImporter::get_max_num_buffer_stream_identifiers() const {
  need_setup(m_->is_loader_setup, "ask for the number of buffer stream identifiers");
  return m_->dev->num_used_streams();
}
void GenomicsDBImporter::write_data_to_buffer_stream(int64_t idx, unsigned partition_idx, const uint8_t* data, size_t n) {
  need_setup(m_->is_loader_setup, "write data to buffer stream");
  m_->dev->write(idx, partition_idx, data, n);
}

void GenomicsDBImporter::import_batch() {
  need_setup(m_->is_loader_setup, "import a batch");
  m_->dev->import_batch(m_->batch_cells);
  m_->exhausted.clear();
  for (const auto& e : m_->dev->exhausted()) m_->exhausted.emplace_back(e.first, (unsigned)e.second);
  if (m_->keep_cells) m_->all_cells.insert(m_->all_cells.end(), m_->batch_cells.begin(), m_->batch_cells.end());
  else if (m_->produce_array && !m_->batch_cells.empty()) {
    if (!m_->spool) {
      m_->spool_path = loader_array_directory(m_->loader, m_->rank) + "/cells.bin.import.tmp";
      m_->spool = fopen(m_->spool_path.c_str(), "wb");
      if (!m_->spool) throw GenomicsDBConfigException("cannot write " + m_->spool_path);
    }
    if (fwrite(m_->batch_cells.data(), 1, m_->batch_cells.size(), m_->spool) != m_->batch_cells.size()) throw GenomicsDBConfigException("short write to " + m_->spool_path);
  }
}
const std::vector<BufferStreamIdentifier>& GenomicsDBImporter::get_exhausted_buffer_stream_identifiers() const { return m_->exhausted; }
bool GenomicsDBImporter::is_done() const { return m_->is_loader_setup && m_->dev->is_done(); }
const std::vector<uint8_t>& GenomicsDBImporter::last_batch_cells() const { return m_->batch_cells; }
const StreamImportStats& GenomicsDBImporter::stats() const {
  need_setup(m_->is_loader_setup, "read the statistics");
  return m_->dev->stats();
}

void GenomicsDBImporter::finish() {
  need_setup(m_->is_loader_setup, "finish");
  if (m_->finished) throw GenomicsDBImporterException("finish() called twice");
  m_->dev->finish();
  if (m_->spool) {
    const bool ok = fclose(m_->spool) == 0;
    m_->spool = nullptr;
    if (!ok) throw GenomicsDBConfigException("cannot write " + m_->spool_path);
  }
  LoaderOutputs out;
  out.loader_text = m_->loader_text; out.rank = m_->rank; out.device = m_->device; out.tool = "GenomicsDBImporter";
  out.spooled_cells_file = m_->spool_path;
  // (an import without a cell and without a merge still writes an empty array file, as vcf2tiledb does)
  produce_loader_outputs(out, m_->doc, m_->loader, m_->keep_cells || m_->spool_path.empty() ? &m_->all_cells : nullptr);
  m_->finished = true;
}

}  // namespace genomicsdb_amd
