// test_genomicsdb_importer - the reference example's driver of GenomicsDBImporter (example/src/test_genomicsdb_importer.cc:193-220):
//   test_genomicsdb_importer -l <loader.json> [-b <buffer_size = 20480>] [-n <num_streams>] [-r <rank>] <stream_to_filename.json>
// Every entry {"stream name": "file"} of the JSON becomes a buffer stream (the first num_streams of them with -n).  A file is read
// whole through zlib (plain, gzip or BGZF text; a plain .bcf as BCF2 records); its header goes to add_buffer_stream, and its records
// are written in pieces of whole lines (or whole BCF2 records) of at most buffer_size bytes - a larger record goes alone - whenever
// import_batch reports the stream exhausted.  A stream whose file is used up gets an empty write.  finish() makes the loader's outputs
// as vcf2tiledb does.  The device is GDBAMD_DEVICE, else LOCAL_RANK, else 0.
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../api/genomicsdb_importer.h"
#include "../common/gz_text.hpp"
#include "../common/mini_json.hpp"
#include "../kernels/gdb_import_stream.h"

using namespace genomicsdb_amd;

namespace {
struct FileStream {
  std::string name, data;
  bool is_bcf = false;
  size_t pos = 0;      // the next record
  // the next piece: whole records up to `room` bytes, at least one
  std::pair<const uint8_t*, size_t> next(size_t room) {
    const size_t begin = pos;
    while (pos < data.size()) {
      size_t end;
      if (is_bcf) {
        uint32_t l_shared = 0, l_indiv = 0;
        if (data.size() - pos < 8) throw std::runtime_error(name + ": truncated BCF2 record");
        memcpy(&l_shared, data.data() + pos, 4); memcpy(&l_indiv, data.data() + pos + 4, 4);
        end = pos + 8 + (size_t)l_shared + l_indiv;
        if (end > data.size()) throw std::runtime_error(name + ": truncated BCF2 record");
      } else {
        const void* nl = memchr(data.data() + pos, '\n', data.size() - pos);
        if (!nl) { data += '\n'; end = data.size(); } else end = (size_t)((const char*)nl - data.data()) + 1;
      }
      if (pos > begin && end - begin > room) break;
      pos = end;
    }
    return {(const uint8_t*)data.data() + begin, pos - begin};
  }
};
}  // namespace

int main(int argc, char** argv) {
  std::string loader_json;
  size_t buffer_size = 20480;
  long num_streams = -1;
  int rank = 0;
  int c;
  while ((c = getopt(argc, argv, "l:b:n:r:")) >= 0) {
    switch (c) {
      case 'l': loader_json = optarg; break;
      case 'b': buffer_size = strtoull(optarg, nullptr, 10); break;
      case 'n': num_streams = atol(optarg); break;
      case 'r': rank = atoi(optarg); break;
      default: std::cerr << "Unknown command line argument\n"; return -1;
    }
  }
  if (loader_json.empty() || optind + 1 > argc) {
    std::cerr << "Needs -l <loader.json> [-b <buffer_size>] [-n <num_streams>] [-r <rank>] <stream_to_filename.json>\n";
    return -1;
  }
  try {
    const mini_json::Value map = mini_json::parse_file(argv[optind]);
    if (!map.IsObject()) throw std::runtime_error("the stream-to-filename JSON must be a dictionary { stream name : file }");
    std::vector<FileStream> streams;
    GenomicsDBImporter importer(loader_json, rank);
    for (size_t i = 0; i < map.obj.size() && (num_streams < 0 || (long)i < num_streams); ++i) {
      FileStream s;
      s.name = map.obj[i].first;
      s.data = gz_text::read_all(map.obj[i].second.GetString());
      s.is_bcf = s.data.size() >= 9 && memcmp(s.data.data(), "BCF\2", 4) == 0;
      if (s.is_bcf) {
        uint32_t l_text = 0;
        memcpy(&l_text, s.data.data() + 5, 4);
        s.pos = 9 + (size_t)l_text;
        if (s.pos > s.data.size()) throw std::runtime_error(s.name + ": the BCF2 header is longer than the file");
      } else {      // the header: through the last leading '#' line
        while (s.pos < s.data.size() && s.data[s.pos] == '#') {
          const void* nl = memchr(s.data.data() + s.pos, '\n', s.data.size() - s.pos);
          s.pos = nl ? (size_t)((const char*)nl - s.data.data()) + 1 : s.data.size();
        }
      }
      importer.add_buffer_stream(s.name, s.is_bcf ? BCF_BUFFER_STREAM_TYPE : VCF_BUFFER_STREAM_TYPE, buffer_size, (const uint8_t*)s.data.data(), s.pos);
      streams.push_back(std::move(s));
    }
    importer.setup_loader();
    const std::vector<int64_t>& file_idx = importer.get_buffer_stream_idx_to_global_file_idx_vec();
    for (size_t i = 0; i < streams.size(); ++i) {
      if (file_idx[i] < 0) continue;
      const auto piece = streams[i].next(buffer_size);
      importer.write_data_to_buffer_stream((int64_t)i, 0, piece.first, piece.second);
    }
    uint64_t num_iterations = 0;
    while (!importer.is_done()) {
      importer.import_batch();
      for (const BufferStreamIdentifier& id : importer.get_exhausted_buffer_stream_identifiers()) {
        const auto piece = streams[(size_t)id.first].next(buffer_size);
        importer.write_data_to_buffer_stream(id.first, id.second, piece.first, piece.second);
      }
      ++num_iterations;
    }
    importer.finish();
    const StreamImportStats& st = importer.stats();
    std::cerr << "GENOMICSDB_TIMER,Rank," << rank << ",import_batches," << num_iterations << ",records," << st.num_records << ",cells," << st.num_cells << ",bytes," << st.num_bytes
              << ",max_pending_cells," << st.max_pending_cells << ",max_pending_bytes," << st.max_pending_bytes << ",deferred," << st.num_deferred_values << ",order_ms,"
              << st.ms_order << ",classify_ms," << st.ms_classify << ",sort_gather_ms," << st.ms_sort_gather << ",compact_ms," << st.ms_compact << ",h2d_s," << st.s_h2d
              << ",d2h_s," << st.s_d2h << "\n";
  } catch (const std::exception& e) {
    std::cerr << "test_genomicsdb_importer: " << e.what() << "\n";
    return -1;
  }
  return 0;
}
