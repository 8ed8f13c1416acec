// loader_outputs.h - what the loader does with the begin-cells of an import, shared by the vcf2tiledb tool and GenomicsDBImporter
// (reference: VCF2TileDBLoader's operators, tiledb_loader.cc:845-965):
//   "produce_tiledb_array": true  -> <workspace>/<array>/cells.bin; with "delete_and_create_tiledb_array": false and an array file
//                                    there, the cells are MERGED into it on the device (kernels/gdb_merge.hip) through a temporary
//                                    name in the same directory; "compress_tiledb_array": the columnar fragment file next to it
//   "produce_combined_vcf": true  -> combined in-line on the GPU and written to stdout
// The merge, the compressed fragment and the combine take the cells of the import WHOLE, in host memory; the windowed merge
// (LoaderOutputs::merge_windowed) reads the array it merges into from its file, window by window.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../common/mini_json.hpp"
#include "../host/variant_query_config.h"

namespace genomicsdb_amd {

struct LoaderOutputs {
  std::string loader_text;      // the loader JSON as text: it doubles as the query JSON of the in-line combine
  int rank = 0, device = 0;
  const char* tool = "";        // the program's name in messages
  // a file in the array's directory that already holds exactly the cells (an import that spooled its batches): renamed to cells.bin
  // instead of written.  Removed when the cells are merged into an existing array
  std::string spooled_cells_file;
  // vcf2tiledb --merge-window-bytes: a merge into an existing array goes window by window from cells.bin, read as a file, and the
  // batch in memory to the new cells.bin (merge_cell_files_device), with this many input bytes on the device (0: derived from its free
  // memory).  Without it the merge runs in-core and turns to the windowed path only when the in-core path refuses the sizes
  bool merge_windowed = false;
  uint64_t merge_window_bytes = 0;
};
// <workspace>/<array> of the rank, created when missing
std::string loader_array_directory(const GenomicsDBImportConfig& loader, int rank);
// true when the outputs that `doc` asks for need the cells in host memory (a merge, a compressed fragment, a combined VCF)
bool loader_outputs_need_cells(const mini_json::Value& doc, const GenomicsDBImportConfig& loader, int rank);
// cells: may be null only with a spooled file and !loader_outputs_need_cells.  Throws; after a throw cells.bin is unchanged
void produce_loader_outputs(const LoaderOutputs& out, const mini_json::Value& doc, const GenomicsDBImportConfig& loader, const std::vector<uint8_t>* cells);

}  // namespace genomicsdb_amd
