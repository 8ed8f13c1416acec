// gdb_columns.h - combined records as typed column tensors in HBM (host-visible interface, no HIP types).
//
// A page of BCF2 records that DevicePipeline::next_page() has left in its arena (output format "bu") is decoded on the device into
// typed columns: the site columns of every record, requested INFO fields as [R, W] and requested FORMAT fields as [R, N, W]
// (R records of the page, N samples of the query, W elements).  The page is read where it lies; nothing passes through text or the
// host.  Bodies: core/gdb_columns.hpp; kernels and their orchestration: gdb_columns.hip.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "gdb_pipeline.h"

namespace genomicsdb_amd {

enum RecordColumnDtype { RC_DEFAULT = 0, RC_INT8 = 1, RC_INT16 = 2, RC_INT32 = 3, RC_INT64 = 4, RC_FLOAT32 = 5, RC_UINT8 = 6 };

// name: "GT" or the id of a numeric FORMAT or INFO line of the engine's header (an id that is both - DP - means the FORMAT field;
// "INFO/DP" and "FORMAT/DP" say which).  dtype: RC_INT8 / RC_INT16 / RC_INT32 for an integer field (RC_DEFAULT: RC_INT32), RC_FLOAT32 or
// RC_DEFAULT for a float field.  width: W; 0 = the longest vector of the field in the page
struct ColumnRequest { std::string name; int dtype = RC_DEFAULT; int width = 0; };
struct RecordColumn { std::string name; int dtype = 0; int ndim = 0; int64_t shape[3] = {0, 0, 0}; void* dev_ptr = nullptr; };
struct ColumnsStats {
  int64_t records = 0;
  uint64_t bytes_read = 0;        // the shared blocks and the blocks of the requested FORMAT fields
  uint64_t bytes_written = 0;     // all columns
  float ms_measure = 0, ms_site = 0, ms_scatter = 0;      // hipEvent time: measure + scan of the allele lengths, site, scatter
  int32_t n_fields = 0;
  int32_t width[GDB_MAX_COLUMN_REQUESTS] = {0};        // W of every requested field, in request order
};

class RecordColumns {
 public:
  // validates the requests against the plan's header and refuses by name - before the device is touched - a string or Flag field, ID and
  // FILTER, a name the header does not have as FORMAT or INFO id, a dtype the field cannot have, an output format other than "bu" and the
  // htsjdk flag use_missing_values_only_not_vector_end (its pages hold no end-of-vector values: L could not be told from padding)
  RecordColumns(const HostPlan& hp, int device, const std::vector<ColumnRequest>& requests);
  ~RecordColumns();
  RecordColumns(const RecordColumns&) = delete;
  RecordColumns& operator=(const RecordColumns&) = delete;
  // the columns of `page`: contig, pos, end, column, qual, n_allele, alleles, alleles_off, then the requested fields in request order
  // (GT followed by GT_phase).  The buffers belong to this object and are overwritten by the next call.  A vector longer than a given
  // width and an integer outside the requested dtype throw, naming the field and the pos of the smallest offending record.
  const std::vector<RecordColumn>& decode(const DevicePipeline::PageView& page, ColumnsStats* stats);
  struct Impl;
 private:
  Impl* m_;
};

}  // namespace genomicsdb_amd
