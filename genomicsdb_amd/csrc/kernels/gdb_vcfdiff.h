// gdb_vcfdiff.h - vcfdiff on the device: two VCF files (text: plain, gzip or BGZF) compared record by record, allele order, the order of
// INFO keys, FORMAT keys and sample columns and float noise below a threshold aside (host-visible interface, no HIP types).  The
// semantic differ of the reference (tools/src/vcfdiff.cc, tools/include/vcfdiff.h); the rule is written out in DESIGN.md ("Comparing
// two VCFs") with its deliberate differences.
//
// The files, windows, batch cuts, BGZF inflate and newline / tab index are the device importer's own (the text tap of DeviceImporter,
// kernels/gdb_import.h).  Per file and batch:
//   k_vdiff_keys     one thread per line -> contig, pos, end, the ref-block and long-REF flags and error bits (core/gdb_vcfdiff.hpp);
//                    the batch's text and tab index are copied device-to-device and stay resident
// the keys go to the host, which checks them and walks both files (serial, O(records)): pairs and events.  Then over the pairs:
//   k_vdiff_compare  one workgroup per pair: the site part once (ID, allele map in LDS, QUAL, FILTER, INFO, the FORMAT key match), then
//                    one lane per gold sample on the light path (identity map or at most 3 alleles); masks by wave reduction
//   k_vdiff_heavy    the other pairs: one wavefront per sample finds the commas of both vectors with __ballot and a prefix popcount
//                    into LDS, then the lanes compare element k against element m(k) in parallel
// Float tokens outside the device parser's exact range come back as a deferred list that the host decides by the same rule.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace genomicsdb_amd {

struct VcfDiffStats {
  int64_t gold_records = 0, test_records = 0;      // record lines kept (inside the regions)
  int64_t pairs_compared = 0, pairs_light = 0, pairs_heavy = 0;
  int64_t deferred = 0;                            // float tokens pairs the host decided
  int64_t events = 0;                              // events listed in the report
  int64_t num_batches = 0;
  uint64_t resident_bytes = 0;                     // text and tab index kept on the device
  float ms_index = 0, ms_inflate = 0, ms_keys = 0, ms_compare = 0;      // HIP-event time per phase, summed
  double s_read = 0, s_walk = 0, s_total = 0;      // wall clock: file read (+ host inflate), the host's walk, all
};

struct VcfDiffRequest {
  std::string gold, test;
  double threshold = 1e-5;                         // -t (vcfdiff.cc:29)
  std::string regions;                             // -r: chr | chr:pos | chr:from-to | chr:from- , comma separated
  int device = 0; uint64_t text_budget_bytes = 0;  // as for DeviceImporter
};

struct VcfDiffEvent {
  int kind = 0;                                    // 0 COMPARED, 1 REF_BLOCKS_OVERLAP, 2 DIFFERENT_POSITIONS, 3 EXTRA_LINES
  int64_t gold_line = 0, test_line = 0;            // 1-based, 0: none
  std::string gold_text, test_text;                // the lines as they stand in the files
  bool compared = false;
  uint32_t flags = 0;                              // 1 ID, 2 ALLELES, 4 QUAL, 8 FILTER
  uint64_t info[4] = {0, 0, 0, 0}, fmt[4] = {0, 0, 0, 0};      // MISSING_IN_TEST, ADDED_IN_TEST, TYPE_DIFFERS, DIFFERS over info_names / fmt_names
};
struct VcfDiffReport {
  int64_t compared = 0;
  std::vector<VcfDiffEvent> events;                // in order; a COMPARED pair is listed only when a bit is set
  std::vector<std::string> info_names, fmt_names;  // the union of both headers: gold's order, then the names only test has
  std::string json;                                // the same as one JSON document
};

// Refused before any launch (VCFDiffException): BCF2 input, differing or duplicate sample names, more than 64 distinct INFO or FORMAT
// names.  A line error names "<path> line <n>", 1-based.  Text that does not fit in the device's free memory is refused with the sizes.
// No device: GenomicsDBDeviceException, there is no CPU path.
VcfDiffReport vcfdiff_device(const VcfDiffRequest& req, VcfDiffStats* stats = nullptr);

}  // namespace genomicsdb_amd
