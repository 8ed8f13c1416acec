// hostsim_histogram - the bodies of the input histogram (csrc/core/gdb_histogram.hpp) on the CPU: a stand-alone program, built with the
// address and undefined-behaviour sanitizers, that the tests run as a subprocess (test infrastructure only).
//
//   hostsim_histogram hist <vid.json> <callsets.json> <file root, or -> <max_histogram_range> <num_bins> <column begin> <column end> <lb row> <ub row>
//       every input file with a callset inside the row bounds is read with the importer's own reader and header rule
//       (common/gz_text.hpp, host/import_common.hpp; BCF2 content: host/import_bcf.hpp), every line behind the header goes through
//       hist_line (every record through hist_bcf_record), and a counted one adds the file's weight to its bin.
//       Prints "stats files <f> records <r> counted <c>", then the reference's print (histogram_text of kernels/gdb_histogram.h).
//       A line error is described in the device path's words.
//   hostsim_histogram bin <max_histogram_range> <num_bins> <column begin> <column end> <column>
//       prints "size <size_of_bin>" and "bin <b> lo <lo> hi <hi>", "out" (outside the column bounds) or "range" (IMP_ERR_HIST_RANGE).
// A named error (an exception of the project's) prints "error: <what>" and ends with status 0: only a crash or a sanitizer report
// ends otherwise.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/common/gz_text.hpp"
#include "../../genomicsdb_amd/csrc/common/mini_json.hpp"
#include "../../genomicsdb_amd/csrc/core/gdb_histogram.hpp"
#include "../../genomicsdb_amd/csrc/host/import_bcf.hpp"
#include "../../genomicsdb_amd/csrc/host/import_common.hpp"
#include "../../genomicsdb_amd/csrc/kernels/gdb_histogram.h"

using namespace genomicsdb_amd;

static std::string range_words(const gdbhist::HistParams& P, const std::string& where) {
  return "a column outside the range of the histogram [0," + std::to_string(P.hi) + "] (" + where + ")";
}

static int hist_main(int argc, char** argv) {
  if (argc < 11) { std::cerr << "hist: 9 arguments needed\n"; return 2; }
  VidMapper vid;
  vid.parse_vid_json(mini_json::parse_file(argv[2]));
  vid.parse_callsets_json(mini_json::parse_file(argv[3]));
  ImportOptions opt;
  if (std::string(argv[4]) != "-") opt.file_root = argv[4];
  const int64_t max_range = strtoll(argv[5], nullptr, 10);
  const uint64_t num_bins = strtoull(argv[6], nullptr, 10);
  if (num_bins == 0) throw VCF2BinaryException("histogram: num_bins is 0");
  if (max_range < 0) throw VCF2BinaryException("histogram: max_histogram_range " + std::to_string(max_range) + " is negative");
  const gdbhist::HistParams P = gdbhist::hist_params((uint64_t)max_range, num_bins, strtoll(argv[7], nullptr, 10), strtoll(argv[8], nullptr, 10));
  opt.row_begin = strtoll(argv[9], nullptr, 10);
  opt.row_end = strtoll(argv[10], nullptr, 10);
  opt = with_clamped_row_bounds(opt, vid);
  const ImportTablesHost H = build_import_tables(vid, true);
  const std::vector<ImportFile> files = import_files(vid, opt);
  std::vector<uint64_t> counts((size_t)num_bins, 0);
  int64_t records = 0, counted = 0;
  auto add = [&](const gdbhist::HistSel& s, uint64_t weight) {
    records += s.record;
    if (s.counted) { ++counted; counts.at((size_t)s.bin) += weight; }
  };
  for (const ImportFile& file : files) {
    if (file.type != GDB_FILE_VCF) throw VCF2BinaryException(file.path + " is a CSV cell file: only (g)VCF text and BCF2 files are counted by this build");
    const uint64_t weight = file.callsets.size();
    const std::string text = gz_text::read_all(file.path);
    if (text.size() >= ((size_t)1 << 31)) throw VCF2BinaryException("2 GiB or more in " + file.path);
    if (is_bcf2(text.data(), text.size())) {
      const BcfHeaderHost hdr = parse_bcf_header(text.data(), text.size(), file, H);
      std::vector<uint64_t> offs;
      bcf_walk_records(text.data(), text.size(), hdr.records_begin, file.path, offs);
      const gdbimp::ImpBcfTables B = hdr.view();
      for (size_t r = 0; r + 1 < offs.size(); ++r) {
        const gdbhist::HistSel s = gdbhist::hist_bcf_record(B, P, (const uint8_t*)text.data(), (uint32_t)offs[r], (uint32_t)offs[r + 1]);
        if (s.err) {
          const std::string where = file.path + " record " + std::to_string(r + 1);
          if (s.err == gdbhist::IMP_ERR_HIST_RANGE) throw VCF2BinaryException(range_words(P, where));
          throw VCF2BinaryException(describe_bcf_error(first_import_error_bit(s.err), H, opt, hdr, (const uint8_t*)text.data(), (uint32_t)offs[r], (uint32_t)offs[r + 1], where));
        }
        add(s, weight);
      }
      continue;
    }
    const ImportHeader hdr = parse_import_header(text, file);
    const gdbimp::ImpTables T = H.view(opt, hdr.n_samples);
    int64_t line_no = hdr.lines_before;
    size_t pos = hdr.record_begin;
    while (pos < text.size()) {
      size_t eol = text.find('\n', pos);
      if (eol == std::string::npos) eol = text.size();
      ++line_no;
      const ImpHostLine hl(text.data(), (uint32_t)pos, (uint32_t)eol);
      const gdbhist::HistSel s = gdbhist::hist_line(T, P, hl.line);
      if (s.err) {
        const std::string where = file.path + " line " + std::to_string(line_no);
        if (s.err == gdbhist::IMP_ERR_HIST_RANGE) throw VCF2BinaryException(range_words(P, where));
        std::string words;
        try { words = describe_line_error(first_import_error_bit(s.err), H, opt, hdr, text.data(), (uint32_t)pos, (uint32_t)eol, where); }
        catch (const VCF2BinaryException& e) {      // the host parser's own words for a POS / END it refuses too: the line is added, as the device path does
          words = e.what();
          if (words.compare(0, 22, "VCF2BinaryException : ") == 0) words = words.substr(22);
          words += " (" + where + ")";
        }
        throw VCF2BinaryException(words);
      }
      add(s, weight);
      pos = eol + 1;
    }
  }
  std::cout << "stats files " << files.size() << " records " << records << " counted " << counted << "\n";
  std::cout << histogram_text(counts.data(), counts.size(), (uint64_t)max_range);
  return 0;
}

static int bin_main(int argc, char** argv) {
  if (argc < 7) { std::cerr << "bin: 5 arguments needed\n"; return 2; }
  const uint64_t num_bins = strtoull(argv[3], nullptr, 10);
  if (num_bins == 0) throw VCF2BinaryException("histogram: num_bins is 0");
  const gdbhist::HistParams P = gdbhist::hist_params(strtoull(argv[2], nullptr, 10), num_bins, strtoll(argv[4], nullptr, 10), strtoll(argv[5], nullptr, 10));
  const gdbhist::HistSel s = gdbhist::hist_column(P, strtoll(argv[6], nullptr, 10));
  std::cout << "size " << P.size_of_bin << "\n";
  if (s.err) std::cout << "range\n";
  else if (!s.counted) std::cout << "out\n";
  else std::cout << "bin " << s.bin << " lo " << gdbhist::hist_bin_lo(P, s.bin) << " hi " << gdbhist::hist_bin_hi(P, s.bin) << "\n";
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  try {
    if (mode == "hist") return hist_main(argc, argv);
    if (mode == "bin") return bin_main(argc, argv);
  } catch (const std::exception& e) {
    std::cout << "error: " << e.what() << "\n";
    return 0;
  }
  std::cerr << "usage: hostsim_histogram hist|bin ..\n";
  return 2;
}
