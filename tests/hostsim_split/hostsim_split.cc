// hostsim_split - the bodies of the device splitter (csrc/core/gdb_split.hpp) on the CPU: a stand-alone program, built with the address
// and undefined-behaviour sanitizers, that the tests run as a subprocess (test infrastructure only).
//
//   hostsim_split split <vid.json> <callsets.json> <file root, or -> <out dir> <begins, comma separated> <ends, comma separated> [more VCF files ..]
//       every input (the "filename"s of the callset mapping, then the extra files) is read with the importer's own reader and header
//       rule (common/gz_text.hpp, host/import_common.hpp), every line behind the header classified with split_classify, and the text
//       of input i for partition p - the '#' lines, then the selected lines with their newlines - written to <out dir>/f<i>_p<p>.txt.
//       Prints "file <i> <name>" per input.  A line error is described in the device path's words.
//   hostsim_split paths <callsets.json> <original> <results dir, or -> <partition>
//       prints VidMapper::get_split_file_path.
// A named error (an exception of the project's) prints "error: <what>" and ends with status 0, like a split: only a crash or a
// sanitizer report ends otherwise.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/common/gz_text.hpp"
#include "../../genomicsdb_amd/csrc/common/mini_json.hpp"
#include "../../genomicsdb_amd/csrc/core/gdb_split.hpp"
#include "../../genomicsdb_amd/csrc/host/import_common.hpp"

using namespace genomicsdb_amd;

static std::vector<int64_t> numbers(const std::string& s) {
  std::vector<int64_t> v;
  size_t b = 0;
  for (size_t i = 0; i <= s.size(); ++i)
    if (i == s.size() || s[i] == ',') { if (i > b) v.push_back(strtoll(s.substr(b, i - b).c_str(), nullptr, 10)); b = i + 1; }
  return v;
}

static int split_main(int argc, char** argv) {
  if (argc < 8) { std::cerr << "split: 6 arguments needed\n"; return 2; }
  VidMapper vid;
  vid.parse_vid_json(mini_json::parse_file(argv[2]));
  vid.parse_callsets_json(mini_json::parse_file(argv[3]));
  ImportOptions opt;
  if (std::string(argv[4]) != "-") opt.file_root = argv[4];
  const std::string out_dir = argv[5];
  const std::vector<int64_t> begins = numbers(argv[6]), ends = numbers(argv[7]);
  if (begins.empty() || begins.size() != ends.size() || begins.size() > gdbsplit::kMaxPartitions) throw VCF2BinaryException("split: begins and ends do not match");
  const gdbsplit::SplitParts P{begins.data(), ends.data(), (uint32_t)begins.size()};
  const ImportTablesHost H = build_import_tables(vid, true);
  std::vector<ImportFile> files = import_files(vid, opt);
  for (int i = 8; i < argc; ++i) { ImportFile f; f.name = argv[i]; f.path = argv[i]; files.push_back(f); }
  for (size_t fi = 0; fi < files.size(); ++fi) {
    const ImportFile& file = files[fi];
    const std::string text = gz_text::read_all(file.path);
    if (text.size() >= ((size_t)1 << 31)) throw VCF2BinaryException("2 GiB or more of text in " + file.path);
    const ImportHeader hdr = parse_import_header(text, file);
    const gdbimp::ImpTables T = H.view(opt, hdr.n_samples);
    std::vector<std::string> out(P.n);
    // the '#' lines in front of the first record (an empty line is no line of the output)
    size_t pos = 0;
    while (pos < hdr.record_begin) {
      size_t eol = text.find('\n', pos);
      if (eol == std::string::npos) eol = text.size();
      size_t ln = eol - pos;
      if (ln && text[pos + ln - 1] == '\r') --ln;
      if (ln) for (std::string& o : out) { o.append(text, pos, eol - pos); o.push_back('\n'); }
      pos = eol + 1;
    }
    int64_t line_no = hdr.lines_before;
    pos = hdr.record_begin;
    while (pos < text.size()) {
      size_t eol = text.find('\n', pos);
      if (eol == std::string::npos) eol = text.size();
      ++line_no;
      const ImpHostLine hl(text.data(), (uint32_t)pos, (uint32_t)eol);
      const gdbsplit::SplitSel s = gdbsplit::split_classify(T, P, hl.line);
      if (s.err) {
        const std::string where = file.path + " line " + std::to_string(line_no);
        std::string words;
        try { words = describe_line_error(first_import_error_bit(s.err), H, opt, hdr, text.data(), (uint32_t)pos, (uint32_t)eol, where); }
        catch (const VCF2BinaryException& e) {      // the host parser's own words for a POS / END it refuses too: the line is added, as the device path does
          words = e.what();
          if (words.compare(0, 22, "VCF2BinaryException : ") == 0) words = words.substr(22);
          words += " (" + where + ")";
        }
        throw VCF2BinaryException(words);
      }
      for (uint32_t p = 0; p < P.n; ++p)
        if (gdbsplit::split_selected(s, p)) { out[p].append(text, pos, eol - pos); out[p].push_back('\n'); }
      pos = eol + 1;
    }
    for (uint32_t p = 0; p < P.n; ++p) {
      const std::string path = out_dir + "/f" + std::to_string(fi) + "_p" + std::to_string(p) + ".txt";
      FILE* f = fopen(path.c_str(), "wb");
      if (!f || fwrite(out[p].data(), 1, out[p].size(), f) != out[p].size()) { if (f) fclose(f); throw VCF2BinaryException("cannot write " + path); }
      fclose(f);
    }
    std::cout << "file " << fi << " " << file.name << "\n";
  }
  return 0;
}

static int paths_main(int argc, char** argv) {
  if (argc < 6) { std::cerr << "paths: 4 arguments needed\n"; return 2; }
  VidMapper vid;
  vid.parse_callsets_json(mini_json::parse_file(argv[2]));
  const std::string dir = std::string(argv[4]) == "-" ? "" : argv[4];
  std::cout << vid.get_split_file_path(argv[3], dir, atoi(argv[5])) << "\n";
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  try {
    if (mode == "split") return split_main(argc, argv);
    if (mode == "paths") return paths_main(argc, argv);
  } catch (const std::exception& e) {
    std::cout << "error: " << e.what() << "\n";
    return 0;
  }
  std::cerr << "usage: hostsim_split split|paths ..\n";
  return 2;
}
