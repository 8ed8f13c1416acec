// vcf_index.h - .tbi / .csi next to a BGZF-compressed output file ("index_output_VCF": true).
//
// The reference asks htslib for it when its file-writing VCFAdapter closes (src/main/cpp/src/vcf/vcf_adapter.cc:275-295:
// tbx_index_build(file, 0, &tbx_conf_vcf) for "z", bcf_index_build(file, 14) for "b"); both htslib functions re-read the finished file.
// htslib is not in the tree (empty submodule): this is a restatement of the two published formats - the tabix index ("TBI\1", The Tabix
// index file format) and the coordinate-sorted index ("CSI\1", CSIv1) - with the UCSC binning scheme both use (min_shift 14, depth 5).
// Host code by nature (the reference's is, too): it walks the BGZF blocks of the file that was written, inflates them with zlib and notes, per
// record, contig, interval and the virtual offsets (block start << 16 | offset inside the block) in front of and behind it.
//
// The device builder (kernels/gdb_index.h) and its CPU harness find chunks and window minima per batch of lines and share the rest with
// build_tbi_index: TbiBatchMerger joins the batches, write_tbi_index fills the empty windows, lays the bytes out and compresses them.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace genomicsdb_amd {

namespace gdbidx { struct IdxChunk; }      // core/gdb_index.hpp

struct TbiChunk { uint64_t beg, end; };
struct TbiRef {
  std::map<uint32_t, std::vector<TbiChunk>> bins;
  std::map<uint32_t, uint64_t> loffset;        // CSI: virtual offset of the first record that overlaps the bin's first 16 kb window (fill_linear)
  std::vector<uint64_t> linear;                // 16 kb windows -> virtual offset of the first record overlapping the window
  uint64_t off_beg = ~0ull, off_end = 0, n_mapped = 0;
  uint32_t last_bin = ~0u;
};

// the serialising half of a .tbi builder: empty windows filled (fill_linear), the byte layout, BGZF; refs[i] belongs to names[i]
void write_tbi_index(const std::string& tbi_path, const std::vector<std::string>& names, std::vector<TbiRef>& refs);

// the serialising half of a .csi builder: refs grows to n_ref contigs (the count of ##contig lines of the BCF header), then as above
// with the CSIv1 layout (min_shift 14, depth 5, per-bin loffset derived from the linear index)
void write_csi_index(const std::string& csi_path, std::vector<TbiRef>& refs, int n_ref);

// the words of a refused record (IDX_ERR_* bits of core/gdb_index.hpp): they name the file and the 1-based line
std::string tbi_record_error(uint32_t bits, const std::string& path, int64_t line);

// What a batch of whole lines leaves, joined across batches: the result does not depend on where the batches were cut.
struct TbiBatchMerger {
  std::vector<std::string> names;
  std::map<std::string, int> name_id;
  std::vector<TbiRef> refs;
  // contig id of a run head's name: ids in order of first appearance, a name that comes back gets its old id
  uint32_t id_of(const std::string& chrom);
  // the batch's chunks, those of one (contig, bin) in file order.  A chunk with IDX_CHUNK_FIRST whose bin is the bin of the contig's
  // last record so far extends that bin's last chunk; the IDX_CHUNK_LAST chunks say what the next batch continues
  void add_chunks(const gdbidx::IdxChunk* chunks, size_t n);
  // window minima of contig tid, windows [0, n): ~0 = no record of the batch touches the window
  void add_windows(uint32_t tid, const uint64_t* minima, size_t n);
  // A batch may end where the virtual offset behind its last line is not known yet (the next member is not written): that one vend
  // is kPendingVoff, and resolve_pending names it before the next batch is added or the index is written
  static constexpr uint64_t kPendingVoff = ~(uint64_t)0;
  int pending_tid = -1; uint32_t pending_bin = 0;
  void resolve_pending(uint64_t voff);
  uint64_t num_bins() const;
  uint64_t num_chunks() const;
  uint64_t num_windows() const;
  void write(const std::string& tbi_path) { write_tbi_index(tbi_path, names, refs); }
};

// The pages of one BGZF output stream ("z": .tbi, "b": .csi), joined in stream order; what the device builder of the output's index
// (kernels/gdb_output_index.h) and its CPU harness share.  A page brings its chunks and window minima with PAGE-RELATIVE virtual offsets
// and with contigs named by their position among the header's ##contig IDs; here the page's file offset is added, text contigs get the
// .tbi's ids (first appearance), and the vend of a page's last record stays pending until the next page or write() says where it is.
struct OutputIndexMerger {
  // header_contigs: the IDs of the header's ##contig lines in order; header_bytes: compressed bytes in front of the first page (> 0)
  OutputIndexMerger(bool bcf, const std::vector<std::string>& header_contigs, uint64_t header_bytes);
  // chunks: those of one contig in file order, tid = header position; page_vend: the page-relative virtual offset behind the page (the
  // vend of its last record).  Contig k's minima are win[win_off[k] .. + extent[k]) (~0: no record).  compressed_bytes: the page's size in the file
  void add_page(gdbidx::IdxChunk* chunks, size_t n_chunks, uint64_t page_vend, const uint32_t* win_off, const uint32_t* extent, const uint64_t* win, uint64_t compressed_bytes);
  // the stream has ended: the 28-byte EOF block follows the last page
  void write(const std::string& path);
  uint32_t last_contig() const { return last_kid; }      // header position of the contig of the last record so far (~0u: none)
  bool bcf;
  std::vector<std::string> contigs;
  uint64_t file_base;
  uint32_t last_kid = ~0u;
  TbiBatchMerger merger;
};

// <path>.tbi for a bgzip'ed VCF (records indexed by CHROM, POS and INFO END= / the REF allele's length, as tabix does for its VCF preset)
void build_tbi_index(const std::string& vcf_gz_path);
// <path>.csi for a bgzip'ed BCF2 file (CHROM index, POS, rlen of the records; min_shift 14 like the reference's call)
void build_csi_index(const std::string& bcf_path);

}  // namespace genomicsdb_amd
