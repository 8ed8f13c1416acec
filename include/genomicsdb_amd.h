/* genomicsdb_amd.h - C ABI of the MI355X variant-combine engine (libgenomicsdb_amd.so).
 *
 * Drop-in boundary for the scan/combine hot path of Intel-HLS/GenomicsDB v0.10.2.  Plain pointers and sizes only.
 * Every function returns an error through gdb_mi355_last_error() (thread-local) instead of throwing across the ABI.
 * There is NO CPU fallback: without a HIP device every engine entry point fails.
 *
 * (1) Query stream - the six entry points the reference exports over JNI
 *     (reference src/main/jni/src/genomicsdb_GenomicsDBQueryStream.cc:29-111, header
 *      src/main/jni/include/genomicsdb_GenomicsDBQueryStream.h:17-58), each a thin shim over GenomicsDBBCFGenerator
 *     (reference src/main/cpp/include/vcf/genomicsdb_bcf_generator.h:33-93).  A JNI stub forwards 1:1.
 * (2) Engine - explicit staging / per-interval execution with the output left in HBM, for callers that own device
 *     memory (bench, multi-GPU drivers).  Replaces the VariantQueryProcessor::scan_and_operate +
 *     BroadCombinedGVCFOperator pair (reference src/main/cpp/include/genomicsdb/query_variants.h:241-243,
 *     include/query_operations/broad_combined_gvcf.h:59-61).
 */
#ifndef GENOMICSDB_AMD_H
#define GENOMICSDB_AMD_H
#include <stddef.h>
#include <stdint.h>

/* ---- limits of this build that the reference does not have ------------------------------------------------------------
 * The reference's per-record tables resize (include/utils/lut.h:65-343); the device's are fixed (core/gdb_types.h, the
 * values below mirror it and tests/test_capi_cpu.py checks that they agree).  A query that needs more is refused when its
 * plan is built (GenomicsDBException naming the limit) or, for data-dependent limits, ends with an error that spells the
 * limit out ("device error bits ...") - never with truncated output. */
#define GDBAMD_MAX_QUERIED_FIELDS 48        /* attributes of one query (plan time) */
#define GDBAMD_MAX_INFO_FIELDS 24           /* ... of which INFO */
#define GDBAMD_MAX_FORMAT_FIELDS 24         /* ... of which FORMAT */
#define GDBAMD_MAX_MERGED_ALLELES 128       /* alleles of one output record, REF and <NON_REF> included (data) */
#define GDBAMD_MAX_INPUT_ALLELES 64         /* alleles of one input cell, REF included (data) */
#define GDBAMD_MAX_PLOIDY 8                 /* general-ploidy genotype enumeration for G-length fields (data) */
#define GDBAMD_MAX_INFO_VECTOR 64           /* elements of an element_wise_sum INFO vector (data) */
#define GDBAMD_MAX_ID_TOKENS 16             /* distinct ';'-separated ID tokens united in one record (data) */
#define GDBAMD_MAX_FILTER_IDS 16            /* distinct FILTER ids united in one record (data) */
#define GDBAMD_MAX_HISTOGRAM_FIELDS 8       /* (bins, counts) INFO fields reduced with histogram_sum (plan time) */
#define GDBAMD_MAX_PIPELINES_PER_PROCESS 256 /* device pipelines alive in one process: one per query stream / engine, two for an engine that streams an array through HBM
                                              * in windows with overlapped staging (each owns a 3.5 KB element of a __constant__ array - 0.9 MB of device memory read
                                              * with scalar loads; handles do not serialise on it) */

#ifdef __cplusplus
extern "C" {
#endif

const char* gdb_mi355_last_error(void);
int gdb_mi355_device_count(void);

/* ---- (1) query stream ------------------------------------------------------------------------------------ */
/* jniGenomicsDBInit: returns a handle or NULL.  chr == "" keeps the intervals of the query JSON; otherwise the
 * interval is contig offset + start-1 .. end-1 (1-based, inclusive).  is_bcf != 0: uncompressed BCF2 ("bu": "BCF\2\2" header,
 * typed records - what GATK4's BCF2Codec reads; vcf_adapter.cc:475-509), with the two htsjdk switches of the JNI
 * (use_missing_values_only_not_vector_end, keep_idx_fields_in_bcf_header); text VCF otherwise.  buffer_capacity is what
 * get_num_bytes_available reports (the reference's RWBuffer size); it does not size the device pages. */
void* gdb_mi355_init(const char* loader_json_file, const char* query_json_file, const char* chr, int start, int end, int rank,
                     uint64_t buffer_capacity, uint64_t segment_size, int is_bcf, int produce_header_only,
                     int use_missing_values_only_not_vector_end, int keep_idx_fields_in_bcf_header);
/* same stream, configuration and cells handed over in memory (tests, embedding) */
void* gdb_mi355_init_from_memory(const char* query_json_text, const uint8_t* cells, uint64_t cells_nbytes, uint64_t buffer_capacity,
                                 int produce_header_only);
void* gdb_mi355_init_from_memory_format(const char* query_json_text, const uint8_t* cells, uint64_t cells_nbytes, uint64_t buffer_capacity,
                                        int produce_header_only, int is_bcf, int use_missing_values_only_not_vector_end, int keep_idx_fields_in_bcf_header);
/* The same two with the reference's vcf_output_format string instead of the JNI's is_bcf flag: "" VCF text, "bu" BCF2, and the
 * BGZF-compressed flavours "z" (VCF text) / "b" (BCF2) that its VCFAdapter writes through htslib (vcf_adapter.cc:340-372,
 * genomicsdb_config_base.cc:34,156-165).  "z" / "b": header = one BGZF block (host), body = BGZF blocks of 8 192 input bytes (GDBAMD_BGZF_BLOCK = 4096 / 6144 / 8192 / 16384)
 * deflated ON THE DEVICE (only compressed bytes cross PCIe), then the 28-byte EOF block.  The compressed bytes are this build's
 * own; the inflated stream equals the "" / "bu" stream. */
void* gdb_mi355_init_output_format(const char* loader_json_file, const char* query_json_file, const char* chr, int start, int end, int rank,
                                   uint64_t buffer_capacity, uint64_t segment_size, const char* output_format, int produce_header_only,
                                   int use_missing_values_only_not_vector_end, int keep_idx_fields_in_bcf_header);
void* gdb_mi355_init_from_memory_output_format(const char* query_json_text, const uint8_t* cells, uint64_t cells_nbytes, uint64_t buffer_capacity,
                                               int produce_header_only, const char* output_format, int use_missing_values_only_not_vector_end,
                                               int keep_idx_fields_in_bcf_header);
uint64_t gdb_mi355_close(void* handle);                         /* jniGenomicsDBClose */
uint64_t gdb_mi355_get_num_bytes_available(void* handle);       /* jniGenomicsDBGetNumBytesAvailable: buffer capacity */
int gdb_mi355_read_next_byte(void* handle);                     /* jniGenomicsDBReadNextByte: byte or -1 */
int64_t gdb_mi355_read(void* handle, uint8_t* dst, uint64_t offset, uint64_t n); /* jniGenomicsDBRead: bytes copied, -1 on error */
int64_t gdb_mi355_skip(void* handle, uint64_t n);               /* jniGenomicsDBSkip */
/* The unread bytes of the current batch where they lie (a pinned ring buffer), without copying: *ptr / *n are valid until the
 * next call on this handle; consume them with gdb_mi355_skip.  1 = bytes available, 0 = end of the stream, -1 = error.
 * (reference: GenomicsDBBCFGenerator::get_read_batch, include/vcf/genomicsdb_bcf_generator.h:60-63, which the JNI read loop uses) */
int gdb_mi355_peek(void* handle, const uint8_t** ptr, uint64_t* n);
/* How the stream was drained so far (not part of the reference's surface; bench / diagnostics).  The device assembles pages
 * of GDBAMD_DEVICE_PAGE_MB (default 2048) MiB alternately into two HBM arenas - independently of buffer_capacity - and drains them
 * through a ring of pinned host buffers (GDBAMD_RING_SLOTS x GDBAMD_RING_SLOT_MB, default 4 x 64 MiB) on a copy stream while the
 * next page is assembled; gdb_mi355_read is served from the ring. */
typedef struct gdb_mi355_stream_stats {
  uint64_t pages, chunks, bytes;                 /* device pages produced, ring chunks copied, body bytes copied to the host */
  double seconds_waiting_for_copies;             /* time read() spent blocked on a copy that had not landed yet */
  double seconds_producing;                      /* host time inside the sweep / sizing / page launches (reader blocked) */
} gdb_mi355_stream_stats;
int gdb_mi355_get_stream_stats(void* handle, gdb_mi355_stream_stats* out);
/* The index of a "z" / "b" stream's bytes as a file - .tbi / .csi -, built ON THE DEVICE from every page while it is in HBM
 * (kernels/gdb_output_index.h): the file gdbamd_build_output_index writes for the finished file, byte for byte, without re-reading it.
 * gdb_mi355_enable_index: only for the output formats "z" / "b", and only before the first body page is produced (before the header
 * has been read to its end).  gdb_mi355_write_index: only once the stream has been read to its end; writes `path` (the caller's
 * choice: <file>.tbi / <file>.csi) and fills *stats (may be NULL).  0, or -1 with gdb_mi355_last_error() saying which condition
 * failed; the stream stays usable as it was. */
typedef struct gdb_mi355_index_stats {
  int64_t pages, records;                        /* device pages indexed, records in them */
  int64_t contigs, bins, chunks, linear_windows; /* of the index as written (bins without the meta bin) */
  int64_t atomics;                               /* atomicMin issued on the window minima */
  double ms_records, ms_voff, ms_chunks, ms_linear; /* device time per phase, summed over the pages */
  double s_write;                                /* wall clock: merge of the pages, layout, compression, file write */
  uint64_t table_bytes;                          /* device memory held by the record tables */
} gdb_mi355_index_stats;
int gdb_mi355_enable_index(void* handle);
int gdb_mi355_write_index(void* handle, const char* path, gdb_mi355_index_stats* stats);

/* ---- (2) engine ------------------------------------------------------------------------------------------ */
typedef struct gdbamd_interval_stats {
  int64_t num_cells, num_cells_in_window, num_records, num_heavy_incidences;
  uint64_t bytes_out, bytes_in_reference_cells;
  int32_t pages, write_launches;
  uint32_t err_bits;
  float ms_sweep, ms_site, ms_size, ms_write, ms_total, ms_write_kernel_avg;
  int32_t num_record_types, resolved_entry_bytes;   /* entry text table: distinct record types, slots, pool bytes; bytes per (record, sample) of the
                                                      * resolved matrix: 8 (offset + length), 5 (compact: no entry longer than 255 bytes), 0 (no matrix) */
  int64_t num_text_slots, text_pool_bytes;
  uint64_t num_remap_elements;           /* sum over re-indexed records of (calls with PL) x (merged genotypes): the PL remap work */
  uint64_t bytes_compressed;             /* output formats "z" / "b": bytes of the pages after BGZF compression (bytes_out: before) */
  float ms_compress;                     /* device time of the compression kernels */
  int32_t page_kernel;                   /* which kernels the interval ran, as the decimal digits S K W C II of its most recent page launch (0: no page was
                                          * launched).  S = sizing kernel of the interval: 0 k_assemble_size, 1 k_assemble_size3<8>, 2 k_assemble_size3<16>,
                                          * 3 k_size2, 4 k_assemble_size_ev.  K = page kernel: 1 k_assemble_write, 2 k_write2, 3 k_write3, 4 k_assemble_write_ev,
                                          * 5 the BCF2 kernels.  W = wavefronts per workgroup, C = 16-byte words per lane in flight in the cooperative copy
                                          * (0: the kernel has no such parameter), II = LDS image in KiB.  The default text path reads 111204. */
  /* the six counters of the reference's GTProfileStats (src/main/cpp/include/genomicsdb/query_variants.h:67-124, -DDO_PROFILING),
   * indexed by the enum below; counted per interval on the device.  The reference counts cell VISITS of its iterators; here every
   * cell is touched once per interval, so: NUM_CELLS = cells of the staged window considered for the interval, IN_LEFT_SWEEP =
   * cells that begin before the interval and are still live at its first column (what gt_get_column has to find),
   * VALID_CELLS_IN_QUERY = cells that contribute to at least one record, ATTR_CELLS_ACCESSED = those x queried attributes,
   * PQ_FLUSHES_DUE_TO_OVERLAPPING_CELLS = cells cut short by the next cell of their own sample, OPERATOR_INVOCATIONS = records */
  uint64_t gt_profile_stats[6];
  int32_t huge_records;                  /* records with so many variant calls (more than 256; more than 24 when the interval averages 24 and more per
                                          * record) that one workgroup each did their call walk (k_site_huge); 0 when that kernel was not launched */
  int32_t huge_fallbacks;                /* ... of which the kernel handed back to the one-thread walk: two alleles with one 32-bit hash, a full allele
                                          * table, several different FILTER ids */
  /* which code took the interval's medians (`median` reducer of INFO fields and QUAL) */
  int32_t sorted_median_fields;          /* median fields ordered by the device-wide sort (the interval averages more than 16 variant calls per record, or
                                          * GDBAMD_SORTED_MEDIAN is set); 0: that path was not taken */
  int32_t big_median_records;            /* records with 49 .. 4096 variant calls whose medians one workgroup each took (k_big_medians): at most 4096 are
                                          * listed per interval; 0 when the medians were sorted or the interval has no median field */
  int32_t big_median_unlisted;           /* ... further such records that found the list full: their medians come from the site kernels */
} gdbamd_interval_stats;
enum { GDBAMD_GT_NUM_CELLS = 0, GDBAMD_GT_NUM_CELLS_IN_LEFT_SWEEP, GDBAMD_GT_NUM_VALID_CELLS_IN_QUERY, GDBAMD_GT_NUM_ATTR_CELLS_ACCESSED,
       GDBAMD_GT_NUM_PQ_FLUSHES_DUE_TO_OVERLAPPING_CELLS, GDBAMD_GT_NUM_OPERATOR_INVOCATIONS, GDBAMD_GT_NUM_STATS };

/* one attribute column in device memory; off == NULL for fixed-length attributes */
typedef struct gdbamd_device_column { const void* data; const uint32_t* off; } gdbamd_device_column;

void* gdbamd_engine_create(const char* query_json_text, int device);          /* NULL on error */
void* gdbamd_engine_create_format(const char* query_json_text, int device, int is_bcf, int use_missing_values_only_not_vector_end);  /* pages hold BCF2 records */
void* gdbamd_engine_create_output_format(const char* query_json_text, int device, const char* output_format, int use_missing_values_only_not_vector_end);  /* "", "bu", "z", "b": with "z" / "b" the pages hold BGZF blocks (no header, no EOF block) */
/* n host bytes as BGZF blocks (no EOF block), compressed by the device kernels; gdbamd_bgzf_bound(n) bytes of dst always suffice */
int gdbamd_bgzf_compress(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_len, float* ms_kernels);
/* the same with the kernel chosen: vcf_text != 0 = the anchored kernel the "z" stream uses for its pages of VCF text (matches begin at tabs /
 * newlines; any bytes give a valid stream), 0 = the byte-level kernel ("b", and what gdbamd_bgzf_compress runs) */
int gdbamd_bgzf_compress_mode(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_len, float* ms_kernels, int vcf_text);
uint64_t gdbamd_bgzf_bound(uint64_t n);
/* the counterpart: a whole BGZF buffer (a chain of members from its first byte to its last, the EOF member included or not) inflated on GPU
 * `device` by the kernel the device importer uses, one wavefront per member; stream, ISIZE and CRC32 of every member are verified there.
 * *dst_len = the inflated size; dst NULL: only that (no device needed).  0 on success; a bad member is an error that names its byte offset. */
int gdbamd_bgzf_decompress(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_len, float* ms_kernels, int device);
void gdbamd_engine_destroy(void* engine);
int gdbamd_engine_num_fields(void* engine);                                     /* plan fields = staged attribute columns */
const char* gdbamd_engine_field_name(void* engine, int f);                      /* array attribute name of plan field f */
int gdbamd_engine_field_info(void* engine, int f, int* elem_type, int* is_var, int* fixed_num);
uint64_t gdbamd_engine_header(void* engine, char* dst, uint64_t cap);           /* VCF header text; returns its length */
/* stage begin-cells given in the reference binary-cell layout (host memory, column-major order) */
int gdbamd_engine_stage_cells(void* engine, const uint8_t* cells, uint64_t nbytes);
/* the same in parts (successive calls continue the column-major order); _end() makes one contiguous fragment in HBM */
int gdbamd_engine_stage_cells_begin(void* engine);
int gdbamd_engine_stage_cells_append(void* engine, const uint8_t* cells, uint64_t nbytes);
int gdbamd_engine_stage_cells_end(void* engine);
/* adopt a columnar fragment that already lives in HBM: row = QUERY row idx, begin/end = columns, cols[num_fields] */
int gdbamd_engine_adopt_device_fragment(void* engine, int64_t ncells, const int32_t* row, const int64_t* begin, const int64_t* end,
                                        const gdbamd_device_column* cols, int ncols, uint64_t reference_cell_bytes);
/* Last column of the first piece of [column_begin, column_end] that can be run on its own with byte-identical output: the cut
 * sits right before a cell begin >= column_begin + max_columns (the reference's sweep closes its interval at every cell
 * begin, query_variants.cc:478-505).  *piece_end = column_end when the interval is narrow enough or no cell begins in between. */
int gdbamd_engine_split_point(void* engine, int64_t column_begin, int64_t column_end, int64_t max_columns, int64_t* piece_end);
/* ColumnHistogramOperator (src/main/cpp/src/query_operations/variant_operations.cc:732-767; gt_mpi_gather --produce-histogram, tools/src/gt_mpi_gather.cc:404-411):
 * the staged begin-cells counted on the device by the bin of their begin column.  nbins must be (hist_end - hist_begin) / bin_size + 1; a cell beginning at or
 * before hist_begin counts for bin 0, one at or behind hist_end for the last bin.  accumulate != 0 adds to what counts holds (arrays streamed in windows). */
int gdbamd_engine_column_histogram(void* engine, uint64_t hist_begin, uint64_t hist_end, uint64_t bin_size, uint64_t* counts, uint64_t nbins, int accumulate);
/* VariantCallPrintOperator (src/main/cpp/src/query_operations/variant_operations.cc:803-843; gt_mpi_gather --print-calls, tools/src/gt_mpi_gather.cc:369-383):
 * the cells of the query's column intervals as the reference's JSON document - per interval first the intervals that began in front of it and
 * intersect its begin, then the cells that begin inside (SingleCellTileDBIterator, src/main/cpp/src/genomicsdb/genomicsdb_iterators.cc:181-510); selected and
 * formatted on the device, one thread per cell.  Call with dst == NULL for the length, then with a buffer of at least that size.  -1: error. */
int64_t gdbamd_engine_print_calls(void* engine, char* dst, uint64_t cap);
/* The other two SingleCellOperatorBase printers over the same cells, same calling convention.  mode 0: --print-calls; 1: --print-csv
 * (VariantCallPrintCSVOperator, variant_operations.cc:845-903: "row,begin,end,<fields>" per cell); 2: --print-AC (AlleleCountOperator, :905-1089:
 * "column REF ALT count" per normalised ALT allele named by a genotype, per query interval in the order of column, REF, ALT).  The reference's tests
 * hold no golden for modes 1 and 2: parity is against the oracle's restatement only. */
int64_t gdbamd_engine_print_cells(void* engine, int mode, char* dst, uint64_t cap);
/* The variants query - what the reference's gt_mpi_gather prints without a mode flag and GenomicsDB::query_variants users get
 * (VariantQueryProcessor::gt_get_column_interval, src/main/cpp/src/genomicsdb/query_variants.cc:687-843; print_variants' default format, variant.cc:983-999):
 * per query interval the calls that cover its begin and the cells that begin inside, grouped into variants by (begin, end, REF, set of ALT), GT and the
 * allele-length fields of a variant with several calls rewritten in merged allele order (GA4GHOperator).  Selected, grouped and formatted on the device.
 * Same calling convention as gdbamd_engine_print_cells.  -1: error. */
int64_t gdbamd_engine_query_variants(void* engine, char* dst, uint64_t cap);
/* "index_output_VCF" (src/main/cpp/src/config/json_config.cc:648, src/main/cpp/src/vcf/vcf_adapter.cc:275-295): the index htslib builds from a finished BGZF
 * file - <path>.tbi for a bgzip'ed VCF (tbx_index_build with the VCF preset), <path>.csi with min_shift 14 for a BGZF BCF2 file (bcf_index_build(.., 14)).
 * The file-writing VCFAdapter and gt_mpi_gather call it when the query JSON says "index_output_VCF": true and the format is "z" / "b". */
int gdbamd_build_output_index(const char* path, int is_bcf);
/* ColumnHistogramOperator::equi_partition_and_print_bins (variant_operations.cc:769-796): the text the reference prints - "Total T #bins P count/bins X.X", one
 * "first_column,last_column,count" line per partition of about equal cell count, an empty line.  Returns the text's length (dst may be NULL), -1 when
 * num_parts >= nbins.  The lines are what column_partitions of a loader JSON should be for P ranks of equal load. */
int64_t gdbamd_equi_partition_text(const uint64_t* counts, uint64_t nbins, uint64_t hist_begin, uint64_t bin_size, uint64_t num_parts, char* dst, uint64_t cap);
/* the staged fragment as a columnar file, and back: file -> HBM copies without parsing.  gdb_mi355_init opens
 * <workspace>/<array>/fragment.gdbamd when present (else cells.bin).  This is the build's own format (the
 * Intel TileDB fork's on-disk format of the reference, variant_storage_manager.cc:61-153, is not available). */
int gdbamd_engine_save_fragment(void* engine, const char* path);
/* the same file with every data section cut into 8 KiB tiles, each a raw DEFLATE stream (stored / fixed-Huffman blocks): compressed
 * bytes cross PCIe and are inflated on the device (fixed and dynamic Huffman codes), one thread per tile (the place of the gzip'd attribute tiles of the reference's
 * TileDB arrays, genomicsdb_iterators.cc:334-423).  Tiles carry no checksum: a tile whose stream is malformed or does not inflate to the
 * tile's size is refused at load (the error names the section, the tile and the reason); damage that leaves a valid stream of the
 * same size is NOT detected ("Compressed fragment files"). */
int gdbamd_engine_save_fragment_compressed(void* engine, const char* path);
/* diagnostic and test hook of that tile inflater: ntiles independent raw DEFLATE streams, concatenated without padding (stream t =
 * bytes [in_off[t], in_off[t + 1]) of src, in_off[0] = 0), through the kernel and launch shape the fragment reader uses on GPU `device`.
 * want[t] <= 8192 = the size tile t must inflate to.  out: ntiles * 8192 bytes, every slot prefilled with `fill` before the launch;
 * status[t]: 0 = inflated to exactly want[t] bytes, else why not (1 block type, 2 code, 3 no end-of-block, 4 symbol, 5 distance,
 * 6 more output than want, 7 input exhausted, 8 LEN / NLEN, 9 fewer bytes than want).  0 on success (refused tiles are no error). */
int gdbamd_inflate_tiles(const uint8_t* src, const uint64_t* in_off, const uint32_t* want, uint64_t ntiles, uint8_t fill, uint8_t* out, uint8_t* status, int device);
int gdbamd_engine_load_fragment(void* engine, const char* path);
/* Arrays larger than the staging budget (GDBAMD_STAGE_BUDGET_MB, default 8192 MiB of cells per window): instead of staging by
 * hand, name a source and let the engine pass it through HBM in column windows, carrying the intervals that are still live at a
 * window's end into the next one on the device (the analogue of the reference's segment-at-a-time array iterator and
 * VariantQueryProcessorScanState: variant_storage_manager.cc:61-153, query_variants.h:126-191).
 *   open_array:         <dir>/fragment.gdbamd when it is valid for this query (checked against the array schema, the vid /
 *                       callset mapping and the cells.bin it was made from), else <dir>/cells.bin
 *   open_memory_cells:  begin-cells in host memory (the caller keeps them alive until the engine is destroyed)
 *   open_cell_callback: cells produced on demand; fn hands out the next chunk of whole begin columns (valid until the next call)
 *                       and returns 1, or returns 0 when there are no more; one pass, front to back
 * cover(column) stages windows until `column` is covered and returns the range [*lo, *hi] of query positions the staged
 * fragment serves: run intervals inside it, then ask again with *hi + 1. */
typedef int (*gdbamd_cell_chunk_fn)(void* user, const uint8_t** cells, uint64_t* nbytes);
int gdbamd_engine_open_array(void* engine, const char* dir);
int gdbamd_engine_open_memory_cells(void* engine, const uint8_t* cells, uint64_t nbytes);
int gdbamd_engine_open_cell_callback(void* engine, gdbamd_cell_chunk_fn fn, void* user);
/* Page-lock a range of the caller's own host memory (the cells handed to open_memory_cells / stage_cells_append, a chunk buffer of
 * a cell callback) so that the engine's host -> HBM copies are DMA transfers that overlap the kernels of the window being
 * computed; copies from pageable memory go through the runtime's bounce buffers on the calling thread and hold up the other
 * pipeline's launches.  The range stays valid and pinned until gdbamd_unpin_host_memory; 0 on success (on failure the memory is
 * left as it was: the copies still work, only slower). */
int gdbamd_pin_host_memory(const void* p, uint64_t nbytes);
int gdbamd_unpin_host_memory(const void* p);
int gdbamd_engine_cover(void* engine, int64_t column, int64_t* lo, int64_t* hi);
/* what is staged: #begin-cells and the sum of their reference binary-cell sizes ("bytes_in" of the byte accounting) */
int gdbamd_engine_staged_info(void* engine, int64_t* ncells, uint64_t* reference_cell_bytes);
/* reference bases for TileDB columns [begin, begin+len) (host pointer) */
int gdbamd_engine_set_reference(void* engine, int64_t begin, const char* bases, uint64_t len);
/* scan + combine one column interval.  The VCF body is produced page by page in HBM (arena_bytes per page); when
 * host_out != NULL the pages are copied there (at most host_cap bytes, *host_len = total body bytes). */
int gdbamd_engine_run_interval(void* engine, int64_t column_begin, int64_t column_end, uint64_t arena_bytes, char* host_out,
                               uint64_t host_cap, uint64_t* host_len, gdbamd_interval_stats* stats);

/* n query intervals of the staged fragment, up to `lanes` (1 .. 4) of them in flight at a time: lane l takes intervals l, l + lanes, ... on a
 * device pipeline of its own (own stream, entry table, matrix and page arenas) that works on the SAME staged fragment - the latency-bound
 * sweep / site / sizing kernels of one interval overlap with the store-bound page kernel of another.  The pages stay in HBM (each lane's
 * last page is valid until the lane's next interval) unless host_out != NULL: then interval i's body is copied to host_out[i] (at most
 * host_cap[i] bytes; host_len[i] = its length either way).  stats[i] belongs to interval i.  lanes = 1 is a loop of gdbamd_engine_run_interval.
 * (The reference scans a partition with one thread: tools/src/gt_mpi_gather.cc:322-366; this is the device's way to keep two batches of
 * the same partition in flight.) */
int gdbamd_engine_run_intervals(void* engine, int n, const int64_t* column_begins, const int64_t* column_ends, uint64_t arena_bytes, int lanes,
                                gdbamd_interval_stats* stats, char* const* host_out, const uint64_t* host_cap, uint64_t* host_len);

/* HBM a NEW lane pipeline takes for intervals of `interval_columns` positions at the query's sample count (~45 bytes of page and ~18 bytes
 * of tables per sample and position, the page capped by arena_bytes, + 2 GiB).  gdbamd_engine_run_intervals creates no more new lanes than
 * the device's free memory holds (4 GiB kept spare) and reports the clamp on stderr; lane pipelines stay allocated (grow-only) until
 * gdbamd_engine_release_lanes or the engine's destruction. */
int gdbamd_engine_lane_footprint(void* engine, int64_t interval_columns, uint64_t arena_bytes, uint64_t* bytes);
int gdbamd_engine_release_lanes(void* engine);

/* the same in two steps, for consumers that take the pages where they are (HBM): prepare = sweep, site and sizing passes of
 * the interval; next_page = the next <= arena_bytes of whole records.  *dev_ptr is device memory, valid until the next call
 * on this engine.  next_page returns 1 (a page), 0 (interval exhausted) or -1 (error).
 * (reference: the RWBuffer hand-over of GenomicsDBBCFGenerator::produce_next_batch, src/main/cpp/src/vcf/genomicsdb_bcf_generator.cc:96-125) */
int gdbamd_engine_prepare_interval(void* engine, int64_t column_begin, int64_t column_end);
int gdbamd_engine_next_page(void* engine, uint64_t arena_bytes, const void** dev_ptr, uint64_t* nbytes);

/* ---- the page as typed columns in HBM ---------------------------------------------------------------------
 * For consumers on the GPU (a genotype matrix, a filter, a model): the page gdbamd_engine_next_page has just returned, decoded on the device
 * into typed arrays that never pass through text or the host.  The engine's output format must be "bu": the decoder reads the BCF2 records
 * where they lie (BCFv2.2 layout: typed descriptors, int8 / int16 / int32 / float / char vectors, one block per FORMAT field).
 * With R = records of the page and N = samples of the query, every page gives
 *   contig int32[R] (the BCF rid), pos int64[R] (1-based), end int64[R] (pos + rlen - 1), column int64[R] (TileDB column of pos),
 *   qual float32[R] (bit pattern kept; missing = 0x7F800001), n_allele int32[R], alleles uint8[total] with alleles_off int64[R + 1]
 *   (REF and the ALTs of record r joined by ',' are alleles[alleles_off[r] .. alleles_off[r + 1]))
 * and per requested field, in request order: a FORMAT field as [R, N, W], an INFO field as [R, W]; "GT" as the allele indices (-1: missing)
 * followed by GT_phase uint8[R, N, W] (the phase bit of every element; 0 where it is missing or behind the end).
 * Sentinels are BCF's own for the column's dtype: missing -128 / -32768 / INT32_MIN / 0x7F800001, end-of-vector the next value up.  Elements
 * behind a vector's end up to W are end-of-vector; a field that a record does not have is [missing, end-of-vector, ...] for every sample.
 * Nothing is truncated or wrapped: a vector longer than a given width, and an integer outside the dtype (htslib's bounds: int8 holds
 * -120 .. 127, int16 -32760 .. 32767), are errors that name the field and the pos of the smallest offending record. */
enum { GDBAMD_DTYPE_DEFAULT = 0, GDBAMD_DTYPE_INT8 = 1, GDBAMD_DTYPE_INT16 = 2, GDBAMD_DTYPE_INT32 = 3, GDBAMD_DTYPE_INT64 = 4, GDBAMD_DTYPE_FLOAT32 = 5, GDBAMD_DTYPE_UINT8 = 6 };
#define GDBAMD_MAX_COLUMN_REQUESTS 32
/* name: "GT" or the id of an Integer or Float FORMAT or INFO line of the engine's header; an id that is both (DP) means the FORMAT field,
 * "INFO/DP" and "FORMAT/DP" say which.  dtype: INT8 / INT16 / INT32 for integers (DEFAULT: INT32), FLOAT32 or DEFAULT for floats.
 * width: W; 0 = the longest vector of the field in the page (at least 1) */
typedef struct gdbamd_column_request { const char* name; int32_t dtype; int32_t width; } gdbamd_column_request;
/* name: owned by the engine, valid as long as dev_ptr */
typedef struct gdbamd_column { const char* name; int32_t dtype; int32_t ndim; int64_t shape[3]; void* dev_ptr; } gdbamd_column;
typedef struct gdbamd_columns_stats {
  int64_t records;
  uint64_t bytes_read;                   /* what the decoder read of the page: the shared blocks and the blocks of the requested FORMAT fields */
  uint64_t bytes_written;                /* all columns */
  float ms_measure, ms_site, ms_scatter; /* hipEvent time of the per-record walk + the scan of the allele lengths, the site columns, the field columns */
  int32_t n_fields;
  int32_t width[GDBAMD_MAX_COLUMN_REQUESTS];   /* W of every requested field, in request order */
} gdbamd_columns_stats;
/* Chooses the fields (n may be 0: the site columns alone).  Refused by name, before anything is launched: a string or Flag field, ID and
 * FILTER, a name that is neither a FORMAT nor an INFO id of the header, a dtype the field cannot have, an engine whose output format is not
 * "bu" or that was created with use_missing_values_only_not_vector_end.  0, or -1 with gdb_mi355_last_error(). */
int gdbamd_engine_columns_select(void* engine, const gdbamd_column_request* requests, int n);
/* Decodes the page last returned by gdbamd_engine_next_page.  out_columns[0 .. min(cap, *n)) are filled, *n is their number (8 + one per
 * field + one for GT_phase).  The columns lie in buffers the engine owns and grows on demand (checked against the free device memory first;
 * refused with the sizes when they do not fit); they are valid until the next page is asked for (a buffer that has to grow is freed first: the pointers of the page before are gone then, also within
 * one interval).  Any other call on the engine after gdbamd_engine_next_page - staging, run_interval, the lanes, the printers - takes the page away.  Without a page, or before
 * gdbamd_engine_columns_select: an error.  0, or -1. */
int gdbamd_engine_page_columns(void* engine, gdbamd_column* out_columns, int cap, int* n, gdbamd_columns_stats* stats);

/* ---- (3) host-only helpers (no device needed) ----------------------------------------------------------- */
/* column partition of `rank` as the loader JSON defines it: begin from "column_partitions"[rank], end = next sorted begin - 1
 * (reference: GenomicsDBImportConfig::get_column_partition, src/main/cpp/src/config/json_config.cc:340-417) */
int gdbamd_column_partition(const char* loader_json_text, int rank, int64_t* begin, int64_t* end);

/* (g)VCF import: the files of the callset mapping -> begin-cells (reference binary cell layout, column-major) whose begin
 * column lies in [column_begin, column_end]; what vcf2tiledb's conversion step produces for one column partition
 * (reference: VCF2Binary::convert_VCF_to_binary_for_callset, src/main/cpp/src/vcf/vcf2binary.cc:991-1196, fields :715-989;
 * hand-over order of VCF2TileDBLoader, src/main/cpp/src/loader/tiledb_loader.cc:845-965).  file_root prefixes relative
 * "filename" entries (NULL / "": as they are).  *cells is malloc'ed: release with gdbamd_free.  0 on success. */
int gdbamd_import_cells(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int treat_deletions_as_intervals,
                        int64_t column_begin, int64_t column_end, uint8_t** cells, uint64_t* nbytes, int64_t* ncells);
/* The same import with the conversion on GPU `device` (kernels/gdb_import.hip): byte for byte the cells of gdbamd_import_cells.
 * The host reads the files; the device inflates BGZF input (see below), indexes, measures, writes, sorts and gathers.  text_budget_bytes: record text
 * per batch (0: default).  Numeric tokens outside the device's exact fast path are parsed by the host importer's functions
 * (stats slot 5 counts them).  Refused with an error that names the field: 2-dimensional (allele-specific) fields and flattened
 * tuple elements - gdbamd_import_cells serves those vids.  stats: NULL or GDBAMD_IMPORT_NUM_STATS doubles:
 *   0 files, 1 records, 2 cells, 3 spanning cells, 4 bytes, 5 deferred values, 6 batches, 7 text bytes,
 *   8..11 HIP-event ms of index / measure / write / sort + gather, 12..16 wall seconds of file read, H2D, deferred parse, D2H, total */
#define GDBAMD_IMPORT_NUM_STATS 17
int gdbamd_import_cells_device(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int treat_deletions_as_intervals,
                               int64_t column_begin, int64_t column_end, uint8_t** cells, uint64_t* nbytes, int64_t* ncells, int device, uint64_t text_budget_bytes,
                               double* stats);
/* The same with the inflate mode chosen and more statistics.  A BGZF file - gzip members with the "BC" subfield from the first byte to the last,
 * what bgzip and htslib write - crosses the link compressed: the host inflates only the members that hold the '#' lines, the device the rest
 * (kernels/gdb_inflate.hip), in windows of about text_budget_bytes, and verifies stream, ISIZE and CRC32 of every member; a member that fails
 * refuses the file with an error that names the file and the member's byte offset.  inflate_mode: 0 auto (BGZF on the device, every other file
 * through zlib on the host), 1 always on the host, 2 a file that is not BGZF is an error.  gdbamd_import_cells_device is this call with mode 0.
 * stats: NULL or nstats doubles; slots 0..16 as above, then 17 bytes of the input files as stored, 18 BGZF members inflated on the device,
 * 19 files inflated whole on the host, 20 HIP-event ms of the inflate kernel, 21 input bytes uploaded (text, or compressed members).
 * Batches never cross a window, so slot 6 (batches) can be larger than with inflate on the host for the same budget; the cells are the same. */
#define GDBAMD_IMPORT_NUM_STATS_EX 22
int gdbamd_import_cells_device_ex(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int treat_deletions_as_intervals,
                                  int64_t column_begin, int64_t column_end, uint8_t** cells, uint64_t* nbytes, int64_t* ncells, int device, uint64_t text_budget_bytes,
                                  int inflate_mode, double* stats, int nstats);
/* BCF2 input.  The device calls above sniff every file's content, not its name: input whose (inflated) bytes begin with 'BCF\2\1' or 'BCF\2\2'
 * is BCF2 - plain (bcftools -Ou, an htsjdk BCF stream) or BGZF / gzip (the usual .bcf) - and gives the cells of the same records written as VCF
 * text; one callset mapping may mix VCF and BCF2 files.  Compressed BCF2 is inflated on the host (inflate_mode 2 refuses it with an error that
 * says so); nothing of a BCF2 file is deferred, and stats slot 7 counts its record bytes.  The host walks the record chain and names file,
 * 1-based record number and byte offset of a broken one; the device refuses, with file and record number, an unknown type code, a vector that
 * runs past its block, a dictionary or contig id outside the header's range and an n_sample other than the header's.  Float or char values for
 * an integer attribute of the vid are an error that names the field; integers for a float attribute are converted.
 * gdbamd_import_cells (the host importer) refuses a BCF2 file by name.
 *
 * Buffer streams (the reference's jniAddBufferStream / VCFBufferReader): a callset whose "filename" equals names[i] is read from the nbytes[i]
 * bytes at data[i] instead of a file - VCF text or BCF2, plain or gzip, sniffed like a file's content.  A name that no callset uses is an
 * error; a callset without a stream is read from its file as before.  nstreams 0 is gdbamd_import_cells_device_ex. */
int gdbamd_import_cells_device_streams(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int treat_deletions_as_intervals,
                                       int64_t column_begin, int64_t column_end, uint8_t** cells, uint64_t* nbytes, int64_t* ncells, int device,
                                       uint64_t text_budget_bytes, int inflate_mode, double* stats, int nstats, int nstreams, const char* const* names,
                                       const void* const* data, const uint64_t* stream_nbytes);
/* Incremental import (the loader JSON's "lb_callset_row_idx" / "ub_callset_row_idx", src/main/cpp/src/loader/tiledb_loader.cc:107-139): the two imports
 * above for the callsets whose row_idx lies in [lb, ub] only - clamped as the reference clamps them (negative -> 0, swapped when reversed, ub capped at the
 * mapping's largest row; genomicsdb_config_base.cc:167-180).  A file or stream without a callset in bounds is not opened and not counted (*nfiles, stats
 * slot 0); of a multi-sample file only the samples in bounds give cells, and a sum-like INFO value is still divided by the number of samples in the file's
 * header, so a file split across batches gives the cells of the file imported at once.  lb 0 and ub INT64_MAX - 1 are the calls above. */
int gdbamd_import_cells_rows(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int treat_deletions_as_intervals,
                             int64_t column_begin, int64_t column_end, uint8_t** cells, uint64_t* nbytes, int64_t* ncells, int64_t lb_callset_row_idx,
                             int64_t ub_callset_row_idx, int64_t* nfiles);
int gdbamd_import_cells_device_rows(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int treat_deletions_as_intervals,
                                    int64_t column_begin, int64_t column_end, uint8_t** cells, uint64_t* nbytes, int64_t* ncells, int device,
                                    uint64_t text_budget_bytes, int inflate_mode, double* stats, int nstats, int nstreams, const char* const* names,
                                    const void* const* data, const uint64_t* stream_nbytes, int64_t lb_callset_row_idx, int64_t ub_callset_row_idx);
/* The other half of an incremental import: nstreams >= 1 streams of begin-cells in host memory, each in column-major (column, row) order as the imports above
 * or a cells.bin give them, merged into one stream in that order on GPU `device` (kernels/gdb_merge.hip) - what the reference reaches with a new fragment
 * and consolidate_tiledb_array.  Only the 24-byte header [row i64][col i64][cell_size u64] of a cell is read; payloads move as opaque bytes.  Errors (-1, no
 * result): a size chain that runs past its stream's end (stream index and byte offset), a stream that is not sorted (stream and cell index), a negative row,
 * a row that two streams share (the smallest).  Equal keys inside one stream keep their order.  Streams, keys and result must fit in device memory together.
 * *cells is malloc'ed: release with gdbamd_free.  stats: NULL or nstats doubles:
 *   0 streams, 1 cells in, 2 cells out, 3 bytes out, 4 output cells per workgroup of the rank kernel (its tile),
 *   5..8 HIP-event ms of keys + checks / rank / size scan / gather, 9..11 wall seconds of H2D, D2H, total */
#define GDBAMD_MERGE_NUM_STATS 12
int gdbamd_merge_cells(int nstreams, const void* const* data, const uint64_t* nbytes, uint8_t** cells, uint64_t* out_nbytes, int64_t* ncells, int device,
                       double* stats, int nstats);
/* The same merge from files to a file, for arrays larger than device memory: source i is the file paths[i], read with pread, or, when paths[i] is NULL, the
 * nbytes[i] bytes at data[i] (paths or data may be NULL as a whole when no source is of that kind).  The sources are merged round by round through pinned
 * staging and device pools bounded by window_bytes - the input cell bytes resident on the device, carried and fresh, over all sources; 0: derived from the
 * free device memory - with the transfers overlapped with the kernels; a round that can emit nothing (a cell, or a run of one key, larger than a source's
 * share of the window) doubles that share.  The result, byte for byte what gdbamd_merge_cells gives, goes to <output_path>.merge.tmp and is renamed to
 * output_path on success; after an error neither is left.  The refusals are those of gdbamd_merge_cells with cell indices and byte offsets counted from the
 * start of the source; the shared row named is the smallest one known in the round that first finds one.  Device memory: about 8.7 x window_bytes plus
 * nsources x largest row / 8 bytes, whatever the sources' lengths.  Returns the number of cells, -1: error.  stats: NULL or nstats doubles:
 *   0..11 as gdbamd_merge_cells (HIP-event ms summed over the rounds; 9, 10 stay 0), 12 rounds, 13 cells carried (summed over the rounds), 14 growths of a
 *   share, 15 window bytes as used, 16 peak device bytes, 17 pinned host bytes, 18..20 wall seconds of the host thread reading, writing, waiting for the device */
#define GDBAMD_MERGE_FILES_NUM_STATS 21
int64_t gdbamd_merge_cell_files(int nsources, const char* const* paths, const void* const* data, const uint64_t* nbytes, const char* output_path, int device,
                                uint64_t window_bytes, double* stats, int nstats);
/* vcf2tiledb --split-files on GPU `device` (kernels/gdb_split.hip; reference tools/src/vcf2tiledb.cc:118-151): every (g)VCF text file of the callset
 * mapping - plain, gzip or BGZF; then the nextra paths of extra_paths - is cut into one BGZF file + <file>.tbi per column partition, in one pass per file.
 * Partition p is [begins[p], ends[p]] (the loader JSON's column_partitions with derived ends; they must not overlap, at most 4096).  A partition's file holds
 * every '#' line and, in file order and verbatim, every record line whose interval overlaps the partition: [col, tend], col = contig offset + POS - 1,
 * tend = contig offset + END - 1 with INFO END (the last END counts), else col + len(REF) - 1.  A line that spans partitions goes to each; a partition
 * without records still gets the header, the EOF block and an index.  produce: the one partition index to write, or -1 for all.  An output is
 * <results_directory, or the input's directory>/partition_<p>_<the input's basename> unless the callset mapping's "split_files_paths" names it;
 * single_output_name (NULL / "": none) names the output of exactly one input and one partition.  Errors that name file and 1-based line: a contig that is
 * not in the vid, POS / END that is no plain integer, fewer than 8 columns; BCF2 and CSV inputs are refused by name before anything runs.  After an error
 * no output of the failing input exists.  text_budget_bytes and inflate_mode as for gdbamd_import_cells_device_ex.
 * *outputs (may be NULL) receives one line "original filename \t partition \t path \n" per file written, malloc'ed: release with gdbamd_free.
 * stats: NULL or nstats doubles:
 *   0 files, 1 record lines, 2 record lines written (summed over the partitions), 3 text bytes in, 4 text bytes out, 5 compressed bytes out, 6 batches,
 *   7..10 HIP-event ms of index / classify / scan + gather / deflate, 11..15 wall seconds of file read, H2D, D2H + write, .tbi build, total,
 *   16 HIP-event ms of the BGZF inflate kernel */
#define GDBAMD_SPLIT_NUM_STATS 17
int gdbamd_split_files_device(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int npartitions, const int64_t* begins,
                              const int64_t* ends, int produce, const char* results_directory, const char* single_output_name, int device,
                              uint64_t text_budget_bytes, int inflate_mode, int nextra, const char* const* extra_paths, double* stats, int nstats, char** outputs);
/* The same with the outputs' .tbi built on the device (index_on_device != 0; kernels/gdb_index.hip): each output is indexed while it is written, from its
 * packed text that is still in device memory, the sizes of the blocks the deflate just made and the header member written on the host; the finished file is
 * not read again.  The files are those of index_on_device == 0, byte for byte.  stats as above (11..15: .tbi build is the wall clock of index building on
 * either path) plus 17 HIP-event ms of the index kernels (0 with the host builder). */
#define GDBAMD_SPLIT_INDEX_NUM_STATS 18
int gdbamd_split_files_device_index(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int npartitions, const int64_t* begins,
                                    const int64_t* ends, int produce, const char* results_directory, const char* single_output_name, int device,
                                    uint64_t text_budget_bytes, int inflate_mode, int nextra, const char* const* extra_paths, double* stats, int nstats, char** outputs,
                                    int index_on_device);
/* <path>.tbi of a bgzipped VCF, built on GPU `device` (kernels/gdb_index.hip): the file gdbamd_build_output_index(path, 0) writes, byte for byte.  The file
 * crosses the link compressed and is inflated on the device in batches of whole lines of about text_budget_bytes (0: 64 MiB); per batch the device finds the
 * record lines, their intervals, bins, virtual offsets, chunks and the minima of the 16 kb windows, the host joins the batches, lays the index out and
 * compresses it.  Written through a temporary name: after an error no .tbi exists.  Refused: a file that is not a BGZF chain from its first byte to its last
 * (with the byte offset where the chain breaks), a member with a bad stream, ISIZE or CRC32, a record with POS < 1 or POS / END >= 2^31 (file and 1-based
 * line).  stats may be NULL. */
typedef struct gdbamd_index_stats {
  int64_t members, batches, lines, records;     /* BGZF members; batches; lines; record lines */
  int64_t contigs, bins, chunks, linear_windows; /* of the index as written (bins without the meta bin) */
  uint64_t text_bytes;                          /* inflated bytes */
  int64_t atomics;                              /* atomic minima issued on the windows (one per run of records that share a window inside a wavefront) */
  double ms_inflate, ms_index, ms_records, ms_chunks, ms_linear;  /* HIP-event ms of inflate, line index, select + records, sorts + chunks, windows */
  double s_read, s_serialize_write, s_total;    /* wall seconds of file read, merge + layout + compress + write, the whole call */
} gdbamd_index_stats;
int gdbamd_index_vcf_device(const char* path, int device, uint64_t text_budget_bytes, gdbamd_index_stats* stats);
/* vcf_histogram on GPU `device` (kernels/gdb_histogram.hip; reference tools/src/vcf_histogram.cc, tiledb_loader.cc:428-456, utils/histogram.cc): one pass
 * over every input file of the callset mapping - (g)VCF text, plain, gzip or BGZF, and BCF2; a file whose name is one of the nstreams `names` is read from
 * memory - counts its records per bin of a uniform histogram over the columns [0, max_histogram_range]:
 *   size_of_bin = (max_histogram_range + 1 + (num_bins - 1)) / num_bins,  bin = column / size_of_bin,  column = contig offset + POS - 1.
 * A record counts iff its column lies in [column_begin, column_end], and it counts once per callset of its file whose row lies in
 * [lb_callset_row_idx, ub_callset_row_idx]; a file without such a callset is not opened.  counts: num_bins values, filled on success only.
 * Refused before anything runs: num_bins == 0, a negative max_histogram_range, counters that do not fit in device memory, CSV cell files (by name).
 * Errors that name file and 1-based line / record: a counted column above max_histogram_range, a contig that is not in the vid, POS / END that is no plain
 * integer, fewer than 8 columns.  text_budget_bytes and inflate_mode as for gdbamd_import_cells_device_ex.  stats may be NULL. */
typedef struct gdbamd_histogram_stats {
  int64_t num_files, num_records, num_counted;  /* files read; record lines / records seen; those inside the column bounds */
  uint64_t total_weight;                        /* the sum of all bins */
  int64_t num_batches, num_atomics;             /* batches; atomic adds on the counters (one per run of equal bins inside a wavefront) */
  double ms_index, ms_inflate, ms_histogram;    /* HIP-event ms of the index pass, the BGZF inflate kernel and the histogram kernel, summed over the batches */
  double s_read, s_h2d, s_total;                /* wall seconds of file read (+ host inflate), uploads, the whole call */
} gdbamd_histogram_stats;
int gdbamd_input_histogram(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int64_t max_histogram_range, uint64_t num_bins,
                           int64_t column_begin, int64_t column_end, int64_t lb_callset_row_idx, int64_t ub_callset_row_idx, int device,
                           uint64_t text_budget_bytes, int inflate_mode, int nstreams, const char* const* names, const void* const* data,
                           const uint64_t* stream_nbytes, uint64_t* counts, gdbamd_histogram_stats* stats);
/* Histogram::print of the reference: "Histogram: [\n", then "lo,hi,count\n" for every non-zero bin (lo = b * size_of_bin, hi = (b + 1) * size_of_bin - 1), then
 * "]\n".  Returns the length of the text (dst may be NULL: call once to measure, once to write), -1 when num_bins is 0 or max_histogram_range negative */
int64_t gdbamd_histogram_text(const uint64_t* counts, uint64_t num_bins, int64_t max_histogram_range, char* dst, uint64_t cap);
/* vcfdiff on GPU `device` (kernels/gdb_vcfdiff.hip; reference tools/src/vcfdiff.cc): two VCF text files - plain, gzip or BGZF - compared record by record,
 * the order of ALT alleles (AD / PL / AF and the like go through the allele permutation), of INFO keys, FORMAT keys and sample columns and float noise below
 * `threshold` aside; DESIGN.md, "Comparing two VCFs", has the rule.  regions: NULL / "" or chr | chr:pos | chr:from-to | chr:from- , comma separated.
 * *report_json is one JSON document, malloc'ed: release with gdbamd_free:
 *   {"compared": pairs compared, "events": [{"kind": "COMPARED" | "REF_BLOCKS_OVERLAP" | "DIFFERENT_POSITIONS" | "EXTRA_LINES", "gold_line", "test_line" (1-based,
 *    0: none), "gold_text", "test_text", and where a compare ran "flags": ["ID" | "ALLELES" | "QUAL" | "FILTER"], "info" and "format": {"MISSING_IN_TEST",
 *    "ADDED_IN_TEST", "TYPE_DIFFERS", "DIFFERS": [field names]}}]}   in order; a COMPARED pair is listed only when a bit is set.
 * Refused before anything runs: BCF2 input, differing or duplicate sample names, more than 64 distinct INFO or FORMAT names.  Errors that name file and
 * 1-based line: a contig or an INFO / FORMAT key that the file's header lacks, fewer than 8 columns, POS / END that is no plain integer, a contig whose
 * records are not contiguous or whose POS goes back.  Both files' text must fit in device memory.  stats may be NULL. */
typedef struct gdbamd_vcfdiff_stats {
  int64_t gold_records, test_records;           /* record lines inside the regions */
  int64_t pairs_compared, pairs_light, pairs_heavy;  /* pairs; those on the lane-per-sample path; those on the wavefront-per-sample path */
  int64_t deferred;                             /* float token pairs outside the device parser's exact range, decided by the host */
  int64_t events, num_batches;
  uint64_t resident_bytes;                      /* text and tab index kept on the device */
  double ms_index, ms_inflate, ms_keys, ms_compare;  /* HIP-event ms per phase, summed */
  double s_read, s_walk, s_total;               /* wall seconds of file read (+ host inflate), the host's walk, the whole call */
} gdbamd_vcfdiff_stats;
int gdbamd_vcfdiff(const char* gold, const char* test, double threshold, const char* regions, int device, uint64_t text_budget_bytes, char** report_json,
                   gdbamd_vcfdiff_stats* stats);
/* The streaming importer (GenomicsDBImporter, csrc/api/genomicsdb_importer.h; kernels/gdb_import_stream.hip): buffer streams of VCF text or BCF2
 * records imported batch by batch on one GPU with bounded device memory; INTEGRATION.md has the protocol.  loader_json: the path of a loader JSON, or
 * the JSON itself (a string that begins with '{').  device < 0: GDBAMD_DEVICE, else LOCAL_RANK, else 0.  Every call but create and destroy returns 0
 * on success and -1 on an error, whose text gdb_mi355_last_error has; create returns NULL on an error.
 *   add_buffer_stream  before setup_loader only; init: the header (VCF text through the #CHROM line, or BCF\2\2 + l_text + text)
 *   setup_loader       callsets_json: NULL / "" or {"callsets": ..} to join those of the loader's callset_mapping_file; *max_identifiers: the number of used streams
 *   stream_file_idx    the stream's index among the sources of the callset mapping, -1: no callset inside the row bounds uses it
 *   write              whole records; replaces the stream's buffer; partition_idx must be 0
 *   import_batch       *cells (cells may be NULL: the cells are not wanted) is malloc'ed, release with gdbamd_free; exhausted_pairs: room for 2 * max_identifiers
 *                      values, receives (stream, 0) pairs, *n_exhausted their number.  A reported stream is refilled, or ended by a write of 0 bytes or by no write
 *   is_done            1 when every used stream has ended and nothing is pending, else 0
 *   finish             only when done: the loader's outputs (produce_tiledb_array, produce_combined_vcf, ..)
 *   stats              GDBAMD_IMPORTER_NUM_STATS doubles: 0 batches, 1 records, 2 cells and 3 bytes handed over, 4 max pending cells, 5 max pending bytes,
 *                      6 deferred values, 7 cells replayed at the partition begin, 8..11 HIP-event ms of order check / classify / sort + gather / compact,
 *                      12..13 wall seconds of H2D and D2H */
#define GDBAMD_IMPORTER_NUM_STATS 14
void* gdbamd_importer_create(const char* loader_json, int rank, int device);
int gdbamd_importer_add_buffer_stream(void* importer, const char* name, int is_bcf, uint64_t capacity, const uint8_t* init, uint64_t init_nbytes);
int gdbamd_importer_setup_loader(void* importer, const char* callsets_json, int64_t* max_identifiers);
int gdbamd_importer_stream_file_idx(void* importer, int64_t stream_idx, int64_t* file_idx);
int gdbamd_importer_write(void* importer, int64_t stream_idx, unsigned partition_idx, const uint8_t* data, uint64_t nbytes);
int gdbamd_importer_import_batch(void* importer, uint8_t** cells, uint64_t* nbytes, int64_t* exhausted_pairs, int64_t* n_exhausted);
int gdbamd_importer_is_done(void* importer);
int gdbamd_importer_finish(void* importer);
int gdbamd_importer_stats(void* importer, double* stats);
void gdbamd_importer_destroy(void* importer);
/* {"contigs":[{"<name>":[begin,end]},...]}: the 1-based chromosome intervals that column partition `rank` of the loader JSON covers (reference
 * VidMapper::get_contig_intervals_for_column_partition, vid_mapper.cc:576-609).  *json is malloc'ed: release with gdbamd_free */
int gdbamd_chromosome_intervals_for_column_partition(const char* loader_json, int rank, char** json);
void gdbamd_free(void* p);

#ifdef __cplusplus
}
#endif
#endif
