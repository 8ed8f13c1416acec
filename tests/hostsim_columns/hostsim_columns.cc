// hostsim_columns.cc - CPU harness around the bodies of the column decoder (csrc/core/gdb_columns.hpp): the passes of
// kernels/gdb_columns.hip in the same order - measure every record, raise the faults, scan the allele lengths, site, scatter - with a
// loop where the device has a grid.  Test infrastructure only.  Built twice: as a library that tests/test_columns_bodies_cpu.py
// loads, and (-DHOSTSIM_COLUMNS_MAIN) as a stand-alone program under the address and undefined-behaviour sanitizers that decodes a
// "bu" stream from a file and prints a hash of every column.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/core/gdb_columns.hpp"

using namespace genomicsdb_amd;
using namespace genomicsdb_amd::gdbcol;

namespace {
struct Column { std::string name; int dtype = 0, ndim = 0; int64_t shape[3] = {0, 0, 0}; std::vector<uint8_t> data; };
struct Result { std::vector<Column> cols; };

Column make_column(const std::string& name, int dtype, int ndim, int64_t a, int64_t b = 1, int64_t c = 1) {
  Column col; col.name = name; col.dtype = dtype; col.ndim = ndim; col.shape[0] = a; col.shape[1] = ndim > 1 ? b : 0; col.shape[2] = ndim > 2 ? c : 0;
  col.data.assign((size_t)(a * b * c) * col_dtype_size(dtype) + 8, 0);      // (+ 8: data() of an empty column is a pointer all the same)
  return col;
}

Result* decode(const uint8_t* page, const uint64_t* rec_off, int64_t R, int n_sample, const int64_t* contig_off, int n_contig, const ColFields& Q,
               const std::vector<std::string>& names, std::string* error) {
  std::vector<ColEntry> E((size_t)R * (size_t)std::max(Q.n, 1));
  std::vector<ColRecord> rec((size_t)R);
  std::vector<int64_t> alleles_off((size_t)R + 1, 0);
  std::vector<uint32_t> err((size_t)kColErrWords, 0xFFFFFFFFu), max_len((size_t)kColMaxFields, 1u);
  err[0] = 0;
  auto fail = [&]() -> bool {
    uint32_t r; int kind, field;
    if (!col_first_fault(err.data(), &r, &kind, &field)) return false;
    const int64_t pos = rec_off[r + 1] - rec_off[r] >= 16 ? (int64_t)(int32_t)bcf_u32(page + rec_off[r], 12) + 1 : 0;
    const bool whole = kind == COL_ERR_RECORD;
    *error = col_fault_text(kind, whole ? "" : names[(size_t)field], whole ? 0 : Q.f[field].dtype, whole ? 0 : Q.f[field].width, pos, r);
    return true;
  };
  // measure
  for (int64_t r = 0; r < R; ++r) {
    uint64_t bytes = 0;
    const ColFault f = col_measure(Q, page, rec_off[r], rec_off[r + 1], n_sample, n_contig, E.data() + (size_t)r * Q.n, &rec[(size_t)r], &alleles_off[(size_t)r], max_len.data(), &bytes);
    if (col_faulted(f)) col_raise(err.data(), f, (uint32_t)r);
  }
  if (fail()) return nullptr;
  // scan
  int64_t total = 0;
  for (int64_t r = 0; r <= R; ++r) { const int64_t n = r < R ? alleles_off[(size_t)r] : 0; alleles_off[(size_t)r] = total; total += n; }
  // site
  Result* res = new Result;
  res->cols.push_back(make_column("contig", COL_INT32, 1, R));
  res->cols.push_back(make_column("pos", COL_INT64, 1, R));
  res->cols.push_back(make_column("end", COL_INT64, 1, R));
  res->cols.push_back(make_column("column", COL_INT64, 1, R));
  res->cols.push_back(make_column("qual", COL_FLOAT32, 1, R));
  res->cols.push_back(make_column("n_allele", COL_INT32, 1, R));
  res->cols.push_back(make_column("alleles", COL_UINT8, 1, total));
  res->cols.push_back(make_column("alleles_off", COL_INT64, 1, R + 1));
  memcpy(res->cols[7].data.data(), alleles_off.data(), (size_t)(R + 1) * sizeof(int64_t));
  ColSiteOut so{(int32_t*)res->cols[0].data.data(), (int64_t*)res->cols[1].data.data(), (int64_t*)res->cols[2].data.data(), (int64_t*)res->cols[3].data.data(),
                (uint32_t*)res->cols[4].data.data(), (int32_t*)res->cols[5].data.data(), res->cols[6].data.data(), alleles_off.data()};
  for (int64_t r = 0; r < R; ++r) col_site(page, rec_off[r], rec[(size_t)r], contig_off, r, so);
  // scatter
  for (int i = 0; i < Q.n; ++i) {
    const ColField& q = Q.f[i];
    const uint32_t W = q.width > 0 ? (uint32_t)q.width : max_len[(size_t)i];
    const int64_t N = q.is_info ? 1 : n_sample;
    Column out = q.is_info ? make_column(names[(size_t)i], q.dtype, 2, R, W) : make_column(names[(size_t)i], q.dtype, 3, R, N, W);
    Column phase;
    if (q.is_gt) phase = make_column(names[(size_t)i] + "_phase", COL_UINT8, 3, R, N, W);
    const uint32_t es = col_dtype_size(q.dtype);
    for (int64_t r = 0; r < R; ++r)
      for (int64_t s = 0; s < N; ++s) {
        const size_t at = (size_t)(r * N + s) * W;
        const ColFault f = col_scatter(q, i, E[(size_t)r * Q.n + i], page, (uint64_t)s, W, out.data.data() + at * es, q.is_gt ? phase.data.data() + at : nullptr);
        if (col_faulted(f)) col_raise(err.data(), f, (uint32_t)r);
      }
    res->cols.push_back(std::move(out));
    if (q.is_gt) res->cols.push_back(std::move(phase));
  }
  if (fail()) { delete res; return nullptr; }
  return res;
}

ColFields fields_of(int nf, const int32_t* keys, const int32_t* dtypes, const int32_t* widths, const int32_t* flags) {
  ColFields Q; memset(&Q, 0, sizeof(Q));
  Q.n = nf;
  for (int i = 0; i < nf; ++i) {
    Q.f[i].key = keys[i]; Q.f[i].dtype = dtypes[i]; Q.f[i].width = widths[i];
    Q.f[i].is_info = flags[i] & 1; Q.f[i].is_float = (flags[i] >> 1) & 1; Q.f[i].is_gt = (flags[i] >> 2) & 1;
  }
  return Q;
}
}  // namespace

extern "C" {
// flags: bit 0 INFO field, bit 1 float field, bit 2 GT.  -> handle, or NULL with the fault's text in err
void* hostsim_columns_decode(const uint8_t* page, const uint64_t* rec_off, int64_t R, int n_sample, const int64_t* contig_off, int n_contig, int nf,
                             const char* const* names, const int32_t* keys, const int32_t* dtypes, const int32_t* widths, const int32_t* flags, char* err, uint64_t err_cap) {
  if (nf < 0 || nf > kColMaxFields) { snprintf(err, err_cap, "more than %d fields", kColMaxFields); return nullptr; }
  std::vector<std::string> nm;
  for (int i = 0; i < nf; ++i) nm.push_back(names[i]);
  std::string text;
  Result* res = decode(page, rec_off, R, n_sample, contig_off, n_contig, fields_of(nf, keys, dtypes, widths, flags), nm, &text);
  if (!res) snprintf(err, err_cap, "%s", text.c_str());
  return res;
}
int hostsim_columns_count(void* h) { return (int)((Result*)h)->cols.size(); }
int hostsim_columns_get(void* h, int i, char* name, uint64_t name_cap, int* dtype, int* ndim, int64_t* shape, const void** data) {
  const Column& c = ((Result*)h)->cols[(size_t)i];
  snprintf(name, name_cap, "%s", c.name.c_str());
  *dtype = c.dtype; *ndim = c.ndim; shape[0] = c.shape[0]; shape[1] = c.shape[1]; shape[2] = c.shape[2]; *data = c.data.data();
  return 0;
}
void hostsim_columns_free(void* h) { delete (Result*)h; }
}

#ifdef HOSTSIM_COLUMNS_MAIN
// hostsim_columns_main STREAM.bcf N_SAMPLE N_CONTIG [name:key:dtype:width:flags ...]
// prints "name dtype shape fnv1a64" per column, or "fault: <text>" (exit status 3)
int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s STREAM.bcf N_SAMPLE N_CONTIG [name:key:dtype:width:flags ...]\n", argv[0]); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  std::vector<uint8_t> data;
  uint8_t buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) data.insert(data.end(), buf, buf + n);
  fclose(fp);
  if (data.size() < 9 || memcmp(data.data(), "BCF\2\2", 5) != 0) { fprintf(stderr, "no BCF2 stream\n"); return 2; }
  const uint64_t body = 9ull + bcf_u32(data.data(), 5);
  if (body > data.size()) { fprintf(stderr, "header runs past the file\n"); return 2; }
  std::vector<uint8_t> page(data.begin() + (std::ptrdiff_t)body, data.end());      // exactly the records: a read past them is the sanitizer's to find
  std::vector<uint64_t> rec_off{0};
  while (rec_off.back() + 8 <= page.size()) {
    const uint64_t at = rec_off.back(), len = 8ull + bcf_u32(page.data() + at, 0) + bcf_u32(page.data() + at, 4);
    if (at + len > page.size()) break;
    rec_off.push_back(at + len);
  }
  if (rec_off.back() != page.size()) { fprintf(stderr, "truncated record\n"); return 2; }
  const int n_sample = atoi(argv[2]), n_contig = atoi(argv[3]);
  std::vector<int64_t> contig_off((size_t)std::max(n_contig, 1));
  for (int i = 0; i < n_contig; ++i) contig_off[(size_t)i] = (int64_t)i * 1000000000ll;
  std::vector<std::string> names;
  std::vector<int32_t> keys, dtypes, widths, flags;
  for (int a = 4; a < argc; ++a) {
    char name[128]; int k, d, w, f;
    if (sscanf(argv[a], "%127[^:]:%d:%d:%d:%d", name, &k, &d, &w, &f) != 5) { fprintf(stderr, "bad field %s\n", argv[a]); return 2; }
    names.push_back(name); keys.push_back(k); dtypes.push_back(d); widths.push_back(w); flags.push_back(f);
  }
  if (names.size() > (size_t)kColMaxFields) { fprintf(stderr, "too many fields\n"); return 2; }
  std::string text;
  Result* res = decode(page.data(), rec_off.data(), (int64_t)rec_off.size() - 1, n_sample, contig_off.data(), n_contig,
                       fields_of((int)names.size(), keys.data(), dtypes.data(), widths.data(), flags.data()), names, &text);
  if (!res) { printf("fault: %s\n", text.c_str()); return 3; }
  for (const Column& c : res->cols) {
    const int64_t n = c.shape[0] * (c.ndim > 1 ? c.shape[1] : 1) * (c.ndim > 2 ? c.shape[2] : 1);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < (size_t)n * col_dtype_size(c.dtype); ++i) { h ^= c.data[i]; h *= 1099511628211ull; }
    printf("%s %d %lld,%lld,%lld %016llx\n", c.name.c_str(), c.dtype, (long long)c.shape[0], (long long)c.shape[1], (long long)c.shape[2], (unsigned long long)h);
  }
  delete res;
  return 0;
}
#endif
