// gdb_import_csv.hpp - bodies of the device importer's CSV path: one line of a CSV cell file -> one begin-cell.  The format is the
// reference loader's CSV2TileDBBinary (src/main/cpp/src/loader/tiledb_loader_text_file.cc:281-519, include/vcf/vcf.h:238-337):
// no header, one cell per non-empty line, tokens separated by ',' in the order of the binary cell,
//   row, column, END, REF, ALT, QUAL, FILTER, INFO attributes in vid order, FORMAT attributes in vid order
// with a fixed-length attribute of k elements as k tokens, a variable-length numeric attribute (FILTER and GT among them) as a count
// token and that many element tokens, and REF, ALT and a variable-length char attribute as one token copied verbatim.  When
// attributes are still open behind the last token, ONE empty token is supplied (handle_end_of_line).
// Plain functions that compile under g++ and hipcc (GDB_HD), like core/gdb_import.hpp whose sink, tables and slots they use: the
// kernels of kernels/gdb_import.hip and the CPU harness tests/hostsim_import_csv/ run the same code.
//
// Numbers.  A numeric token that is empty or begins with '*' is the TileDB null of its type.  The tokens that decide what a line
// becomes - row, column, END and the counts - are read here in full by imp_csv_integer, strtoll(tok, &end, 0) in integer arithmetic.
// A value token is taken here only where its bits are certain:
//   integers  -?(0|[1-9][0-9]*) that fit in 64 bits (no '+', no leading zero: base 0 reads those differently or the same, the host decides);
//   floats    the decimal forms of imp_parse_decimal (gdb_import.hpp) whose double is not exactly half way between two floats: the
//             double is then on the same side of every float boundary as the decimal itself, so the cast rounds as strtof does;
//   every other value token is DEFERRED (ImpDeferred, kinds IMP_KIND_CSV_*): the host reads it with strtoll(base 0) / strtof,
//   prefix semantics (host/import_common.hpp).
#pragma once
#include "gdb_import.hpp"

namespace genomicsdb_amd {
namespace gdbimp {

enum ImpCsvErr : uint32_t {         // continue ImpErr / ImpBcfErr
  IMP_ERR_CSV_QUOTE = 4096u,        // a '"' in the line: libcsv's quoting rules are not restated
  IMP_ERR_CSV_COORD = 8192u,        // row, column or END from which nothing can be parsed, or which 64 bits do not hold
  IMP_ERR_CSV_COUNT = 16384u,       // a count token that is null, negative, unparsable, or larger than the tokens the line has left
  IMP_ERR_CSV_EXTRA = 32768u,       // tokens left over after the last attribute
  IMP_ERR_CSV_OPEN = 65536u         // attributes still open after the one supplied empty token
};

constexpr int64_t kNullInt64 = INT64_MAX;

GDB_HD bool imp_csv_is_null(const char* text, ImpTok t) { return t.n() == 0u || text[t.b] == '*'; }

GDB_HD uint32_t imp_csv_digit(char c) {
  if (c >= '0' && c <= '9') return (uint32_t)(c - '0');
  if (c >= 'a' && c <= 'f') return (uint32_t)(c - 'a') + 10u;
  if (c >= 'A' && c <= 'F') return (uint32_t)(c - 'A') + 10u;
  return 99u;
}
// strtoll(token, &end, 0): 0 nothing parsed, 1 fine, 2 out of range (strtoll would saturate)
GDB_HD int imp_csv_integer(const char* p, uint32_t n, int64_t* out) {
  uint32_t i = 0;
  while (i < n && (p[i] == ' ' || (p[i] >= '\t' && p[i] <= '\r'))) ++i;
  bool neg = false;
  if (i < n && (p[i] == '+' || p[i] == '-')) { neg = p[i] == '-'; ++i; }
  uint32_t base = 10;
  if (i < n && p[i] == '0') {
    if (i + 2u < n && (p[i + 1u] == 'x' || p[i + 1u] == 'X') && imp_csv_digit(p[i + 2u]) < 16u) { base = 16; i += 2u; }
    else base = 8;         // (the '0' itself is the first digit)
  }
  const uint64_t limit = neg ? (uint64_t)1 << 63 : ((uint64_t)1 << 63) - 1u;
  uint64_t w = 0;
  bool any = false, fits = true;
  for (; i < n; ++i) {
    const uint32_t d = imp_csv_digit(p[i]);
    if (d >= base) break;
    any = true;
    if (w > (limit - d) / base) fits = false; else w = w * base + d;
  }
  if (!any) return 0;
  if (!fits) return 2;
  *out = neg ? (int64_t)(0u - w) : (int64_t)w;
  return 1;
}

// -?(0|[1-9][0-9]*): the integers base 0 and base 10 read alike
GDB_HD bool imp_csv_plain_int(const char* p, uint32_t n, int64_t* out) {
  const uint32_t s = (n && p[0] == '-') ? 1u : 0u;
  if (s >= n || p[0] == '+' || (p[s] == '0' && n - s > 1u)) return false;
  return imp_parse_int(p, n, out);
}
GDB_HD bool imp_csv_plain_float(const char* p, uint32_t n, float* out) {
  double v;
  if (!imp_parse_decimal(p, n, &v)) return false;
  union { double d; uint64_t u; } x; x.d = v;
  if ((x.u & 0x1FFFFFFFull) == 0x10000000ull) return false;     // exactly half way between two floats: the decimal may lie on either side
  *out = (float)v;
  return true;
}

// the tokens of a line, then the one empty token of handle_end_of_line
struct ImpCsvCursor {
  const char* text; uint32_t at, end; bool supplied;
  GDB_HD bool more() const { return at <= end; }       // real tokens left
  GDB_HD bool next(ImpTok* t) {
    if (at <= end) return imp_next(text, &at, end, ',', t);
    if (supplied) return false;
    supplied = true;
    t->b = t->e = end;
    return true;
  }
};

template <bool W>
GDB_HD void imp_csv_number(ImpSink<W>& o, const char* text, ImpTok t, bool is_int, int what) {
  if (!W) { o.n += 4; return; }
  if (imp_csv_is_null(text, t)) { if (is_int) o.i32(kNullInt); else o.u32(kNullFloatBits); return; }
  if (is_int) {
    int64_t v;
    if (imp_csv_plain_int(text + t.b, t.n(), &v)) o.i32((int32_t)v);
    else o.defer(t, what, IMP_KIND_CSV_INT, 0u, 0);
  } else {
    float f;
    if (imp_csv_plain_float(text + t.b, t.n(), &f)) o.f32(f);
    else o.defer(t, what, IMP_KIND_CSV_FLOAT, 0u, 0);
  }
}

// one attribute: fixed = num_elements tokens, variable-length char = one token, variable-length numeric = count + elements
template <bool W>
GDB_HD void imp_csv_attr(ImpSink<W>& o, ImpCsvCursor& c, bool fixed, uint32_t num_elements, bool is_char, bool is_int, int what) {
  ImpTok t;
  if (is_char) {       // (fixed-length char attributes are refused before any line is read)
    if (!c.next(&t)) { o.err |= IMP_ERR_CSV_OPEN; return; }
    o.chars(c.text, t);
    return;
  }
  uint32_t n = num_elements;
  if (!fixed) {
    if (!c.next(&t)) { o.err |= IMP_ERR_CSV_OPEN; return; }
    int64_t v = 0;
    const int64_t room = (int64_t)c.end - (int64_t)c.at + 2;       // the tokens the rest of the line can hold, the supplied one included
    if (imp_csv_is_null(c.text, t) || imp_csv_integer(c.text + t.b, t.n(), &v) != 1 || v < 0 || v > room) {
      o.err |= IMP_ERR_CSV_COUNT;      // (a larger count cannot be met, and is not walked)
      return;
    }
    n = (uint32_t)v;
    o.i32((int32_t)n);
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (!c.next(&t)) { o.err |= fixed ? IMP_ERR_CSV_OPEN : IMP_ERR_CSV_COUNT; return; }
    imp_csv_number<W>(o, c.text, t, is_int, what);
  }
}

// everything of a cell after [row][col][cell_size], from the cursor behind the column token
template <bool W>
GDB_HD void imp_csv_body(const ImpTables& T, ImpCsvCursor& c, ImpSink<W>& o) {
  ImpTok t;
  int64_t end = kNullInt64;
  if (!c.next(&t)) { o.err |= IMP_ERR_CSV_OPEN; return; }
  if (!imp_csv_is_null(c.text, t) && imp_csv_integer(c.text + t.b, t.n(), &end) != 1) { o.err |= IMP_ERR_CSV_COORD; return; }
  o.i64(end);
  for (int k = 0; k < 2; ++k) {        // REF, ALT
    if (!c.next(&t)) { o.err |= IMP_ERR_CSV_OPEN; return; }
    o.chars(c.text, t);
  }
  imp_csv_attr<W>(o, c, true, 1u, false, false, IMP_WHAT_QUAL);
  if (!o.err) imp_csv_attr<W>(o, c, false, 0u, false, true, IMP_WHAT_FILTER);
  for (int i = 0; i < T.n_info && !o.err; ++i) {
    const ImpAttr& a = T.info[i];
    imp_csv_attr<W>(o, c, a.fixed != 0, a.num_elements, a.elem == GDB_ET_CHAR, a.elem == GDB_ET_INT, i);
  }
  for (int i = 0; i < T.n_fmt && !o.err; ++i) {
    const ImpAttr& a = T.fmt[i];
    imp_csv_attr<W>(o, c, a.fixed != 0, a.num_elements, a.elem == GDB_ET_CHAR, a.elem == GDB_ET_INT, IMP_WHAT_FMT_BASE + i);
  }
  if (!o.err && c.more()) o.err |= IMP_ERR_CSV_EXTRA;
}

// the rows of the file's callsets, ascending
struct ImpCsvRows { const int64_t* row; int32_t n; };
GDB_HD bool imp_csv_has_row(const ImpCsvRows& R, int64_t row) {
  int32_t lo = 0, hi = R.n;
  while (lo < hi) { const int32_t mid = lo + (hi - lo) / 2; if (R.row[mid] < row) lo = mid + 1; else hi = mid; }
  return lo < R.n && R.row[lo] == row;
}

// row and column of a line (both passes); the cursor is left behind the column token.  Returns ImpErr bits
GDB_HD uint32_t imp_csv_coords(const ImpLine& L, ImpCsvCursor* c, int64_t* row, int64_t* col) {
  c->text = L.text; c->at = L.begin; c->end = L.end; c->supplied = false;
  ImpTok t;
  if (!c->next(&t) || imp_csv_integer(L.text + t.b, t.n(), row) != 1) return IMP_ERR_CSV_COORD;
  if (!c->more() || !c->next(&t) || imp_csv_integer(L.text + t.b, t.n(), col) != 1) return IMP_ERR_CSV_COORD;
  return 0;
}

// measure pass of one line.  An empty line gives nothing; a line of another file's row or outside the column partition is dropped
// after its row and column were read (an interval that begins in front of the partition is NOT replayed: the reference's CSV reader
// looks at the column only, tiledb_loader_text_file.cc:234-278).  *row_out: the line's row
GDB_HD ImpSlot imp_csv_measure(const ImpTables& T, const ImpCsvRows& R, const ImpLine& L, int64_t* row_out) {
  ImpSlot s; s.col = 0; s.end = 0; s.size = 0; s.kind = IMP_SLOT_NONE; s.err = 0;
  *row_out = -1;
  if (L.end == L.begin) return s;
  for (uint32_t i = L.begin; i < L.end; ++i) if (L.text[i] == '"') { s.err = IMP_ERR_CSV_QUOTE; return s; }
  ImpCsvCursor c;
  int64_t row = 0;
  s.err = imp_csv_coords(L, &c, &row, &s.col);
  if (s.err) return s;
  *row_out = row;
  if (s.col < T.column_begin || s.col > T.column_end || !imp_csv_has_row(R, row)) return s;
  if (s.col < 0 || (s.col >> (63 - T.key_row_bits)) != 0) { s.err = IMP_ERR_COORD_RANGE; return s; }
  ImpSink<false> o;
  imp_csv_body<false>(T, c, o);
  s.err = o.err;
  if (s.err) return s;
  s.kind = IMP_SLOT_CELL;
  s.size = 24u + o.n;
  return s;
}

// write pass: the cell's bytes at o.out (s.size bytes, as measured); returns ImpErr bits.  *row_out: the line's row, for the sort key
GDB_HD uint32_t imp_csv_write(const ImpTables& T, const ImpLine& L, const ImpSlot& s, ImpSink<true>& o, int64_t* row_out) {
  ImpCsvCursor c;
  int64_t row = 0, col = 0;
  const uint32_t e = imp_csv_coords(L, &c, &row, &col);
  *row_out = row;
  if (e) return e;
  o.limit = s.size;
  o.i64(row); o.i64(s.col); o.i64((int64_t)s.size);
  imp_csv_body<true>(T, c, o);
  return o.err;
}

}  // namespace gdbimp
}  // namespace genomicsdb_amd
