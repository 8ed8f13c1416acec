// harness.cc - TEST infrastructure: drives the GenomicsDBImporter natives (genomicsdb_amd/csrc/jni/jni_importer.cc) the way the JVM
// would, without a JVM: the library is opened by its path and the natives are looked up by their JNI names; the JNIEnv's interface
// function table holds plain C++ stand-ins for the functions the glue uses, at the specification's table indices.
//   jni_importer_harness <libtiledbgenomicsdb.so> <loader.json> <stream_to_filename.json> <buffer_size>
// Call order = GATK's GenomicsDBImporter.java: GetChromosomeIntervalsForColumnPartition, InitializeGenomicsDBImporterObject, CopyVidMap,
// CopyCallsetMap, AddBufferStream per stream (the header), SetupGenomicsDBLoader, WriteDataToBufferStream per stream, then ImportBatch
// and WriteDataToBufferStream for every reported stream until ImportBatch returns true.  Prints the chromosome intervals.
#include <dlfcn.h>
#include <jni.h>
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/common/mini_json.hpp"

#ifndef GDBAMD_STUB_JNI
#error "the harness is built against csrc/jni/stub/jni.h"
#endif

namespace {
struct FakeString : _jstring { std::string s; };
struct FakeBytes : _jbyteArray { std::vector<jbyte> v; };
struct FakeLongs : _jlongArray { std::vector<jlong> v; };
struct FakeClass : _jclass { std::string name; };
struct FakeEnv : JNIEnv_ {
  JNINativeInterface_ table;
  bool exception_pending = false;
  std::string exception_text;
  FakeClass io_exception;
  std::vector<FakeString*> made;
};
jclass f_FindClass(JNIEnv* e, const char* name) { FakeEnv* fe = static_cast<FakeEnv*>(e); fe->io_exception.name = name; return &fe->io_exception; }
jint f_ThrowNew(JNIEnv* e, jclass, const char* msg) { FakeEnv* fe = static_cast<FakeEnv*>(e); fe->exception_pending = true; fe->exception_text = msg ? msg : ""; return 0; }
jstring f_NewStringUTF(JNIEnv* e, const char* utf) { FakeString* s = new FakeString; s->s = utf; static_cast<FakeEnv*>(e)->made.push_back(s); return s; }
const char* f_GetStringUTFChars(JNIEnv*, jstring s, jboolean* is_copy) { if (is_copy) *is_copy = JNI_FALSE; return static_cast<FakeString*>(s)->s.c_str(); }
void f_ReleaseStringUTFChars(JNIEnv*, jstring, const char*) {}
jbyte* f_GetByteArrayElements(JNIEnv*, jbyteArray a, jboolean* is_copy) { if (is_copy) *is_copy = JNI_FALSE; return static_cast<FakeBytes*>(a)->v.data(); }
void f_ReleaseByteArrayElements(JNIEnv*, jbyteArray, jbyte*, jint) {}
jlong* f_GetLongArrayElements(JNIEnv*, jlongArray a, jboolean* is_copy) { if (is_copy) *is_copy = JNI_FALSE; return static_cast<FakeLongs*>(a)->v.data(); }
void f_ReleaseLongArrayElements(JNIEnv*, jlongArray, jlong*, jint) {}

std::string read_file(const std::string& path) {      // plain or gzip
  gzFile f = gzopen(path.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
  std::string out;
  char buf[1 << 16];
  int n;
  while ((n = gzread(f, buf, sizeof(buf))) > 0) out.append(buf, (size_t)n);
  gzclose(f);
  return out;
}
struct Source {
  std::string name, data; size_t pos = 0;
  FakeBytes next(size_t room) {      // whole lines up to `room` bytes, at least one
    const size_t begin = pos;
    while (pos < data.size()) {
      const size_t nl = data.find('\n', pos);
      const size_t end = nl == std::string::npos ? data.size() : nl + 1;
      if (pos > begin && end - begin > room) break;
      pos = end;
    }
    FakeBytes b;
    b.v.assign(data.begin() + (long)begin, data.begin() + (long)pos);
    b.v.resize(b.v.size() + 1);      // (an array is never empty here; the count says how many bytes are valid)
    return b;
  }
};
template <class F> F sym(void* lib, const char* name) {
  void* p = dlsym(lib, (std::string("Java_com_intel_genomicsdb_importer_GenomicsDBImporterJni_") + name).c_str());
  if (!p) { fprintf(stderr, "no symbol %s\n", name); exit(2); }
  return reinterpret_cast<F>(p);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 5) { fprintf(stderr, "usage: jni_importer_harness <library> <loader.json> <stream_to_filename.json> <buffer_size>\n"); return 2; }
  void* lib = dlopen(argv[1], RTLD_NOW);
  if (!lib) { fprintf(stderr, "%s\n", dlerror()); return 2; }
  const size_t buffer_size = strtoull(argv[4], nullptr, 10);
  FakeEnv env;
  memset(&env.table, 0, sizeof(env.table));
  env.table.slot[6] = (void*)f_FindClass; env.table.slot[14] = (void*)f_ThrowNew; env.table.slot[167] = (void*)f_NewStringUTF; env.table.slot[169] = (void*)f_GetStringUTFChars;
  env.table.slot[170] = (void*)f_ReleaseStringUTFChars; env.table.slot[184] = (void*)f_GetByteArrayElements; env.table.slot[188] = (void*)f_GetLongArrayElements;
  env.table.slot[192] = (void*)f_ReleaseByteArrayElements; env.table.slot[196] = (void*)f_ReleaseLongArrayElements;
  env.functions = &env.table;
  auto check = [&](const char* where) { if (env.exception_pending) { fprintf(stderr, "%s: %s\n", where, env.exception_text.c_str()); exit(1); } };

  auto intervals = sym<jstring (*)(JNIEnv*, jclass, jstring, jint)>(lib, "jniGetChromosomeIntervalsForColumnPartition");
  auto init = sym<jlong (*)(JNIEnv*, jobject, jstring, jint)>(lib, "jniInitializeGenomicsDBImporterObject");
  auto copy_vid = sym<jlong (*)(JNIEnv*, jobject, jlong, jbyteArray)>(lib, "jniCopyVidMap");
  auto copy_callsets = sym<jlong (*)(JNIEnv*, jobject, jlong, jbyteArray)>(lib, "jniCopyCallsetMap");
  auto add = sym<void (*)(JNIEnv*, jobject, jlong, jstring, jboolean, jlong, jbyteArray, jlong)>(lib, "jniAddBufferStream");
  auto setup = sym<jlong (*)(JNIEnv*, jobject, jlong, jstring)>(lib, "jniSetupGenomicsDBLoader");
  auto write = sym<void (*)(JNIEnv*, jobject, jlong, jint, jint, jbyteArray, jlong)>(lib, "jniWriteDataToBufferStream");
  auto import_batch = sym<jboolean (*)(JNIEnv*, jobject, jlong, jlongArray)>(lib, "jniImportBatch");
  sym<jint (*)(JNIEnv*, jobject, jstring, jint)>(lib, "jniGenomicsDBImporter");      // (the file import: present; tests/test_import_device.py runs it as vcf2tiledb)

  FakeString loader;
  loader.s = argv[2];
  jstring text = intervals(&env, nullptr, &loader, 0);
  check("GetChromosomeIntervalsForColumnPartition");
  printf("%s\n", static_cast<FakeString*>(text)->s.c_str());

  jlong h = init(&env, nullptr, &loader, 0);
  check("InitializeGenomicsDBImporterObject");
  FakeBytes none;
  none.v.resize(1);
  if (copy_vid(&env, nullptr, h, &none) != h || copy_callsets(&env, nullptr, h, &none) != h) { fprintf(stderr, "CopyVidMap / CopyCallsetMap changed the handle\n"); return 1; }

  const mini_json::Value map = mini_json::parse_file(argv[3]);
  std::vector<Source> sources;
  for (const auto& kv : map.obj) {
    Source s;
    s.name = kv.first;
    s.data = read_file(kv.second.GetString());
    while (s.pos < s.data.size() && s.data[s.pos] == '#') { const size_t nl = s.data.find('\n', s.pos); s.pos = nl == std::string::npos ? s.data.size() : nl + 1; }
    FakeString name;
    name.s = s.name;
    FakeBytes head;
    head.v.assign(s.data.begin(), s.data.begin() + (long)s.pos);
    add(&env, nullptr, h, &name, JNI_FALSE, (jlong)buffer_size, &head, (jlong)s.pos);
    check("AddBufferStream");
    sources.push_back(s);
  }
  FakeString no_callsets;
  const jlong max_ids = setup(&env, nullptr, h, &no_callsets);
  check("SetupGenomicsDBLoader");
  if (max_ids != (jlong)sources.size()) { fprintf(stderr, "SetupGenomicsDBLoader: %lld identifiers for %zu streams\n", (long long)max_ids, sources.size()); return 1; }
  for (size_t i = 0; i < sources.size(); ++i) {
    FakeBytes b = sources[i].next(buffer_size);
    write(&env, nullptr, h, (jint)i, 0, &b, (jlong)b.v.size() - 1);
    check("WriteDataToBufferStream");
  }
  FakeLongs ids;
  ids.v.assign(2 * (size_t)max_ids + 1, -7);
  for (int batches = 0;; ++batches) {
    if (batches > 100000) { fprintf(stderr, "the import does not end\n"); return 1; }
    const jboolean done = import_batch(&env, nullptr, h, &ids);
    check("ImportBatch");
    if (done) break;
    const jlong n = ids.v[2 * (size_t)max_ids];
    if (n <= 0 || n > max_ids) { fprintf(stderr, "ImportBatch: %lld exhausted streams\n", (long long)n); return 1; }
    for (jlong k = 0; k < n; ++k) {
      const jlong s = ids.v[2 * (size_t)k], part = ids.v[2 * (size_t)k + 1];
      if (s < 0 || s >= (jlong)sources.size() || part != 0) { fprintf(stderr, "ImportBatch: identifier (%lld, %lld)\n", (long long)s, (long long)part); return 1; }
      FakeBytes b = sources[(size_t)s].next(buffer_size);
      write(&env, nullptr, h, (jint)s, 0, &b, (jlong)b.v.size() - 1);
      check("WriteDataToBufferStream");
    }
  }
  for (FakeString* s : env.made) delete s;
  return 0;
}
