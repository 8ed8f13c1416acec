// jni_importer.cc - the nine native methods of com.intel.genomicsdb.importer.GenomicsDBImporterJni that GATK4's GenomicsDBImport
// reaches (reference src/main/jni/src/genomicsdb_GenomicsDBImporter.cc:37-255; names and argument lists are fixed by the Java
// class), on top of GenomicsDBImporter (csrc/api/genomicsdb_importer.h).  Linked into libtiledbgenomicsdb.so next to the query
// stream's natives; compiled against csrc/jni/stub/jni.h where no JDK is present, like jni_query_stream.cc.
// An error becomes a java.io.IOException where the reference lets its C++ exception escape into the JVM.
#include <jni.h>

#include <cstdint>
#include <exception>
#include <string>
#include <vector>

#include "../api/genomicsdb_importer.h"

using namespace genomicsdb_amd;

namespace {
inline GenomicsDBImporter* importer_of(jlong h) { return reinterpret_cast<GenomicsDBImporter*>(static_cast<std::uintptr_t>(h)); }
void throw_io(JNIEnv* env, const char* what) {
  jclass cls = env->FindClass("java/io/IOException");
  if (cls) env->ThrowNew(cls, what);
}
struct UtfChars {          // GetStringUTFChars / ReleaseStringUTFChars as a scope
  JNIEnv* env; jstring s; const char* p;
  UtfChars(JNIEnv* e, jstring js) : env(e), s(js), p(js ? e->GetStringUTFChars(js, NULL) : NULL) {}
  ~UtfChars() { if (p) env->ReleaseStringUTFChars(s, p); }
};
template <class F, class R> R guarded(JNIEnv* env, F f, R on_error) {
  try { return f(); }
  catch (const std::exception& e) { throw_io(env, e.what()); }
  catch (...) { throw_io(env, "GenomicsDBImporter: unknown exception"); }
  return on_error;
}
}  // namespace

extern "C" {

// the file import of the loader JSON on the device and the loader's outputs: vcf2tiledb --import-on-device
JNIEXPORT jint JNICALL Java_com_intel_genomicsdb_importer_GenomicsDBImporterJni_jniGenomicsDBImporter(JNIEnv* env, jobject, jstring loader_configuration_file, jint rank) {
  UtfChars l(env, loader_configuration_file);
  if (!l.p) { throw_io(env, "GenomicsDBImporter: null loader configuration file"); return -1; }
  return guarded(env, [&]() -> jint { import_files_of_loader(l.p, (int)rank); return 0; }, (jint)-1);
}

JNIEXPORT jlong JNICALL Java_com_intel_genomicsdb_importer_GenomicsDBImporterJni_jniInitializeGenomicsDBImporterObject(JNIEnv* env, jobject, jstring loader_configuration_file,
                                                                                                                    jint rank) {
  UtfChars l(env, loader_configuration_file);
  if (!l.p) { throw_io(env, "GenomicsDBImporter: null loader configuration file"); return 0; }
  return guarded(env, [&]() -> jlong { return static_cast<jlong>(reinterpret_cast<std::uintptr_t>(new GenomicsDBImporter(l.p, (int)rank))); }, (jlong)0);
}

JNIEXPORT void JNICALL Java_com_intel_genomicsdb_importer_GenomicsDBImporterJni_jniAddBufferStream(JNIEnv* env, jobject, jlong handle, jstring stream_name, jboolean is_bcf,
                                                                                                 jlong buffer_capacity, jbyteArray buffer, jlong num_valid_bytes_in_buffer) {
  UtfChars name(env, stream_name);
  if (!name.p || !handle) { throw_io(env, "GenomicsDBImporter: null handle or stream name"); return; }
  jbyte* bytes = buffer ? env->GetByteArrayElements(buffer, NULL) : NULL;
  guarded(env, [&]() -> int {
    importer_of(handle)->add_buffer_stream(name.p, is_bcf ? BCF_BUFFER_STREAM_TYPE : VCF_BUFFER_STREAM_TYPE, (size_t)buffer_capacity, reinterpret_cast<const uint8_t*>(bytes),
                                           bytes ? (size_t)num_valid_bytes_in_buffer : 0);
    return 0;
  }, 0);
  if (bytes) env->ReleaseByteArrayElements(buffer, bytes, 0);
}

// -> the maximum number of buffer stream identifiers a batch can report
JNIEXPORT jlong JNICALL Java_com_intel_genomicsdb_importer_GenomicsDBImporterJni_jniSetupGenomicsDBLoader(JNIEnv* env, jobject, jlong handle,
                                                                                                        jstring buffer_stream_callset_mapping_json_string) {
  UtfChars json(env, buffer_stream_callset_mapping_json_string);
  if (!handle) { throw_io(env, "GenomicsDBImporter: null handle"); return 0; }
  return guarded(env, [&]() -> jlong {
    importer_of(handle)->setup_loader(json.p ? json.p : "");
    return (jlong)importer_of(handle)->get_max_num_buffer_stream_identifiers();
  }, (jlong)0);
}

JNIEXPORT void JNICALL Java_com_intel_genomicsdb_importer_GenomicsDBImporterJni_jniWriteDataToBufferStream(JNIEnv* env, jobject, jlong handle, jint buffer_stream_idx,
                                                                                                         jint partition_idx, jbyteArray buffer,
                                                                                                         jlong num_valid_bytes_in_buffer) {
  if (!handle) { throw_io(env, "GenomicsDBImporter: null handle"); return; }
  jbyte* bytes = buffer ? env->GetByteArrayElements(buffer, NULL) : NULL;
  guarded(env, [&]() -> int {
    GenomicsDBImporter* imp = importer_of(handle);
    if (!imp->is_done()) imp->write_data_to_buffer_stream(buffer_stream_idx, (unsigned)partition_idx, reinterpret_cast<const uint8_t*>(bytes), bytes ? (size_t)num_valid_bytes_in_buffer : 0);
    return 0;
  }, 0);
  if (bytes) env->ReleaseByteArrayElements(buffer, bytes, 0);
}

// fills (stream, partition) pairs and puts their number at index 2 * max; when the import is done it is finished, the importer is
// destroyed and true is returned (reference :168-205)
JNIEXPORT jboolean JNICALL Java_com_intel_genomicsdb_importer_GenomicsDBImporterJni_jniImportBatch(JNIEnv* env, jobject, jlong handle,
                                                                                                 jlongArray exhausted_buffer_stream_identifiers) {
  if (!handle) { throw_io(env, "GenomicsDBImporter: null handle"); return JNI_TRUE; }
  return guarded(env, [&]() -> jboolean {
    GenomicsDBImporter* imp = importer_of(handle);
    if (imp->is_done()) return JNI_TRUE;
    imp->import_batch();
    const std::vector<BufferStreamIdentifier>& ids = imp->get_exhausted_buffer_stream_identifiers();
    jlong* out = env->GetLongArrayElements(exhausted_buffer_stream_identifiers, NULL);
    if (out) {
      for (size_t i = 0; i < ids.size(); ++i) { out[2 * i] = (jlong)ids[i].first; out[2 * i + 1] = (jlong)ids[i].second; }
      out[2 * imp->get_max_num_buffer_stream_identifiers()] = (jlong)ids.size();
      env->ReleaseLongArrayElements(exhausted_buffer_stream_identifiers, out, 0);
    }
    if (!imp->is_done()) return JNI_FALSE;
    imp->finish();
    delete imp;
    return JNI_TRUE;
  }, (jboolean)JNI_TRUE);
}

JNIEXPORT jstring JNICALL Java_com_intel_genomicsdb_importer_GenomicsDBImporterJni_jniGetChromosomeIntervalsForColumnPartition(JNIEnv* env, jclass,
                                                                                                                            jstring loader_configuration_file, jint rank) {
  UtfChars l(env, loader_configuration_file);
  if (!l.p) { throw_io(env, "GenomicsDBImporter: null loader configuration file"); return NULL; }
  return guarded(env, [&]() -> jstring { return env->NewStringUTF(chromosome_intervals_for_column_partition(l.p, (int)rank).c_str()); }, (jstring)NULL);
}

// The reference parses the protobuf bytes of the vid map / callset map and then discards what it parsed (:259-323): the importer goes
// on with the files of its loader JSON.  This build has no protobuf; the bytes are not looked at and the handle comes back unchanged.
JNIEXPORT jlong JNICALL Java_com_intel_genomicsdb_importer_GenomicsDBImporterJni_jniCopyVidMap(JNIEnv*, jobject, jlong handle, jbyteArray) { return handle; }
JNIEXPORT jlong JNICALL Java_com_intel_genomicsdb_importer_GenomicsDBImporterJni_jniCopyCallsetMap(JNIEnv*, jobject, jlong handle, jbyteArray) { return handle; }

}  // extern "C"
