// libvc2hip C-ABI (include/vc2hip.h): context, workspace, launch sequencing, error mapping.
// No torch types, no CPU fallback: every entry point either runs the HIP kernels or fails.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "vc2hip_internal.h"

void vc2_upload_tables_slices(const QuantTables &t, hipStream_t s);
void vc2_upload_tables_transcode(const QuantTables &t, hipStream_t s);
int vc2_halo_x(int kernel);
int vc2_halo_y(int kernel);
void vc2_upload_vlc_lut(hipStream_t s);
void vc2_upload_unpack_lut(hipStream_t s);
bool vc2_slice_index_supported(int prefix, int scalar);
size_t vc2_pack_lds_bytes(int prefix, int scalar);
int vc2_pack_image_mode(int prefix, int scalar);
void vc2_upload_tables_fast(const QuantTables &t, hipStream_t s);
bool vc2_fast_level_applicable(LevelParams &p);
int vc2_launch_forward_fast(Launcher &L, int kernel, bool first, const LevelParams &p, int n, bool store16, hipStream_t s);
int vc2_launch_inverse_fast(Launcher &L, int kernel, bool final_level, const LevelParams &p, int n, bool store16, hipStream_t s);
bool vc2_fast_small_gather(const LevelParams &p);
void vc2_upload_tables_stream(const QuantTables &t, hipStream_t s);
size_t vc2_stream_level_applicable(LevelParams &p, int kernel, bool edge, bool inverse, bool store16, int n_pictures);
int vc2_launch_forward_stream(Launcher &L, int kernel, bool first, const LevelParams &p, int n, bool store16, size_t lds, hipStream_t s);
int vc2_launch_inverse_stream(Launcher &L, int kernel, bool final_level, const LevelParams &p, int n, bool store16, size_t lds, hipStream_t s);
size_t vc2_pair_applicable(PairParams &pp, int kernel, bool edge, bool inverse, bool store16, int n_pictures);
int vc2_launch_forward_pair(Launcher &L, int kernel, bool first, const PairParams &pp, int n, bool store16, size_t lds, hipStream_t s);
int vc2_launch_inverse_pair(Launcher &L, int kernel, bool final_level, const PairParams &pp, int n, bool store16, size_t lds, hipStream_t s);
void vc2_upload_tables_pair(const QuantTables &t, hipStream_t s);
int vc2_launch_plane_transform(Launcher &L, int kernel, int32_t *plane, long long plane_stride, int ph, int pw, int depth, bool inverse,
                               int n, hipStream_t s);
void vc2_launch_plane_ingest(Launcher &L, const void *raw, const RawPlane &rl, int pic_h, int pic_w, int word_bytes, int bit_depth,
                             int32_t *plane, long long plane_stride, int ph, int pw, int n, hipStream_t s);
void vc2_launch_plane_emit(Launcher &L, const int32_t *plane, long long plane_stride, int pw, void *raw, const RawPlane &rl, int pic_h,
                           int pic_w, int word_bytes, int bit_depth, int n, hipStream_t s, int norm = 0);
void vc2_launch_ll_into_plane(Launcher &L, const int32_t *ll, long long ll_stride, int llh, int llw, int32_t *plane, long long plane_stride,
                              int pw, int depth, int n, hipStream_t s);
void vc2_launch_fill_i32(Launcher &L, int32_t *p, int32_t v, size_t n, hipStream_t s);
struct IndexOffsets { const int8_t *p; size_t stride; }; // vc2hip_set_index_offsets, as an encoding call hands it down (p null: none)
void vc2_launch_fill_u64(Launcher &L, unsigned long long *p, unsigned long long v, size_t n, hipStream_t s);

// ------------------------------------------------------------------------------------------
// profiling hook: optional hipEvent pair around every launch
// ------------------------------------------------------------------------------------------
struct ProfEntry {
  std::string name;
  int launches = 0;
  double ms = 0;
};
struct Launcher {
  bool on = false;
  std::string only;               // non-empty: event pairs for the launches of these names only (vc2hip_profile_only: "a" or "a,b,c")
  const char *last_name = nullptr;
  std::string launch_error;
  std::vector<ProfEntry> entries;
  // A start / stop event pair per kernel launch, attached to the launch itself (see VC2_LAUNCH)
  struct Pending { int entry; hipEvent_t a, b; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> pool;
  int cur_entry = -1;
  hipEvent_t get() {
    hipEvent_t e;
    if (!pool.empty()) { e = pool.back(); pool.pop_back(); }
    else (void)hipEventCreate(&e);
    return e;
  }
  void collect() {
    for (auto &p : pending) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { entries[p.entry].ms += ms; entries[p.entry].launches++; }
      pool.push_back(p.a);
      pool.push_back(p.b);
    }
    pending.clear();
  }
};
void vc2_prof_begin(Launcher &L, const char *name, hipStream_t s) {
  (void)s;
  L.last_name = name;
  if (!L.on) return;
  if (!L.only.empty() && ("," + L.only + ",").find(std::string(",") + name + ",") == std::string::npos) return; // (a comma-separated list of names)
  int idx = -1;
  for (size_t i = 0; i < L.entries.size(); ++i) if (L.entries[i].name == name) { idx = (int)i; break; }
  if (idx < 0) { L.entries.push_back(ProfEntry{name, 0, 0}); idx = (int)L.entries.size() - 1; }
  L.cur_entry = idx;
}
void vc2_prof_pair(Launcher &L, hipEvent_t *a, hipEvent_t *b) {
  *a = *b = nullptr;
  if (!L.on || L.cur_entry < 0) return;
  *a = L.get();
  *b = L.get();
  L.pending.push_back(Launcher::Pending{L.cur_entry, *a, *b});
}
void vc2_prof_end(Launcher &L, hipStream_t s) {
  (void)s;
  // every launcher calls this right after its launches: catch launch failures (bad grid / LDS size)
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess && L.launch_error.empty())
    L.launch_error = std::string("kernel launch failed (") + (L.last_name ? L.last_name : "?") + "): " + hipGetErrorString(le);
  L.cur_entry = -1;
#ifdef VC2HIP_ABLATE // VC2HIP_DEBUG_SYNC=1 (tools/probe/fault_bisect.py): wait for every stage and name it -- the last name printed before a fault is the stage at fault
  {
    static const bool dbg_sync = getenv("VC2HIP_DEBUG_SYNC") != nullptr;
    if (dbg_sync) {
      fprintf(stderr, "vc2hip stage %s ...", L.last_name ? L.last_name : "?");
      fflush(stderr);
      const hipError_t e = hipStreamSynchronize(s);
      fprintf(stderr, " %s\n", e == hipSuccess ? "done" : hipGetErrorString(e));
      fflush(stderr);
    }
  }
#endif
}
void vc2_prof_break(Launcher &L) { (void)L; }

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
struct Buf {
  void *p = nullptr;
  size_t cap = 0;
};
enum { B_RAW, B_STORE, B_STOREW, B_LL0, B_LLW, B_QIDX, B_SLOTS, B_SIZES, B_OFFS, B_LENS, B_PAYLOAD,
       B_INDEX, B_PLANE, B_PLANE2, B_CBRB, B_CBRO, B_QM, B_UNITS, B_SEGS,
       B_FRAGS, B_FRAGPIC, B_FRAGJUMP, // stream_write_fragments_dev: fragment tables, per-picture results, the cut's workspace
       B_RSTORE, B_RSTOREW, // encode_recon_batch_dev: the quantised coefficients in the decoder's layout
       B_PLANE_QM,          // plane_inverse: the device copy of the quantisation matrix in plane_qm_held
       B_CAPTAB,            // HQ_CAPPED: the per-picture length table (vc2hip_cap.h)
       B_CAPCOST,           // HQ_CAPPED_FILL: the per-slice costs of the third round
       B_PKIN, B_PKOUT,     // vc2hip_set_packed_format: the planar staging of a call's input and of its output pictures
       B_TCLEN, B_TCQ,      // vc2hip_transcode_batch_dev: the indices handed to the slice coder, the pictures' indices of the capped form
       B_CBRB2, B_CBRO2,    // budget_tables' second slot: the output side of vc2hip_transcode_cbr_batch_dev
       B_COUNT };

struct vc2hip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // The context's work is ordered on a caller's stream: it was made by vc2hip_create_on_stream / _on_stream_with_flags, or it
  // is a vc2hip_set_streams lane of such a context (a lane owns its stream, but the fork event pulls it into whatever the
  // caller's stream is doing -- a graph capture included).  Such a context never waits for the GPU in a batch call and
  // records nothing of its own while its stream is being captured (include/vc2hip.h).
  bool follows_caller = false;
  unsigned *d_err = nullptr;
  unsigned *h_err = nullptr; // pinned: the first VC2_ERRBLK_COPY bytes of the error block
  Buf buf[B_COUNT];
  Launcher L;
  std::string err;
  // cached CBR / LD slice-size tables (re-uploaded only when the parameters change)
  int cbr_key[2][5] = {{-1, -1, -1, -1, -1}, {-1, -1, -1, -1, -1}}; // (two slots: budget_tables)
  uint64_t cbr_total[2] = {0, 0};
  int32_t plane_qm_held[VC2_MAX_BANDS] = {}; // the quantisation matrix in B_PLANE_QM (whole-plane inverse path), entry by entry
  int plane_qm_n = 0;                        // ... and how many entries of it (0: none uploaded yet)
  int debug_skip = 0;
  // VBR payload assembly.  Default: fixed-stride slots + scan + compaction (three launches).
  // VC2HIP_SINGLE_PASS_VBR=1: decoupled look-back inside the pack kernel -- measured 2x SLOWER on
  // MI355X when it was measured (1.28 vs 0.62 + 0.20 ms per 16 UHD pictures: the look-back sits on every workgroup's
  // critical path and the kernel is latency-bound), kept as a tested alternative.
  // Round 6: where k_hq_pack16 codes the slices AND a launch holds enough pictures the look-back IS the default (its grid
  // puts the same tile of all pictures side by side: vc2hip_pack16.h); VC2HIP_FLAG_TWO_PASS_VBR keeps the slots there too.
  bool two_pass_vbr = true;
  bool force_two_pass_vbr = false;
#ifndef VC2_ONE_PASS_MIN_PICTURES
#define VC2_ONE_PASS_MIN_PICTURES 112
#endif
  bool force_generic = false; // VC2HIP_GENERIC_DWT=1: always use the generic level kernels (tests)
  bool allow_store16 = true;  // VC2HIP_STORE32=1: keep the int32 coefficient store on the batch path too (tests, A/B)
  bool allow_planes = true; // decode: band planes for the streaming levels (A/B and test switch VC2HIP_NO_BANDPLANES)
  // Byte band planes (BandPlanes::bytes8): 0 = by what the previous batch looked like (its payload bits per sample, its
  // escapes), 1 = always, 2 = never (VC2HIP_FLAG_PLANES8_ALWAYS / _NEVER).  The choice never changes a result: a value that
  // does not fit a byte escapes to the wide array; it decides between half the band-plane bytes and many escapes.
  int planes8_mode = 0;
  bool planes8_on = false;             // the adaptive state: off until a batch has shown small coefficients
  unsigned long long *d_stat = nullptr; // device: [0] pieces with an escape from a byte plane (k_hq_unpack16<true>)
  unsigned long long *h_stat = nullptr; // pinned: [0] that count, [1..] the batch's payload lengths (first 60 pictures)
  hipEvent_t stat_ev = nullptr;
  bool stat_pending = false, stat_was8 = false, stat_seen = false;
  int stat_n = 0;                      // lengths copied
  int stat_n_total = 0;                // pictures of that batch (the escape count is over all of them)
  int last_plane_bits = 0;             // vc2hip_band_plane_bits: the most recent HQ decode call's band planes (0 none, 16, 8)
  std::vector<vc2hip_dwt_launch> dwt_rec; // vc2hip_dwt_launches: the transform launches of the most recent call that ran one
  bool dwt_rec_stale = true;              // set by every entry point: the next recorded launch starts a new record
  double stat_samples = 0;             // samples per picture of that batch
  int ld_batch = 1;         // pictures of the LD batch being encoded (fill_ld_enc sizes the scratch array with it)
  bool allow_heads = true;  // record heads for the levels below them (A/B and test switch VC2HIP_NO_HEADS)
  bool allow_cbr_index = true; // decode of HQ_CBR pictures: offsets from the budgets, verified (VC2HIP_NO_CBR_INDEX=1: always the general index)
  bool allow_stream = true;   // VC2HIP_NO_STREAM=1: tile kernels instead of the streaming level kernels (tests, A/B)
  bool allow_pair = true;     // VC2HIP_FLAG_NO_PAIR: one launch per transform level (vc2hip_dwt_pair.hip off; tests, A/B)
  bool cbr_general = false;   // VC2HIP_FLAG_CBR_GENERAL: the HQ_CBR search without the register kernels
  bool cap_general = false;   // VC2HIP_FLAG_CAP_GENERAL: the HQ_CAPPED measurement without the register kernel
  bool ld_diagonals = false;  // VC2HIP_FLAG_LD_DIAGONALS: the LD index search with one launch per slice anti-diagonal
  unsigned flags = 0;
  // vc2hip_set_streams(k > 1): device-resident batches are cut into k contiguous sub-batches, each on its own
  // stream and workspace (a child context), forked from / joined to `stream` with events.  The kernels of the
  // sub-batches overlap: the tail of one launch is filled by the next stream's work.
  std::vector<vc2hip_ctx *> lanes;    // lanes[0] is the context itself (its own stream), the others are children
  bool in_split = false;              // the context is running its own sub-batch as lane 0
  hipEvent_t fork_ev = nullptr;
  std::vector<hipEvent_t> join_ev;    // end of lane i's latest sub-batch
  bool lanes_pending = false;         // `stream` has not yet been made to wait for the lanes' latest sub-batches
  struct Range { const uint8_t *lo, *hi; };
  struct LaneUse { std::vector<Range> r, w; bool valid = false; }; // one range per caller buffer of the call (BatchBuf)
  std::vector<LaneUse> lane_use;      // what lane i's latest sub-batch read and wrote (caller buffers)
  std::vector<ProfEntry> merged; // profile of this context and its lanes, rebuilt by vc2hip_profile_count
  // pipelined picture calls: VC2HIP_MAX_INFLIGHT slots, each a child context (own stream and workspace)
  struct Flight {
    vc2hip_ctx *lane = nullptr;
    bool open = false, encode = false;
    uint8_t *payload = nullptr;      // caller's pinned buffer (encode)
    size_t cap = 0;
    unsigned long long *h_len = nullptr; // pinned
  };
  Flight flight[VC2HIP_MAX_INFLIGHT];
  int flight_next = 0;               // slot of the next _begin
  // vc2hip_set_sample_layout: where and how the raw words of the device batch calls lie (pure host state; has_layout false:
  // the file format).  layout_bypass: a host-buffer picture call is running its batch call on the context -- file format.
  vc2hip_sample_layout layout = {};
  bool has_layout = false, layout_bypass = false;
  // vc2hip_set_packed_format: v210 or semi-planar pictures (pure host state as the layout; while set the layout is not used)
  vc2hip_packed_format packed = {};
  bool has_packed = false;
  // vc2hip_set_quant_matrix: the quantisation matrix of every call that takes a vc2hip_coding_params (pure host state as the
  // layout; qm_depth 0: none set, every call uses the default matrix of its wavelet and depth -- effective_matrix)
  int32_t qm[VC2_MAX_BANDS] = {};
  int qm_depth = 0;
  // vc2hip_set_index_offsets: the caller's device map of one int8 per slice (the POINTER is the state; null: none).  Read by
  // the three encoding batch entry points, which hand it down; nothing below them looks here.
  const int8_t *idx_offs = nullptr;
  size_t idx_offs_stride = 0;
};

static const char *code_text(int code) {
  switch (code) {
    case VC2HIP_OK: return "ok";
    case VC2HIP_EINVAL: return "invalid argument";
    case VC2HIP_EQINDEX: return "quantization index exceeds maximum implemented value.";
    case VC2HIP_ESCALAR: return "Slice scalar is too small, consider using a larger slice scalar.";
    case VC2HIP_ECBR_TOOBIG: return "SliceIO, HQ CBR mode: Too many bytes for the slice";
    case VC2HIP_ECBR_LEN: return "Slice component length exceeds 1 byte when divided by slice size scalar. See above for suggestions to prevent this.";
    case VC2HIP_ECBR_WRONG: return "SliceIO, HQ CBR mode: Wrong number of bytes for a slice";
    case VC2HIP_EBOUNDED: return "Attempt to write beyond end of bounded write";
    case VC2HIP_ELD_TOOBIG: return "SliceIO, LD mode: Too many bytes for the U and V slices";
    case VC2HIP_ECAP: return "output buffer too small";
    case VC2HIP_ESTREAM: return "truncated or malformed slice data";
    case VC2HIP_ECODE32: return "quantised coefficient magnitude exceeds 65534 (outside the 32-bit exp-Golomb code domain)";
    case VC2HIP_ESYNTAX: return "VC-2 stream syntax error";
    case VC2HIP_EHIP: return "HIP runtime error";
  }
  return "unknown error";
}
extern "C" const char *vc2hip_error_string(int code) { return code_text(code); }

static int set_err(vc2hip_ctx *c, int code, const char *msg = nullptr) {
  if (c) c->err = msg ? msg : code_text(code);
  return code;
}
static int hip_fail(vc2hip_ctx *c, hipError_t e, const char *what) {
  char b[256];
  snprintf(b, sizeof b, "HIP error in %s: %s", what, hipGetErrorString(e));
  return set_err(c, VC2HIP_EHIP, b);
}
#define HIPCHK(ctx, call)                                       \
  do {                                                          \
    hipError_t e_ = (call);                                     \
    if (e_ != hipSuccess) return hip_fail(ctx, e_, #call);      \
  } while (0)

extern "C" const char *vc2hip_last_error(const vc2hip_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// ---- host-side arithmetic shared with the bindings -----------------------------------------
extern "C" int vc2hip_padded_size(int size, int depth) {
  const int cell = 1 << depth;
  return cell * ((size + cell - 1) / cell);
}
extern "C" int vc2hip_slice_size_is_valid(int depth, int len_luma, int len_chroma, int n_size) {
  if (depth <= 0 || depth > 31) return 0;
  const int unit = 1 << depth;
  const int max_slices = (len_luma < len_chroma ? len_luma : len_chroma) / unit;
  if (n_size <= 0 || n_size > max_slices) return 0;
  const int ts = n_size * unit;
  const int pl = vc2hip_padded_size(len_luma, depth), pc = vc2hip_padded_size(len_chroma, depth);
  const int n = (pl + ts - 1) / ts;
  if (pl % n == 0 && (pl / n) % unit == 0 && pc % n == 0 && (pc / n) % unit == 0) return n;
  return 0;
}
// WaveletTransform.cpp:345-423: float variables, double pow, float log/floor (math.h overloads)
extern "C" int vc2hip_quant_matrix(int kernel, int depth, int32_t *out) {
  static const float A[7] = {1.280868846f, 1.224744871f, 1.280868846f, 1.414213562f, 1.414213562f, 0.682408629f, 1.139917028f};
  static const float B[7] = {0.820572875f, 0.847791248f, 0.809253958f, 0.707106871f, 0.707106871f, 1.367856979f, 0.887168005f};
  static const int S[7] = {1, 1, 1, 0, 1, 0, 1};
  if (kernel < 0 || kernel > 6 || depth < 0 || depth > 30) return VC2HIP_EINVAL;
  if (depth == 0) { out[0] = 0; return 0; }
  const float a2 = A[kernel] * A[kernel], ab = A[kernel] * B[kernel], b2 = B[kernel] * B[kernel];
  std::vector<float> gl(depth + 1), gh(depth + 1), gd(depth + 1);
  float mn = 3.402823466e+38f;
  for (int lv = depth; lv > 0; --lv) {
    const float sc = (float)(pow((double)a2, depth - lv) / pow(2.0, S[kernel] * (depth - lv + 1)));
    gl[lv] = sc * a2; gh[lv] = sc * ab; gd[lv] = sc * b2;
    mn = fminf(fminf(fminf(gl[lv], gh[lv]), gd[lv]), mn);
  }
  auto qv = [&](float g) { return (int)floorf(4.0f * logf(g / mn) / logf(2.0f) + 0.5f); };
  int i = 0;
  out[i++] = qv(gl[1]);
  for (int lv = 1; lv <= depth; ++lv) { out[i++] = qv(gh[lv]); out[i++] = qv(gh[lv]); out[i++] = qv(gd[lv]); }
  return 0;
}
void vc2_allow_lds(const void *kernel, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void *, int>, size_t> done;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  size_t &have = done[std::make_pair(kernel, dev)];
  if (bytes > have) {
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    have = bytes;
  }
}

static int gcd_i(int a, int b) { a = abs(a); b = abs(b); while (b) { int t = a % b; a = b; b = t; } return a; }
extern "C" int vc2hip_slice_bytes(int ys, int xs, int total_bytes, int scalar, int32_t *out) {
  if (ys < 1 || xs < 1 || scalar < 1) return VC2HIP_EINVAL;
  const int n = ys * xs;
  int num = total_bytes / scalar - 4 * n, den = n;
  const int g = gcd_i(num, den);
  if (g) { num /= g; den /= g; }
  const int ratio = num / den, rem = num - ratio * den;
  int residue = 0;
  for (int i = 0; i < n; ++i) {
    residue += rem;
    if (residue < den) out[i] = ratio * scalar + 4;
    else { out[i] = (ratio + 1) * scalar + 4; residue -= den; }
  }
  return 0;
}
// SMPTE 2042-1 quant_factor / quant_offset (the reference holds them as a table, Quantisation.cpp:40-83)
static void make_tables(QuantTables &t) {
  for (int q = 0; q < 120; ++q) {
    const uint64_t base = 1ull << (q / 4);
    uint64_t f;
    switch (q % 4) {
      case 0: f = 4 * base; break;
      case 1: f = (503829 * base + 52958) / 105917; break;
      case 2: f = (665857 * base + 58854) / 117708; break;
      default: f = (440253 * base + 32722) / 65444; break;
    }
    t.qf[q] = (int32_t)(uint32_t)f;
    t.off[q] = q == 0 ? 1 : (q == 1 ? 2 : (int32_t)(((uint32_t)t.qf[q] + 1u)) / 2);
    t.magic[q] = 0;
    t.shift[q] = 0;
    if (t.qf[q] > 1) {
      const uint64_t d = (uint64_t)t.qf[q];
      int l = 0;
      while ((1ull << l) < d) ++l;
      t.magic[q] = (uint32_t)((((1ull << l) - d) << 32) / d + 1);
      t.shift[q] = l - 1;
    }
    const double r = 4.0 / (double)(uint32_t)t.qf[q];
    float up = (float)r;
    if ((double)up < r) up = nextafterf(up, INFINITY);
    t.inv4[q] = up;
  }
}

// ---- lifetime ---------------------------------------------------------------------------------
static int create_common(int device, hipStream_t stream, bool own, vc2hip_ctx **out, unsigned flags = 0) {
  if (!out) return VC2HIP_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return VC2HIP_EHIP;
  vc2hip_ctx *c = new vc2hip_ctx;
  c->device = device;
  // the switches between two correct paths (vc2hip_create_with_flags); only the ablation build (tools/, never the product
  // path) also takes them from the environment, so that its A/B runs need no code
#ifdef VC2HIP_ABLATE
  {
    static const struct { const char *name; unsigned flag; } env[] = {
      {"VC2HIP_STORE32", VC2HIP_FLAG_STORE32}, {"VC2HIP_NO_STREAM", VC2HIP_FLAG_NO_STREAM}, {"VC2HIP_NO_PAIR", VC2HIP_FLAG_NO_PAIR},
      {"VC2HIP_NO_BANDPLANES", VC2HIP_FLAG_NO_BANDPLANES}, {"VC2HIP_NO_HEADS", VC2HIP_FLAG_NO_HEADS},
      {"VC2HIP_NO_CBR_INDEX", VC2HIP_FLAG_NO_CBR_INDEX}, {"VC2HIP_GENERIC_DWT", VC2HIP_FLAG_GENERIC_DWT},
      {"VC2HIP_SINGLE_PASS_VBR", VC2HIP_FLAG_SINGLE_PASS_VBR}, {"VC2HIP_TWO_PASS_VBR", VC2HIP_FLAG_TWO_PASS_VBR}, {"VC2HIP_CBR_GENERAL", VC2HIP_FLAG_CBR_GENERAL}, {"VC2HIP_CAP_GENERAL", VC2HIP_FLAG_CAP_GENERAL},
      {"VC2HIP_PLANES8_ALWAYS", VC2HIP_FLAG_PLANES8_ALWAYS}, {"VC2HIP_PLANES8_NEVER", VC2HIP_FLAG_PLANES8_NEVER}};
    for (const auto &e : env) { const char *v = getenv(e.name); if (v && v[0] == '1') flags |= e.flag; }
    { const char *v = getenv("VC2HIP_LD_ROWS"); if (v && v[0] == '0') flags |= VC2HIP_FLAG_LD_DIAGONALS; }
    { const char *e = getenv("VC2HIP_DEBUG_SKIP"); c->debug_skip = e ? atoi(e) : 0; }
  }
#endif
  c->force_generic = (flags & VC2HIP_FLAG_GENERIC_DWT) != 0;
  c->allow_store16 = !(flags & VC2HIP_FLAG_STORE32);
  c->allow_stream = !(flags & VC2HIP_FLAG_NO_STREAM);
  c->allow_pair = !(flags & VC2HIP_FLAG_NO_PAIR);
  c->allow_planes = !(flags & VC2HIP_FLAG_NO_BANDPLANES);
  c->planes8_mode = (flags & VC2HIP_FLAG_PLANES8_NEVER) ? 2 : (flags & VC2HIP_FLAG_PLANES8_ALWAYS) ? 1 : 0;
  c->allow_heads = !(flags & VC2HIP_FLAG_NO_HEADS);
  c->allow_cbr_index = !(flags & VC2HIP_FLAG_NO_CBR_INDEX);
  c->two_pass_vbr = !(flags & VC2HIP_FLAG_SINGLE_PASS_VBR);
  c->force_two_pass_vbr = (flags & VC2HIP_FLAG_TWO_PASS_VBR) != 0;
  c->cbr_general = (flags & VC2HIP_FLAG_CBR_GENERAL) != 0;
  c->cap_general = (flags & VC2HIP_FLAG_CAP_GENERAL) != 0;
  c->ld_diagonals = (flags & VC2HIP_FLAG_LD_DIAGONALS) != 0;
  c->flags = flags;
  if (hipSetDevice(device) != hipSuccess) { delete c; return VC2HIP_EHIP; }
  if (own) { if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) { delete c; return VC2HIP_EHIP; } }
  c->stream = stream;
  c->own_stream = own;
  c->follows_caller = !own;
  if (hipMalloc((void **)&c->d_err, 256 + 4096) != hipSuccess || // error word, then the LD search tables
     
      hipHostMalloc((void **)&c->h_err, VC2_ERRBLK_COPY) != hipSuccess ||
      hipMalloc((void **)&c->d_stat, 64) != hipSuccess || hipHostMalloc((void **)&c->h_stat, 64 * 8) != hipSuccess ||
      hipEventCreateWithFlags(&c->stat_ev, hipEventDisableTiming) != hipSuccess) { delete c; return VC2HIP_EHIP; }
  (void)hipMemsetAsync(c->d_stat, 0, 64, c->stream);
  (void)hipMemsetAsync(c->d_err, 0, sizeof(unsigned), c->stream);
  QuantTables t;
  make_tables(t);
  vc2_upload_tables(t, c->stream);
  vc2_upload_tables_slices(t, c->stream);
  vc2_upload_tables_fast(t, c->stream);
  vc2_upload_tables_pair(t, c->stream);
  vc2_upload_tables_stream(t, c->stream);
  vc2_upload_tables_recon(t, c->stream);
  vc2_upload_tables_transcode(t, c->stream);
  vc2_upload_vlc_lut(c->stream);
  vc2_upload_unpack_lut(c->stream);
  if (hipStreamSynchronize(c->stream) != hipSuccess) { delete c; return VC2HIP_EHIP; }
  *out = c;
  return VC2HIP_OK;
}
extern "C" int vc2hip_create(int device, vc2hip_ctx **out) { return create_common(device, nullptr, true, out); }
extern "C" int vc2hip_create_with_flags(int device, unsigned flags, vc2hip_ctx **out) { return create_common(device, nullptr, true, out, flags); }
extern "C" int vc2hip_create_on_stream(int device, void *s, vc2hip_ctx **out) { return create_common(device, (hipStream_t)s, false, out); }
extern "C" int vc2hip_create_on_stream_with_flags(int device, void *s, unsigned flags, vc2hip_ctx **out) {
  return create_common(device, (hipStream_t)s, false, out, flags);
}
extern "C" void vc2hip_destroy(vc2hip_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (vc2hip_ctx *l : c->lanes) if (l != c) vc2hip_destroy(l);
  for (auto &f : c->flight) { if (f.lane) vc2hip_destroy(f.lane); if (f.h_len) (void)hipHostFree(f.h_len); }
  for (hipEvent_t e : c->join_ev) (void)hipEventDestroy(e);
  if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
  c->L.collect();
  for (auto e : c->L.pool) (void)hipEventDestroy(e);
  for (auto &b : c->buf) if (b.p) (void)hipFree(b.p);
  if (c->d_err) (void)hipFree(c->d_err);
  if (c->h_err) (void)hipHostFree(c->h_err);
  if (c->h_stat) (void)hipHostFree(c->h_stat);
  if (c->d_stat) (void)hipFree(c->d_stat);
  if (c->stat_ev) (void)hipEventDestroy(c->stat_ev);
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

void vc2_ld_disable_rows();
static int err_from_flags(vc2hip_ctx *c, unsigned f) {
  if (!f) return VC2HIP_OK;
  if (f & VC2_DEVERR_HANDOFF) { // not a property of the input: the batch has to be submitted again
    vc2_ld_disable_rows();
    return set_err(c, VC2HIP_EHIP, "LD index search: a hand-over between workgroups timed out; nothing was written for the batch. "
                                   "The library now searches with one launch per slice diagonal: submit the batch again.");
  }
  if (f & VC2_DEVERR_SYNTAX) {
    static const char *why[VC2_SYN_COUNT] = {"?", "parse info prefix is not BBCD", "unknown parse code",
                                             "data unit runs past the end of the stream", "next_parse_offset is 0",
                                             "end of sequence before the pictures asked for",
                                             "picture parameters differ from the coding parameters",
                                             "quantisation matrix differs from the context's", "asymmetric transform",
                                             "picture before any sequence header and no major version given",
                                             "fragment out of order", "?",
                                             "quantisation matrix entry above 255, the largest the library takes"};
    const unsigned w = *(const unsigned *)((const char *)c->h_err + VC2_ERRBLK_SYNTAX_WHY);
    char b[256];
    if (w == VC2_SYN_SLICE_TOO_LONG) {
      snprintf(b, sizeof b, "picture %llu of the batch has a slice of more than 65535 bytes: a fragment's data length has 16 bits",
               *(const unsigned long long *)((const char *)c->h_err + VC2_ERRBLK_SYNTAX_AT));
      return set_err(c, VC2HIP_ESYNTAX, b);
    }
    snprintf(b, sizeof b, "VC-2 stream syntax error at byte %llu: %s",
             *(const unsigned long long *)((const char *)c->h_err + VC2_ERRBLK_SYNTAX_AT), why[w < VC2_SYN_COUNT ? w : 0]);
    return set_err(c, VC2HIP_ESYNTAX, b);
  }
  if (f & VC2_DEVERR_QINDEX) return set_err(c, VC2HIP_EQINDEX);
  if (f & VC2_DEVERR_SCALAR) return set_err(c, VC2HIP_ESCALAR);
  if (f & VC2_DEVERR_CBR_TOOBIG) return set_err(c, VC2HIP_ECBR_TOOBIG);
  if (f & VC2_DEVERR_CBR_LEN) return set_err(c, VC2HIP_ECBR_LEN);
  if (f & VC2_DEVERR_CODE32) return set_err(c, VC2HIP_ECODE32);
  if (f & VC2_DEVERR_LD_TOOBIG) return set_err(c, VC2HIP_ELD_TOOBIG);
  if (f & VC2_DEVERR_CAP) return set_err(c, VC2HIP_ECAP);
  return set_err(c, VC2HIP_ESTREAM);
}
// make the context's stream wait for whatever its lanes still have in flight
static int join_lanes(vc2hip_ctx *c) {
  if (!c->lanes_pending || c->in_split) return VC2HIP_OK;
  for (size_t i = 1; i < c->lanes.size(); ++i)
    if (c->lane_use[i].valid) HIPCHK(c, hipStreamWaitEvent(c->stream, c->join_ev[i], 0));
  c->lanes_pending = false;
  return VC2HIP_OK;
}
// every entry point that enqueues on the context's stream starts here
static int enter(vc2hip_ctx *c) {
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->in_split) vc2_prof_break(c->L); // whatever the caller enqueued since is not part of the next kernel
  c->dwt_rec_stale = true;
  return join_lanes(c);
}
#define ENTER(ctx) do { int rc_ = enter(ctx); if (rc_) return rc_; } while (0)

extern "C" int vc2hip_set_streams(vc2hip_ctx *c, int k) {
  if (!c || k < 1 || k > 16) return set_err(c, VC2HIP_EINVAL);
  ENTER(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (vc2hip_ctx *l : c->lanes) if (l != c) vc2hip_destroy(l);
  c->lanes.clear();
  c->lane_use.clear();
  for (hipEvent_t e : c->join_ev) (void)hipEventDestroy(e);
  c->join_ev.clear();
  if (k == 1) return VC2HIP_OK;
  if (!c->fork_ev) HIPCHK(c, hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
  for (int i = 0; i < k; ++i) {
    vc2hip_ctx *l = c;
    if (i > 0) {
      const int rc = vc2hip_create_with_flags(c->device, c->flags, &l);
      if (rc) return set_err(c, rc);
      l->L.on = c->L.on;
      l->follows_caller = c->follows_caller;
    }
    c->lanes.push_back(l);
    hipEvent_t e;
    HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->join_ev.push_back(e);
  }
  c->lane_use.assign((size_t)k, vc2hip_ctx::LaneUse());
  return VC2HIP_OK;
}

// One caller buffer of a device batch call.  An item is a picture, or a frame for the two field calls: a frame takes two
// payload slots and two lengths, and that factor of two is in `each` and nowhere else.
static void inherit_matrix(vc2hip_ctx *child, const vc2hip_ctx *c); // (vc2hip_set_quant_matrix, below)
struct BatchBuf {
  const void *p; // null where the call allows it: it has no range then, and a lane's pointer stays null
  size_t each;   // bytes per item
  bool written;
};

// Run fn(lane, item count, the buffers' pointers at the lane's first item) for contiguous sub-batches of the n items on the
// lanes' streams: lane i takes n / k + (i < n % k) of them.  A lane waits for the context's stream (fork) and for every
// other lane whose previous sub-batch touched what it is about to touch (the buffers' ranges: read against written, written
// against both); consecutive calls with the same partition (encode -> decode of the same batch) therefore chain lane by
// lane without a barrier.  The context's stream joins the lanes lazily: at the next entry point that uses it, or at once
// when the stream belongs to the caller (vc2hip_create_on_stream).
template <size_t NB, class F> static int split_batch(vc2hip_ctx *c, int n, const BatchBuf (&bufs)[NB], F fn) {
  const int k = std::min<int>((int)c->lanes.size(), n);
  HIPCHK(c, hipSetDevice(c->device));
  // A caller's stream was joined to every lane when the call before returned, and the fork event below follows that join:
  // there is nothing left of the earlier sub-batches to wait for.  (Their join events may also have been recorded outside
  // the graph capture this call is part of, or inside one that has ended: a wait on them here would not be a graph edge.)
  if (!c->own_stream) for (vc2hip_ctx::LaneUse &u : c->lane_use) u.valid = false;
  HIPCHK(c, hipEventRecord(c->fork_ev, c->stream));
  std::vector<vc2hip_ctx::LaneUse> cur((size_t)c->lanes.size());
  std::vector<int> first((size_t)k), count((size_t)k);
  typedef std::vector<vc2hip_ctx::Range> Ranges;
  auto overlap = [](const Ranges &a, const Ranges &b) {
    for (const vc2hip_ctx::Range &x : a)
      for (const vc2hip_ctx::Range &y : b)
        if (x.lo < y.hi && y.lo < x.hi) return true;
    return false;
  };
  for (int i = 0, f0 = 0; i < k; ++i) {
    count[i] = n / k + (i < n % k ? 1 : 0);
    first[i] = f0;
    f0 += count[i];
    for (const BatchBuf &b : bufs) {
      if (!b.p) continue;
      const uint8_t *lo = (const uint8_t *)b.p + (size_t)first[i] * b.each;
      (b.written ? cur[i].w : cur[i].r).push_back({lo, lo + (size_t)count[i] * b.each});
    }
    cur[i].valid = true;
  }
  for (int i = 0; i < k; ++i) { // all waits before any join event is recorded again
    vc2hip_ctx *l = c->lanes[i];
    if (i > 0) HIPCHK(c, hipStreamWaitEvent(l->stream, c->fork_ev, 0));
    for (size_t j = 0; j < c->lanes.size(); ++j) {
      const vc2hip_ctx::LaneUse &p = c->lane_use[j];
      if ((int)j == i || !p.valid) continue;
      if (overlap(cur[i].r, p.w) || overlap(cur[i].w, p.w) || overlap(cur[i].w, p.r))
        HIPCHK(c, hipStreamWaitEvent(l->stream, c->join_ev[j], 0));
    }
  }
  int rc = VC2HIP_OK;
  for (int i = 0; i < k; ++i) {
    vc2hip_ctx *l = c->lanes[i];
    c->in_split = (i == 0);
    l->layout = c->layout; l->has_layout = c->has_layout; // (host state: a lane's pictures lie as the context's)
    l->packed = c->packed; l->has_packed = c->has_packed;
    if (l != c) inherit_matrix(l, c);
    void *at[NB];
    for (size_t b = 0; b < NB; ++b) at[b] = bufs[b].p ? (uint8_t *)bufs[b].p + (size_t)first[i] * bufs[b].each : nullptr;
    const int r = fn(l, count[i], at);
    c->in_split = false;
    if (r && !rc) rc = i ? set_err(c, r, l->err.c_str()) : r;
    HIPCHK(c, hipEventRecord(c->join_ev[i], l->stream));
    c->lane_use[i] = cur[i];
  }
  c->lanes_pending = true;
  if (!c->own_stream) return join_lanes(c) ? VC2HIP_EHIP : rc;
  return rc;
}
// A device batch call's work, once its front checks have passed: all n items on the context, or cut over its lanes
template <size_t NB, class F> static int run_batch(vc2hip_ctx *c, int n, const BatchBuf (&bufs)[NB], F fn) {
  if (c->lanes.size() > 1 && n > 1) return split_batch(c, n, bufs, fn);
  void *at[NB];
  for (size_t b = 0; b < NB; ++b) at[b] = (void *)bufs[b].p;
  return fn(c, n, at);
}

extern "C" int vc2hip_sync(vc2hip_ctx *c) {
  if (!c) return VC2HIP_EINVAL;
  ENTER(c);
  HIPCHK(c, hipMemcpyAsync(c->h_err, c->d_err, VC2_ERRBLK_COPY, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_err, 0, sizeof(unsigned), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->L.collect();
  int lane_rc = VC2HIP_OK;
  for (vc2hip_ctx *l : c->lanes) { // their work was joined into c->stream; surface their error flags too
    if (l == c) continue;
    const int r = vc2hip_sync(l);
    if (r && !lane_rc) lane_rc = set_err(c, r, l->err.c_str());
  }
  if (!c->L.launch_error.empty()) {
    const std::string m = c->L.launch_error;
    c->L.launch_error.clear();
    return set_err(c, VC2HIP_EHIP, m.c_str());
  }
  const int rc = err_from_flags(c, *c->h_err);
  return rc ? rc : lane_rc;
}

static int need(vc2hip_ctx *c, int which, size_t bytes, void **out) {
  Buf &b = c->buf[which];
  if (b.cap < bytes) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (b.p) HIPCHK(c, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    // Large workspaces are sized in whole 2 MiB units (the driver's large page-table fragments; no measurable effect on
    // the kernels: the 10 % spread of the level-0 transforms between processes that prompted it follows the box and the
    // moment, not the allocation -- see VC2_STREAM_WG_WAVES in vc2hip_dwt_stream.hip).
    size_t cap = bytes >= (1u << 21) ? (bytes + (1u << 21) - 1) & ~(size_t)((1u << 21) - 1) : (bytes + 4095) & ~(size_t)4095;
    { static const size_t unit = (size_t)vc2_tune_int("VC2HIP_ALLOC_ROUND_MB", 0) << 20; // (ablation build: another unit)
      if (unit && bytes >= (1u << 21)) cap = (bytes + unit - 1) / unit * unit; }
    HIPCHK(c, hipMalloc(&b.p, cap));
    b.cap = cap;
#ifdef VC2HIP_ABLATE
    if (getenv("VC2HIP_DEBUG_ALLOC")) fprintf(stderr, "vc2hip alloc: buffer %d at %p, %zu bytes\n", which, b.p, cap);
#endif
  }
  *out = b.p;
  return VC2HIP_OK;
}
#define NEED(ctx, which, bytes, ptr)                                   \
  do {                                                                 \
    void *p_;                                                          \
    int rc_ = need(ctx, which, bytes, &p_);                            \
    if (rc_) return rc_;                                               \
    ptr = (decltype(ptr))p_;                                           \
  } while (0)

// ---- profiling ---------------------------------------------------------------------------------
extern "C" int vc2hip_profile_enable(vc2hip_ctx *c, int on) {
  if (!c) return VC2HIP_EINVAL;
  c->L.on = on != 0;
  for (vc2hip_ctx *l : c->lanes) l->L.on = on != 0;
  return 0;
}
extern "C" int vc2hip_profile_only(vc2hip_ctx *c, const char *name) {
  if (!c) return VC2HIP_EINVAL;
  c->L.only = name ? name : "";
  for (vc2hip_ctx *l : c->lanes) l->L.only = c->L.only;
  return 0;
}
// entries of the context and of its lanes, merged by kernel name
extern "C" int vc2hip_profile_count(vc2hip_ctx *c) {
  if (!c) return 0;
  c->merged = c->L.entries;
  for (vc2hip_ctx *l : c->lanes)
    if (l != c) for (const ProfEntry &e : l->L.entries) {
      bool found = false;
      for (ProfEntry &m : c->merged) if (m.name == e.name) { m.launches += e.launches; m.ms += e.ms; found = true; break; }
      if (!found) c->merged.push_back(e);
    }
  return (int)c->merged.size();
}
extern "C" int vc2hip_profile_get(vc2hip_ctx *c, int i, const char **name, int *launches, double *total_ms) {
  if (!c || i < 0 || i >= (int)c->merged.size()) return VC2HIP_EINVAL;
  if (name) *name = c->merged[i].name.c_str();
  if (launches) *launches = c->merged[i].launches;
  if (total_ms) *total_ms = c->merged[i].ms;
  return 0;
}
extern "C" int vc2hip_profile_reset(vc2hip_ctx *c) {
  if (!c) return VC2HIP_EINVAL;
  c->L.collect(); c->L.entries.clear(); c->merged.clear();
  for (vc2hip_ctx *l : c->lanes) if (l != c) { l->L.collect(); l->L.entries.clear(); }
  return 0;
}

// ------------------------------------------------------------------------------------------
// geometry
// ------------------------------------------------------------------------------------------
static int make_geom(Geom &g, const int ph[3], const int pw[3], const int h[3], const int w[3], int depth,
                     int ys, int xs) {
  if (depth < 1 || depth > VC2_MAX_DEPTH || ys < 1 || xs < 1) return VC2HIP_EINVAL;
  g.depth = depth; g.ys = ys; g.xs = xs;
  int off = 0;
  for (int c = 0; c < 3; ++c) {
    CompGeom &cg = g.c[c];
    cg.h = h[c]; cg.w = w[c]; cg.ph = ph[c]; cg.pw = pw[c];
    if (ph[c] == 0 || pw[c] == 0) { cg.sh = cg.sw = cg.n0 = 0; cg.coef_off = off; continue; }
    if (ph[c] % ys || pw[c] % xs) return VC2HIP_EINVAL;
    cg.sh = ph[c] / ys; cg.sw = pw[c] / xs;
    if (cg.sh % (1 << depth) || cg.sw % (1 << depth)) return VC2HIP_EINVAL;
    cg.n0 = (cg.sh >> depth) * (cg.sw >> depth);
    cg.coef_off = off;
    off += cg.sh * cg.sw;
  }
  g.slice_coefs = off;
  return VC2HIP_OK;
}

static void chroma_dims(int h, int w, int cf, int *ch, int *cw) {
  *ch = cf == VC2HIP_CF420 ? h / 2 : h;
  *cw = cf == VC2HIP_CF444 ? w : w / 2;
}

// encoder-side picture geometry (WaveletTransform.cpp:1267-1273) or decoder-side
// (DecodeStream.cpp:483-498: chroma derived from the padded luma size)
static int picture_geom(Geom &g, const vc2hip_picture_format *f, const vc2hip_coding_params *cp, bool decoder) {
  if (!f || !cp || f->width < 1 || f->height < 1 || f->word_bytes < 1 || f->word_bytes > 4 ||
      f->bit_depth < 1 || f->bit_depth > 8 * f->word_bytes || f->chroma_format < 0 || f->chroma_format > 2 ||
      f->chroma_bit_depth < 0 || f->chroma_bit_depth > 8 * f->word_bytes)
    return VC2HIP_EINVAL;
  int ch, cw;
  chroma_dims(f->height, f->width, f->chroma_format, &ch, &cw);
  int h[3] = {f->height, ch, ch}, w[3] = {f->width, cw, cw}, ph[3], pw[3];
  ph[0] = vc2hip_padded_size(f->height, cp->depth);
  pw[0] = vc2hip_padded_size(f->width, cp->depth);
  if (decoder) chroma_dims(ph[0], pw[0], f->chroma_format, &ph[1], &pw[1]);
  else { ph[1] = vc2hip_padded_size(ch, cp->depth); pw[1] = vc2hip_padded_size(cw, cp->depth); }
  ph[2] = ph[1]; pw[2] = pw[1];
  return make_geom(g, ph, pw, h, w, cp->depth, cp->y_slices, cp->x_slices);
}

extern "C" size_t vc2hip_raw_picture_bytes(const vc2hip_picture_format *f) {
  int ch, cw;
  chroma_dims(f->height, f->width, f->chroma_format, &ch, &cw);
  return ((size_t)f->height * f->width + 2 * (size_t)ch * cw) * f->word_bytes;
}

// ------------------------------------------------------------------------------------------
// the caller's sample layout (vc2hip_set_sample_layout)
// ------------------------------------------------------------------------------------------
// A layout resolved against the pictures of one buffer: every 0 of the struct replaced by what it stands for.
struct RawLayout {
  int le, lsb;
  size_t pitch[3], at[3]; // bytes from row to row; from a picture's base to the plane
  size_t extent;          // from a picture's base to the end of its furthest plane row
  size_t stride;          // from one picture's base to the next
};
// what the struct alone shows (the setter's check); null: the file format
static const char *layout_struct_error(const vc2hip_sample_layout *l) {
  if (!l) return nullptr;
  if ((l->little_endian != 0 && l->little_endian != 1) || (l->lsb_justified != 0 && l->lsb_justified != 1))
    return "sample layout: little_endian and lsb_justified must be 0 or 1";
  size_t any = l->picture_stride;
  for (int k = 0; k < 3; ++k) any |= l->pitch[k] | l->plane_offset[k];
  if (any & 15) return "sample layout: pitches, plane offsets and the picture stride must be multiples of 16 bytes";
  return nullptr;
}
// The 32-bit row offsets of the edge kernels (mul24z(y, pitch / 2) * 2, __umul24(y, pitch / 2) + column: 24-bit factors, a
// 32-bit sum of 16-bit words) carry a plane whose rows lie below 2^23 bytes apart and whose extent stays below 2^31 bytes.
#define VC2_LAYOUT_MAX_PITCH ((size_t)1 << 23)
#define VC2_LAYOUT_MAX_PLANE ((size_t)1 << 31)
// f: the format of the buffer's pictures (frames for the field calls, the reduced pictures for the reduced call).
// l null: the file format, never refused.  Returns null, or why the calls refuse the layout for these pictures.
static const char *resolve_layout(const vc2hip_picture_format *f, const vc2hip_sample_layout *l, RawLayout &r) {
  int ch, cw;
  chroma_dims(f->height, f->width, f->chroma_format, &ch, &cw);
  const size_t row[3] = {(size_t)f->width * f->word_bytes, (size_t)cw * f->word_bytes, (size_t)cw * f->word_bytes};
  const size_t rows[3] = {(size_t)f->height, (size_t)ch, (size_t)ch};
  if (const char *e = layout_struct_error(l)) return e;
  r.le = l ? l->little_endian : 0;
  r.lsb = l ? l->lsb_justified : 0;
  const bool placed = l && (l->plane_offset[0] | l->plane_offset[1] | l->plane_offset[2]);
  const bool custom = l && (placed || l->little_endian || l->lsb_justified || l->picture_stride || l->pitch[0] || l->pitch[1] || l->pitch[2]);
  r.extent = 0;
  for (int k = 0; k < 3; ++k) {
    r.pitch[k] = l && l->pitch[k] ? l->pitch[k] : row[k];
    if (r.pitch[k] < row[k]) return "sample layout: a pitch below the component's row bytes";
    if (custom && (r.pitch[k] >= VC2_LAYOUT_MAX_PITCH || rows[k] * r.pitch[k] >= VC2_LAYOUT_MAX_PLANE))
      return "sample layout: a plane beyond the kernels' 32-bit row offsets (pitch below 2^23 bytes, rows * pitch below 2^31)";
    r.at[k] = placed ? l->plane_offset[k] : k ? r.at[k - 1] + rows[k - 1] * r.pitch[k - 1] : 0;
    const size_t end = rows[k] ? r.at[k] + (rows[k] - 1) * r.pitch[k] + row[k] : r.at[k];
    if (end > r.extent) r.extent = end;
  }
  r.stride = l && l->picture_stride ? l->picture_stride : r.extent;
  if (r.stride < r.extent) return "sample layout: a picture stride below vc2hip_layout_picture_bytes";
  return nullptr;
}
static bool format_ok(const vc2hip_picture_format *f) {
  return f && f->width >= 1 && f->height >= 1 && f->word_bytes >= 1 && f->word_bytes <= 4 && f->chroma_format >= 0 && f->chroma_format <= 2;
}
// the layout of the context's device batch calls: null = the file format
static const vc2hip_sample_layout *active_layout(const vc2hip_ctx *c) { return c->has_layout && !c->layout_bypass ? &c->layout : nullptr; }

// Packed and semi-planar pictures (vc2hip_set_packed_format), resolved against the pictures of a buffer.
// Plane 0: the v210 rows / the Y plane; plane 1: the UV plane (SEMIPLANAR only).
struct PackedLayout {
  int packing, le, lsb;
  int rows[2];
  size_t row[2], pitch[2], at[2]; // bytes of a row; from row to row; from a picture's base to the plane
  size_t extent, stride;
};
static const char *packed_struct_error(const vc2hip_packed_format *p) {
  if (!p || p->packing == VC2HIP_PACKING_NONE) return nullptr;
  if (p->packing != VC2HIP_PACKING_V210 && p->packing != VC2HIP_PACKING_SEMIPLANAR) return "packed format: unknown packing";
  if ((p->little_endian != 0 && p->little_endian != 1) || (p->lsb_justified != 0 && p->lsb_justified != 1))
    return "packed format: little_endian and lsb_justified must be 0 or 1";
  if (p->packing == VC2HIP_PACKING_V210 && (p->little_endian || p->lsb_justified || p->pitch[1] || p->plane_offset[0] || p->plane_offset[1]))
    return "packed format: v210 fixes byte order and justification and has one plane (those fields must be 0)";
  if ((p->pitch[0] | p->pitch[1] | p->plane_offset[0] | p->plane_offset[1] | p->picture_stride) & 15)
    return "packed format: pitches, plane offsets and the picture stride must be multiples of 16 bytes";
  return nullptr;
}
// f: the format of the buffer's pictures (frames for the field calls, the reduced pictures for the reduced call)
static const char *resolve_packed(const vc2hip_picture_format *f, const vc2hip_packed_format *p, PackedLayout &r) {
  if (!p || p->packing == VC2HIP_PACKING_NONE) return "packed format: none";
  if (const char *e = packed_struct_error(p)) return e;
  int ch, cw;
  chroma_dims(f->height, f->width, f->chroma_format, &ch, &cw);
  memset(&r, 0, sizeof r);
  r.packing = p->packing; r.le = p->little_endian; r.lsb = p->lsb_justified;
  int planes;
  if (p->packing == VC2HIP_PACKING_V210) {
    if (f->chroma_format != VC2HIP_CF422 || f->bit_depth != 10 || (f->chroma_bit_depth != 0 && f->chroma_bit_depth != 10) ||
        f->word_bytes != 2 || f->width % 2)
      return "packed format: v210 needs 4:2:2, bit_depth 10, chroma_bit_depth 0 or 10, word_bytes 2 and an even width";
    planes = 1;
    r.rows[0] = f->height; r.row[0] = (size_t)((f->width + 5) / 6) * 16;
  } else {
    if (f->word_bytes != 1 && f->word_bytes != 2) return "packed format: semi-planar pictures have word_bytes 1 or 2";
    planes = 2;
    r.rows[0] = f->height; r.row[0] = (size_t)f->width * f->word_bytes;
    r.rows[1] = ch; r.row[1] = 2 * (size_t)cw * f->word_bytes;
  }
  const bool placed = (p->plane_offset[0] | p->plane_offset[1]) != 0;
  for (int k = 0; k < planes; ++k) {
    r.pitch[k] = p->pitch[k] ? p->pitch[k] : r.row[k];
    if (r.pitch[k] < r.row[k]) return "packed format: a pitch below the row's bytes";
    if (r.pitch[k] >= VC2_LAYOUT_MAX_PITCH || (size_t)r.rows[k] * r.pitch[k] >= VC2_LAYOUT_MAX_PLANE)
      return "packed format: a plane beyond the kernels' 32-bit row offsets (pitch below 2^23 bytes, rows * pitch below 2^31)";
    r.at[k] = placed ? p->plane_offset[k] : k ? r.at[0] + (size_t)r.rows[0] * r.pitch[0] : 0;
    const size_t end = r.rows[k] ? r.at[k] + (size_t)(r.rows[k] - 1) * r.pitch[k] + r.row[k] : r.at[k];
    if (end > r.extent) r.extent = end;
  }
  r.stride = p->picture_stride ? p->picture_stride : r.extent;
  if (r.stride < r.extent) return "packed format: a picture stride below vc2hip_packed_picture_bytes";
  return nullptr;
}
static const vc2hip_packed_format *active_packed(const vc2hip_ctx *c) { return c->has_packed && !c->layout_bypass ? &c->packed : nullptr; }

extern "C" int vc2hip_set_packed_format(vc2hip_ctx *c, const vc2hip_packed_format *p) {
  if (!c) return VC2HIP_EINVAL;
  if (const char *e = packed_struct_error(p)) return set_err(c, VC2HIP_EINVAL, e);
  c->has_packed = p && p->packing != VC2HIP_PACKING_NONE;
  if (c->has_packed) c->packed = *p;
  return VC2HIP_OK;
}
extern "C" size_t vc2hip_packed_picture_bytes(const vc2hip_picture_format *f, const vc2hip_packed_format *p) {
  PackedLayout r;
  if (!format_ok(f) || resolve_packed(f, p, r)) return 0;
  return r.extent;
}

// ... resolved for a buffer of pictures of format f; VC2HIP_EINVAL (nothing launched) where the check needs the format.
// Under a packed format: that format's extent and stride (the planes are the staging's: raw_view)
static int batch_layout(vc2hip_ctx *c, const vc2hip_picture_format *f, RawLayout &r) {
  if (!format_ok(f)) return set_err(c, VC2HIP_EINVAL);
  if (const vc2hip_packed_format *pf = active_packed(c)) {
    PackedLayout pl;
    if (const char *e = resolve_packed(f, pf, pl)) return set_err(c, VC2HIP_EINVAL, e);
    // (lanes cut the batch at the picture stride and every lane's base keeps the 16-byte rule)
    if ((pl.stride & 15) && c->lanes.size() > 1)
      return set_err(c, VC2HIP_EINVAL, "packed format: with vc2hip_set_streams(k > 1) the picture stride must be a multiple of 16 bytes");
    memset(&r, 0, sizeof r);
    r.le = pl.le; r.lsb = pl.lsb; r.extent = pl.extent; r.stride = pl.stride;
    return VC2HIP_OK;
  }
  if (const char *e = resolve_layout(f, active_layout(c), r)) return set_err(c, VC2HIP_EINVAL, e);
  return VC2HIP_OK;
}

extern "C" int vc2hip_set_sample_layout(vc2hip_ctx *c, const vc2hip_sample_layout *l) {
  if (!c) return VC2HIP_EINVAL;
  if (const char *e = layout_struct_error(l)) return set_err(c, VC2HIP_EINVAL, e);
  bool any = false;
  if (l) {
    any = l->little_endian || l->lsb_justified || l->picture_stride;
    for (int k = 0; k < 3; ++k) any = any || l->pitch[k] || l->plane_offset[k];
  }
  c->has_layout = any; // (an all-zero layout is the file format)
  if (any) c->layout = *l;
  return VC2HIP_OK;
}
extern "C" size_t vc2hip_layout_picture_bytes(const vc2hip_picture_format *f, const vc2hip_sample_layout *l) {
  RawLayout r;
  if (!format_ok(f) || resolve_layout(f, l, r)) return 0;
  return r.extent;
}
struct LayoutBypass { // a host-buffer picture call: its pictures are in the file format whatever the context's layout
  vc2hip_ctx *c; bool was;
  explicit LayoutBypass(vc2hip_ctx *ctx) : c(ctx), was(ctx->layout_bypass) { c->layout_bypass = true; }
  ~LayoutBypass() { c->layout_bypass = was; }
};

// ---- the context's quantisation matrix (vc2hip_set_quant_matrix) ----------------------------------
// Host state only.  Every kernel takes its matrix by value in its parameters (the qmatrix member of the params structs), so
// a captured call keeps the one it was captured with; the one device-side copy, plane_inverse's, is keyed by its entries.
extern "C" int vc2hip_set_quant_matrix(vc2hip_ctx *c, const int32_t *m, int depth) {
  if (!c) return VC2HIP_EINVAL;
  if (!m) { c->qm_depth = 0; return VC2HIP_OK; }
  if (depth < 1 || depth > VC2_MAX_DEPTH) return set_err(c, VC2HIP_EINVAL, "set_quant_matrix: depth must be 1 ... 7");
  for (int b = 0; b < 3 * depth + 1; ++b)
    if (m[b] < 0 || m[b] > 255) return set_err(c, VC2HIP_EINVAL, "set_quant_matrix: every entry must be 0 ... 255");
  memcpy(c->qm, m, (size_t)(3 * depth + 1) * 4);
  c->qm_depth = depth;
  return VC2HIP_OK;
}
extern "C" int vc2hip_get_quant_matrix(const vc2hip_ctx *c, int32_t *out, int cap) {
  if (!c || cap < 0 || (cap && !out)) return VC2HIP_EINVAL;
  const int n = c->qm_depth ? 3 * c->qm_depth + 1 : 0;
  for (int b = 0; b < n && b < cap; ++b) out[b] = c->qm[b];
  return n;
}
// The one owner: the matrix a call of context c with coding parameters cp quantises by -- the context's while one is set
// (cp->depth must be its depth), else the default of cp's wavelet and depth.  qm: VC2_MAX_BANDS entries.  Its refusal is
// matrix_depth_check, which the entry points make before they launch anything (batch_args, the fronts of the picture and
// stream calls); a context with no matrix set is refused nothing it was not refused before.
static int matrix_depth_check(vc2hip_ctx *c, const vc2hip_coding_params *cp) {
  if (c->qm_depth && cp->depth != c->qm_depth)
    return set_err(c, VC2HIP_EINVAL, "the context's quantisation matrix is for another transform depth than cp->depth");
  return VC2HIP_OK;
}
static int effective_matrix(vc2hip_ctx *c, const vc2hip_coding_params *cp, int32_t *qm) {
  if (int rc = matrix_depth_check(c, cp)) return rc;
  if (c->qm_depth) { memcpy(qm, c->qm, (size_t)(3 * c->qm_depth + 1) * 4); return VC2HIP_OK; }
  const int rc = cp->depth > VC2_MAX_DEPTH ? VC2HIP_EINVAL : vc2hip_quant_matrix(cp->kernel, cp->depth, qm);
  return rc ? set_err(c, rc) : VC2HIP_OK;
}
// a child context (a vc2hip_set_streams lane, a picture in flight) codes with its parent's matrix at the time of the call
static void inherit_matrix(vc2hip_ctx *child, const vc2hip_ctx *c) {
  child->qm_depth = c->qm_depth;
  memcpy(child->qm, c->qm, sizeof c->qm);
}

static size_t max_slice_bytes(int prefix, int scalar) { return (size_t)prefix + 4 + 3 * 255 * (size_t)scalar; }
extern "C" size_t vc2hip_max_payload_bytes(const vc2hip_picture_format *f, const vc2hip_coding_params *cp) {
  (void)f;
  const size_t n = (size_t)cp->y_slices * cp->x_slices;
  if (cp->mode == VC2HIP_HQ_CONSTQ || cp->mode == VC2HIP_HQ_CAPPED || cp->mode == VC2HIP_HQ_CAPPED_FILL) return n * max_slice_bytes(cp->prefix, cp->scalar);
  if (cp->mode == VC2HIP_HQ_CBR) return (size_t)cp->compressed_bytes + n * (cp->prefix + (size_t)cp->scalar + 4);
  return (size_t)cp->compressed_bytes + n;
}

// ------------------------------------------------------------------------------------------
// level sequencing
// ------------------------------------------------------------------------------------------
struct LLPlanes { // per level l >= 1: compact LL_l planes for the three components
  void *p[VC2_MAX_DEPTH + 1][3];    // int32_t elements, or int16_t with ...
  int32_t *w[VC2_MAX_DEPTH + 1][3]; // ... their wide planes (vc2hip_store.h); null for int32 planes
  long long stride[VC2_MAX_DEPTH + 1][3];
};

// planes start on 16-byte boundaries whatever the element size: sizes are rounded up to 8 elements
static size_t ll_elems(const Geom &g, int n) {
  size_t e = 0;
  for (int l = 1; l <= g.depth; ++l)
    for (int c = 0; c < 3; ++c) e += (((size_t)(g.c[c].ph >> l) * (g.c[c].pw >> l) * n + 7) & ~(size_t)7);
  return e;
}
static size_t ll_bytes(const Geom &g, int n) { return ll_elems(g, n) * sizeof(int32_t); }
static void ll_layout(const Geom &g, int n, void *base, int elem_bytes, int32_t *wide, LLPlanes &ll) {
  size_t off = 0;
  memset(&ll, 0, sizeof ll);
  for (int l = 1; l <= g.depth; ++l)
    for (int c = 0; c < 3; ++c) {
      const size_t e = (size_t)(g.c[c].ph >> l) * (g.c[c].pw >> l);
      ll.p[l][c] = (char *)base + off * elem_bytes;
      ll.w[l][c] = wide ? wide + off : nullptr;
      ll.stride[l][c] = (long long)e;
      off += (e * n + 7) & ~(size_t)7;
    }
}
static void ll_layout(const Geom &g, int n, int32_t *base, LLPlanes &ll) { ll_layout(g, n, base, 4, nullptr, ll); }

// A coefficient store of n pictures, as the transforms, the slice coders and the slice readers are handed it
struct Store {
  void *p;          // int32_t elements, or int16_t (s16) with ...
  int32_t *wide;    // ... their wide elements (vc2hip_store.h); null for an int32 store
  bool s16;
  long long stride; // elements per picture: the slice records (record_stride), on the decoding side band planes and record heads behind them
};
static long long record_stride(const Geom &g) { return (long long)g.ys * g.xs * g.slice_coefs; }
static Store records32(const Geom &g, int32_t *p) { return Store{p, nullptr, false, record_stride(g)}; } // (the fine-grained int32 calls)
// The per-slice byte budgets of HQ_CBR and LD pictures on the device (budget_tables): one picture's worth, shared by the batch
struct Budgets {
  const int32_t *bytes; // per slice; null: no budgets (VBR)
  const uint32_t *offs; // per slice: where it starts in the picture's payload
  uint64_t total;       // the picture's payload bytes
};

// vc2hip_dwt_launches: one entry per transform launch, on the host where it is issued
static void record_dwt(vc2hip_ctx *c, bool inverse, int level, int levels, int family, bool edge, bool s16, int segments, int tail,
                       bool small_gather, int n, int band_planes = 0) {
  if (c->dwt_rec_stale) { c->dwt_rec.clear(); c->dwt_rec_stale = false; }
  vc2hip_dwt_launch r;
  r.inverse = inverse; r.level = level; r.levels = levels; r.family = family; r.edge = edge; r.store_bits = s16 ? 16 : 32;
  r.segments = segments; r.tail = tail; r.small_gather = small_gather; r.pictures = n; r.band_planes = band_planes;
  c->dwt_rec.push_back(r);
}

// the band planes an inverse level reads its bands from: 0 (the slice records), 16 or 8 (BandPlanes::bytes8)
static int band_plane_bits(const LevelParams &p) {
  for (int k = 0; k < 3; ++k) if (p.bp_base[k] >= 0) return p.bp8 ? 8 : 16;
  return 0;
}

static void fill_level(LevelParams &p, const Geom &g, int level, int kernel, const int32_t *qm) {
  const int D = g.depth, Lv = D - level;
  p.band = 3 * (Lv - 1) + 1;
  p.ys = g.ys; p.xs = g.xs; p.slice_coefs = g.slice_coefs;
  const int hx = vc2_halo_x(kernel), hy = vc2_halo_y(kernel);
  for (int c = 0; c < 3; ++c) {
    const CompGeom &cg = g.c[c];
    p.in_h[c] = cg.ph >> level; p.in_w[c] = cg.pw >> level;
    p.pic_h[c] = cg.h; p.pic_w[c] = cg.w;
    p.coef_off[c] = cg.coef_off;
    p.rec_stride[c] = g.slice_coefs;
    if (cg.ph == 0) { p.tiles_x[c] = p.tiles_y[c] = 0; p.fh[c] = p.fw[c] = 2; p.tsy[c] = p.tsx[c] = 1; continue; }
    p.fh[c] = cg.sh >> level; p.fw[c] = cg.sw >> level;
    // tile 32 x 128 samples, whole slices, power-of-two slice counts, LDS <= 64 KiB
    int tsy = 1, tsx = 1;
    while (tsy * 2 * p.fh[c] <= 64 && tsy * 2 <= g.ys) tsy *= 2;
    while (tsx * 2 * p.fw[c] <= 128 && tsx * 2 <= g.xs) tsx *= 2;
    while ((size_t)(tsy * p.fh[c] + 2 * hy) * (tsx * p.fw[c] + 2 * hx) * 4 > 150 * 1024) {
      if (tsx > 1) tsx /= 2; else if (tsy > 1) tsy /= 2; else break;
    }
    p.tsy[c] = tsy; p.tsx[c] = tsx;
    p.tiles_y[c] = (g.ys + tsy - 1) / tsy;
    p.tiles_x[c] = (g.xs + tsx - 1) / tsx;
    p.band_n[c] = (p.fh[c] / 2) * (p.fw[c] / 2);
    p.band_off[c] = p.band_n[c]; // == n0 * 4^(Lv-1): HL at 1x, LH at 2x, HH at 3x
  }
  for (int b = 0; b < 3 * D + 1; ++b) p.qmatrix[b] = qm ? qm[b] : 0;
}

// forward transform of n pictures: raw words (first level fused) or int32 LL_0 planes (src_l: stride only) -> store
// st.s16: 16-bit store and level planes with their wide planes (only with the fast kernels: use_store16)
static int run_forward(vc2hip_ctx *c, const Geom &g, int kernel, int n, const void *const src[3],
                       const RawPlane src_l[3], bool src_raw, const vc2hip_picture_format *f,
                       const Store &st, const LLPlanes &ll) {
  const bool s16 = st.s16;
  auto level_params = [&](LevelParams &p, int level) {
    memset(&p, 0, sizeof p);
    fill_level(p, g, level, kernel, nullptr);
    p.store = st.p; p.store_stride = st.stride;
    p.store_wide = st.wide;
    p.err = c->d_err;
    p.ll_to_store = (level == g.depth - 1);
    const bool first = (level == 0) && src_raw;
    for (int k = 0; k < 3; ++k) {
      if (level == 0) { p.plane[k] = (void *)src[k]; p.plane_stride[k] = src_l[k].stride; }
      else { p.plane[k] = ll.p[level][k]; p.plane_wide[k] = ll.w[level][k]; p.plane_stride[k] = ll.stride[level][k]; }
      p.ll[k] = ll.p[level + 1][k]; p.ll_wide[k] = ll.w[level + 1][k]; p.ll_stride[k] = ll.stride[level + 1][k];
    }
    if (first) {
      for (int k = 0; k < 3; ++k) { p.raw_pitch[k] = src_l[k].pitch; p.field_step[k] = src_l[k].field_step; }
      p.field_shift = src_l[0].field_shift;
      p.word_bytes = f->word_bytes;
      const int lsb = src_l[0].lsb; // the caller's sample layout (raw_planes): LSB-justified words need no shift
      p.sample_shift = lsb ? 0 : 8 * f->word_bytes - f->bit_depth;
      p.sample_offset = 1 << (f->bit_depth - 1);
      const int cd = f->chroma_bit_depth ? f->chroma_bit_depth : f->bit_depth;
      p.sample_shift_c = lsb ? 0 : 8 * f->word_bytes - cd;
      p.sample_offset_c = 1 << (cd - 1);
      p.sample_bits = f->bit_depth; p.sample_bits_c = cd;
      p.sample_mask = f->bit_depth < 32 ? (1u << f->bit_depth) - 1 : ~0u;
      p.sample_mask_c = cd < 32 ? (1u << cd) - 1 : ~0u;
      p.sample_le = src_l[0].le;
      p.perm_rd = src_l[0].le ? VC2_PERM_RD_LE : VC2_PERM_RD_BE;
    }
  };
  for (int level = 0; level < g.depth; ++level) {
    LevelParams p;
    level_params(p, level);
    const bool first = (level == 0) && src_raw;
    // two levels in one launch (vc2hip_dwt_pair.hip): level + 1's input plane is never written
    if (!c->force_generic && c->allow_stream && c->allow_pair && level + 1 < g.depth) {
      PairParams pp;
      memset(&pp, 0, sizeof pp);
      pp.a = p;
      pp.a.debug_skip = c->debug_skip;
      level_params(pp.b, level + 1);
      const size_t lds = vc2_pair_applicable(pp, kernel, first, false, s16, n);
      if (lds) {
        int rc = vc2_launch_forward_pair(c->L, kernel, first, pp, n, s16, lds, c->stream);
        if (rc) return set_err(c, rc, "invalid wavelet kernel");
        record_dwt(c, false, level, 2, VC2HIP_DWT_PAIR, first, s16, pp.a.st_segmax, 0, false, n);
        ++level;
        continue;
      }
    }
    LevelParams pf = p;
    pf.debug_skip = c->debug_skip;
    if (!c->force_generic && c->allow_stream) {
      LevelParams ps = p;
      const size_t lds = vc2_stream_level_applicable(ps, kernel, first, false, s16, n);
      if (lds) {
        int rc = vc2_launch_forward_stream(c->L, kernel, first, ps, n, s16, lds, c->stream);
        if (rc) return set_err(c, rc, "invalid wavelet kernel");
        record_dwt(c, false, level, 1, VC2HIP_DWT_STREAM, first, s16, ps.st_segmax, ps.st_tail, false, n);
        continue;
      }
    }
    if (!c->force_generic && vc2_fast_level_applicable(pf)) {
      int rc = vc2_launch_forward_fast(c->L, kernel, first, pf, n, s16, c->stream);
      if (rc) return set_err(c, rc, "invalid wavelet kernel");
      record_dwt(c, false, level, 1, VC2HIP_DWT_FAST, first, s16, 0, 0, false, n);
      continue;
    }
    if (s16) return set_err(c, VC2HIP_EINVAL, "internal: 16-bit store without the fast level kernels");
    if (vc2_level_lds_bytes(kernel, p) > 160 * 1024) return set_err(c, VC2HIP_EINVAL, "slice too large for one LDS tile");
    int rc = vc2_launch_forward_level(c->L, kernel, first, p, n, c->stream);
    if (rc) return set_err(c, rc, "invalid wavelet kernel");
    record_dwt(c, false, level, 1, VC2HIP_DWT_TILE, first, false, 0, 0, false, n);
  }
  return VC2HIP_OK;
}

// inverse transform of n pictures: store (optionally dequantised on load) -> int32 planes or raw words
struct InverseJob {
  Store store;                    // (a dry run looks at s16 and the stride only)
  const int32_t *qidx = nullptr;  // with qm: dequantise on load (null: the store holds coefficients)
  const int32_t *qm = nullptr;
  bool ll_ready = false;          // LD: the deepest LL planes are reconstructed already (ld_restore_ll), not read from the store
  const BandPlanes *bp = nullptr; // the decoder's band planes: levels < bp->levels read their bands from them (the store stride then includes them)
  const HeadSplit *hs = nullptr;  // the record heads, read by the levels from head_level on
  int head_level = 1 << 30;
  // reduced pictures (decode_batch_common): g is the picture the kept levels make; the launch that writes the raw words
  // normalises by norm_shift bits, and the launch record counts levels in the CODED picture
  int norm_shift = 0, level_base = 0;
  void *const *dst = nullptr;     // level 0's output planes and how they lie; f null: int32 planes, else raw words of that format
  const RawPlane *dst_l = nullptr;
  const vc2hip_picture_format *f = nullptr;
};
// What a dry run of run_inverse finds, bit l for level l: the level would go through the streaming kernel, through its TAIL
// instantiation, or -- not streaming -- through the fast tile kernel
struct InversePlan { unsigned stream, fast, tail; };
// plan != nullptr: a dry run -- nothing is launched (the planning step of the band planes and record heads asks before the
// slices are decoded).
static int run_inverse(vc2hip_ctx *c, const Geom &g, int kernel, int n, const InverseJob &job, const LLPlanes &ll, InversePlan *plan = nullptr) {
  const bool s16 = job.store.s16, dst_raw = job.f != nullptr;
  const RawPlane *const dst_l = job.dst_l;
  const vc2hip_picture_format *const f = job.f;
  const BandPlanes *const bp = job.bp;
  if (plan) *plan = InversePlan{0, 0, 0};
  auto level_params = [&](LevelParams &p, int level) {
    memset(&p, 0, sizeof p);
    fill_level(p, g, level, kernel, job.qm);
    if (job.hs && level >= job.head_level) // the deep levels' coefficients live in the record heads (HeadSplit)
      for (int k = 0; k < 3; ++k) if (g.c[k].ph) { p.rec_stride[k] = job.hs->n[k]; p.coef_off[k] = (int)job.hs->base[k]; }
    p.store = job.store.p; p.store_stride = job.store.stride;
    for (int k = 0; k < 3; ++k) p.bp_base[k] = (bp && level < bp->levels && g.c[k].ph) ? bp->base[k][level] : -1;
    p.bp8 = bp && level < bp->levels && bp->bytes8;
    p.store_wide = job.store.wide;
    p.qidx = job.qidx; p.err = c->d_err; p.dequant = job.qm != nullptr;
    p.ll_from_store = (level == g.depth - 1) && !job.ll_ready;
    const bool fin = (level == 0) && dst_raw;
    for (int k = 0; k < 3; ++k) {
      if (level == 0) { p.plane[k] = job.dst ? job.dst[k] : nullptr; p.plane_stride[k] = dst_l ? dst_l[k].stride : 0; }
      else { p.plane[k] = ll.p[level][k]; p.plane_wide[k] = ll.w[level][k]; p.plane_stride[k] = ll.stride[level][k]; }
      p.ll[k] = ll.p[level + 1][k]; p.ll_wide[k] = ll.w[level + 1][k]; p.ll_stride[k] = ll.stride[level + 1][k];
    }
    if (fin) {
      for (int k = 0; k < 3; ++k) { p.raw_pitch[k] = dst_l[k].pitch; p.field_step[k] = dst_l[k].field_step; }
      p.field_shift = dst_l[0].field_shift;
      p.word_bytes = f->word_bytes;
      p.sample_shift = dst_l[0].lsb ? 0 : 8 * f->word_bytes - f->bit_depth; // (the clip keeps a sample inside its bits: every other bit is zero)
      p.sample_offset = 1 << (f->bit_depth - 1);
      p.sample_le = dst_l[0].le;
      p.perm_wr = dst_l[0].le ? VC2_PERM_WR_LE : VC2_PERM_WR_BE;
      p.clip_lo = -(1 << (f->bit_depth - 1));
      p.clip_hi = (1 << (f->bit_depth - 1)) - 1;
      p.norm_shift = job.norm_shift;
    }
  };
  for (int level = g.depth - 1; level >= 0; --level) {
    LevelParams p;
    level_params(p, level);
    const bool fin = (level == 0) && dst_raw;
    // levels `level` and `level - 1` in one launch (vc2hip_dwt_pair.hip): the plane between them is never written
    if (!plan && !c->force_generic && c->allow_stream && c->allow_pair && level >= 1) {
      PairParams pp;
      memset(&pp, 0, sizeof pp);
      level_params(pp.a, level - 1);
      pp.b = p;
      pp.a.debug_skip = c->debug_skip;
      const bool fin_a = (level - 1 == 0) && dst_raw;
      // The pair that ends with the picture's samples keeps its two launches: measured on 32 UHD pictures, k_inv_pair over
      // levels 1 + 0 takes 0.68 ms where the two one-level kernels take 0.47 + 0.16 -- level a alone runs at four
      // wavefronts per SIMD and at the memory system's pace (0.455 ms in this kernel's frame), with level b's engine in its
      // registers it runs at two and at the pace its instruction stream issues.  The deeper pairs gain.
      static const int inv_final = vc2_tune_int("VC2HIP_PAIR_INV_FINAL", 0);
      const size_t lds = (fin_a && !inv_final) ? 0 : vc2_pair_applicable(pp, kernel, fin_a, true, s16, n);
      if (lds) {
        int rc = vc2_launch_inverse_pair(c->L, kernel, fin_a, pp, n, s16, lds, c->stream);
        if (rc) return set_err(c, rc, "invalid wavelet kernel");
        record_dwt(c, true, job.level_base + level - 1, 2, VC2HIP_DWT_PAIR, fin_a, s16, pp.a.st_segmax, 0, false, n,
                   std::max(band_plane_bits(pp.a), band_plane_bits(pp.b)));
        --level;
        continue;
      }
    }
    LevelParams pf = p;
    pf.debug_skip = c->debug_skip;
    if (!c->force_generic && c->allow_stream) {
      LevelParams ps = p;
      const size_t lds = vc2_stream_level_applicable(ps, kernel, fin, true, s16, n);
      if (lds) {
        if (plan) { plan->stream |= 1u << level; if (ps.st_tail) plan->tail |= 1u << level; continue; }
        int rc = vc2_launch_inverse_stream(c->L, kernel, fin, ps, n, s16, lds, c->stream);
        if (rc) return set_err(c, rc, "invalid wavelet kernel");
        record_dwt(c, true, job.level_base + level, 1, VC2HIP_DWT_STREAM, fin, s16, ps.st_segmax, ps.st_tail, false, n, band_plane_bits(ps));
        continue;
      }
    }
    if (plan) { if (!c->force_generic && vc2_fast_level_applicable(pf)) plan->fast |= 1u << level; continue; }
    if (bp && level < bp->levels) return set_err(c, VC2HIP_EINVAL, "internal: band planes without the streaming kernel");
    if (!c->force_generic && vc2_fast_level_applicable(pf)) {
      int rc = vc2_launch_inverse_fast(c->L, kernel, fin, pf, n, s16, c->stream);
      if (rc) return set_err(c, rc, "invalid wavelet kernel");
      record_dwt(c, true, job.level_base + level, 1, VC2HIP_DWT_FAST, fin, s16, 0, 0, vc2_fast_small_gather(pf), n, band_plane_bits(pf));
      continue;
    }
    if (s16) return set_err(c, VC2HIP_EINVAL, "internal: 16-bit store without the fast level kernels");
    if (vc2_level_lds_bytes(kernel, p) > 160 * 1024) return set_err(c, VC2HIP_EINVAL, "slice too large for one LDS tile");
    int rc = vc2_launch_inverse_level(c->L, kernel, fin, p, n, c->stream);
    if (rc) return set_err(c, rc, "invalid wavelet kernel");
    record_dwt(c, true, job.level_base + level, 1, VC2HIP_DWT_TILE, fin, false, 0, 0, false, n, band_plane_bits(p));
  }
  return VC2HIP_OK;
}

// The HQ batch path keeps the store and the level planes as 16-bit elements + wide planes (vc2hip_store.h) when every
// level runs through the fast kernels and every component record can be moved eight coefficients at a time.
static bool use_store16(const vc2hip_ctx *c, const Geom &g, int kernel) {
  if (!c->allow_store16 || c->force_generic) return false;
  for (int k = 0; k < 3; ++k) {
    if (!g.c[k].ph) continue;
    if ((g.c[k].sh * g.c[k].sw) % 8 || g.c[k].coef_off % 8) return false;
  }
  if (g.slice_coefs % 8) return false;
  for (int level = 0; level < g.depth; ++level) {
    LevelParams p;
    memset(&p, 0, sizeof p);
    fill_level(p, g, level, kernel, nullptr);
    if (!vc2_fast_level_applicable(p)) return false;
  }
  return true;
}

// A slice that does not fit the LDS tile of any level kernel (the reference admits slices up to the whole picture):
// the transform then runs on whole planes in HBM (vc2hip_dwt_plane.hip), the store is filled / read by the layout
// conversion kernels.
static bool needs_plane_path(const vc2hip_ctx *c, const Geom &g, int kernel) {
  for (int level = 0; level < g.depth; ++level) {
    LevelParams p;
    memset(&p, 0, sizeof p);
    fill_level(p, g, level, kernel, nullptr);
    LevelParams pf = p;
    if (!c->force_generic && vc2_fast_level_applicable(pf)) continue;
    if (vc2_level_lds_bytes(kernel, p) > 160 * 1024) return true;
  }
  return false;
}
static size_t plane_elems(const Geom &g) {
  size_t e = 0;
  for (int k = 0; k < 3; ++k) e += (size_t)g.c[k].ph * g.c[k].pw;
  return e;
}
// raw pictures -> store (forward), general geometry
static int plane_forward(vc2hip_ctx *c, const Geom &g, int kernel, int n, const void *const src[3], const RawPlane ss[3],
                         const vc2hip_picture_format *f, int32_t *d_store) {
  int32_t *d_plane;
  NEED(c, B_PLANE, plane_elems(g) * n * 4, d_plane);
  size_t off = 0;
  for (int k = 0; k < 3; ++k) {
    const CompGeom &cg = g.c[k];
    if (!cg.ph) continue;
    const long long ps = (long long)cg.ph * cg.pw;
    int32_t *pl = d_plane + off;
    off += (size_t)ps * n;
    vc2_launch_plane_ingest(c->L, src[k], ss[k], cg.h, cg.w, f->word_bytes, k && f->chroma_bit_depth ? f->chroma_bit_depth : f->bit_depth, pl, ps,
                            cg.ph, cg.pw, n, c->stream);
    const int rc = vc2_launch_plane_transform(c->L, kernel, pl, ps, cg.ph, cg.pw, g.depth, false, n, c->stream);
    if (rc) return set_err(c, rc, "invalid wavelet kernel");
    record_dwt(c, false, 0, g.depth, VC2HIP_DWT_PLANE, false, false, 0, 0, false, n);
    for (int p = 0; p < n; ++p)
      vc2_launch_plane_to_store(c->L, pl + (size_t)p * ps, cg.ph, cg.pw, g.depth, g.ys, g.xs,
                                d_store + (size_t)p * g.ys * g.xs * g.slice_coefs, g.slice_coefs, cg.coef_off, c->stream);
  }
  return VC2HIP_OK;
}
// store (quantised) -> raw pictures (inverse), general geometry
// ll (LD pictures): the DC-predicted LL reconstruction of every component, which replaces the plane's LL band
static int plane_inverse(vc2hip_ctx *c, const Geom &g, int kernel, int n, const int32_t *d_store, const int32_t *d_q, const int32_t *qm,
                         void *const dst[3], const RawPlane ds[3], const vc2hip_picture_format *f, const LLPlanes *ll = nullptr,
                         int norm_shift = 0, int level_base = 0) { // (the last two: as run_inverse's)
  int32_t *d_plane;
  int *d_qm;
  NEED(c, B_PLANE, plane_elems(g) * n * 4, d_plane);
  NEED(c, B_PLANE_QM, 256, d_qm);
  // the device copy is keyed by the matrix itself (a context's matrix is the caller's to change: vc2hip_set_quant_matrix):
  // uploaded when an entry in use differs, as the CBR / LD budget tables are -- no copy and no wait in any later call.  (A
  // reduced picture uses the first 3 (depth - drop) + 1 entries of the CODED picture's matrix: those are what is compared.)
  const int nb = 3 * g.depth + 1;
  if (nb != c->plane_qm_n || memcmp(qm, c->plane_qm_held, (size_t)nb * 4)) {
    c->plane_qm_n = 0;
    HIPCHK(c, hipMemcpyAsync(d_qm, qm, (size_t)nb * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // qm lives on the caller's stack
    memcpy(c->plane_qm_held, qm, (size_t)nb * 4);
    c->plane_qm_n = nb;
  }
  const int ns = g.ys * g.xs;
  size_t off = 0;
  for (int k = 0; k < 3; ++k) {
    const CompGeom &cg = g.c[k];
    if (!cg.ph) continue;
    const long long ps = (long long)cg.ph * cg.pw;
    int32_t *pl = d_plane + off;
    off += (size_t)ps * n;
    for (int p = 0; p < n; ++p)
      vc2_launch_store_to_plane(c->L, d_store + (size_t)p * ns * g.slice_coefs, g.slice_coefs, cg.coef_off, pl + (size_t)p * ps, cg.ph,
                                cg.pw, g.depth, g.ys, g.xs, d_q + (size_t)p * ns, d_qm, 1, c->d_err, c->stream);
    if (ll) vc2_launch_ll_into_plane(c->L, (const int32_t *)ll->p[g.depth][k], ll->stride[g.depth][k], cg.ph >> g.depth, cg.pw >> g.depth, pl, ps,
                                     cg.pw, g.depth, n, c->stream);
    const int rc = vc2_launch_plane_transform(c->L, kernel, pl, ps, cg.ph, cg.pw, g.depth, true, n, c->stream);
    if (rc) return set_err(c, rc, "invalid wavelet kernel");
    record_dwt(c, true, level_base, g.depth, VC2HIP_DWT_PLANE, false, false, 0, 0, false, n);
    vc2_launch_plane_emit(c->L, pl, ps, cg.pw, dst[k], ds[k], cg.h, cg.w, f->word_bytes, f->bit_depth, n, c->stream, norm_shift);
  }
  return VC2HIP_OK;
}

static void fill_comp_arrays(const Geom &g, int n[3], int off[3], int n0[3]) {
  for (int c = 0; c < 3; ++c) { n[c] = g.c[c].sh * g.c[c].sw; off[c] = g.c[c].coef_off; n0[c] = g.c[c].n0 ? g.c[c].n0 : 1; }
}

struct PackJob {
  Store store;
  const int32_t *qidx;         // n x slices
  const int32_t *qm = nullptr; // null: the store holds quantised values already (the fine-grained API)
  int prefix, scalar;
  Budgets budgets = {};        // HQ_CBR; none: VBR
  uint8_t *payload;            // the slots, their stride and their lengths
  long long stride;
  unsigned long long *lens;
};
// pack n pictures from the store into the job's payload slots; VBR goes through slots + scan + compaction
static int run_pack(vc2hip_ctx *c, const Geom &g, int n, const PackJob &job) {
  const int ns = g.ys * g.xs;
  const int prefix = job.prefix, scalar = job.scalar;
  const int32_t *const d_cbr_bytes = job.budgets.bytes;
  PackParams p;
  memset(&p, 0, sizeof p);
  p.store = job.store.p; p.store_stride = job.store.stride;
  p.store16 = job.store.s16; p.store_wide = job.store.wide;
  p.qidx = job.qidx; p.n_slices = ns; p.slice_coefs = g.slice_coefs;
  fill_comp_arrays(g, p.comp_n, p.comp_off, p.comp_n0);
  p.depth = g.depth; p.prefix = prefix; p.scalar = scalar;
  for (int b = 0; b < 3 * g.depth + 1; ++b) p.qmatrix[b] = job.qm ? job.qm[b] : 0;
  p.err = c->d_err; p.quantise = job.qm != nullptr;
  p.payload = job.payload; p.payload_stride = job.stride;
  const bool gimg = vc2_pack_image_mode(prefix, scalar) < 0; // slice images in the slots (global memory): CBR goes through slots too
  if (d_cbr_bytes && !gimg) {
    p.cbr_bytes = d_cbr_bytes; p.cbr_offsets = job.budgets.offs;
    vc2_launch_pack(c->L, p, n, c->stream);
    vc2_launch_fill_u64(c->L, job.lens, job.budgets.total, (size_t)n, c->stream);
    return VC2HIP_OK;
  }
  // single pass: slice offsets by decoupled look-back inside the pack kernel -- the default where k_hq_pack16 codes the
  // slices (round 6), everywhere with VC2HIP_FLAG_SINGLE_PASS_VBR, nowhere with VC2HIP_FLAG_TWO_PASS_VBR
  // (the look-back pays from ~100 pictures per launch on: the grid puts the same tile of ALL pictures side by side, and a
  // picture's tile t - 1 is only that many workgroups ahead of tile t.  128 UHD pictures: 1.69 ms against 1.47 + 0.51 for
  // slots and compaction; 96: 1.46 = 1.46; 64: 1.15 against 0.75 + 0.25)
  // Only where four slice images fit in LDS (image mode 0): the look-back counts tiles of FOUR slices (k_hq_pack16 has no other form; k_hq_pack's long modes were what overran) --
  // the status words above are sized for them, k_hq_pack adds up four wavefronts' byte counts and takes the picture's length
  // from tile (slices + 3) / 4 - 1.  Long slices (a scalar of 46 or more: two wavefronts or one per workgroup) made twice or
  // four times as many tiles and ran the status words off their buffer: they go through the slots, whatever the flag
  const bool one_pass = vc2_pack_image_mode(prefix, scalar) == 0 && !d_cbr_bytes &&
                        (!c->two_pass_vbr || (!c->force_two_pass_vbr && n >= VC2_ONE_PASS_MIN_PICTURES && vc2_pack_one_pass_default(p)));
  if (one_pass) {
    const long long lb_stride = (long long)((ns + 3) / 4) + 8;
    unsigned long long *lb;
    NEED(c, B_SIZES, (size_t)n * lb_stride * 8, lb);
    HIPCHK(c, hipMemsetAsync(lb, 0, (size_t)n * lb_stride * 8, c->stream));
    vc2_prof_break(c->L);
    p.lookback = lb; p.lookback_stride = lb_stride; p.lens = job.lens;
    vc2_launch_pack(c->L, p, n, c->stream);
    return VC2HIP_OK;
  }
  // (images kept in the slots themselves: room for the two guard words of an image)
  // (under HQ_CBR a slice is up to scalar - 1 bytes longer than that: V's room holds a remainder the length byte does not show)
  const int slot = (int)((max_slice_bytes(prefix, scalar) + (gimg ? 8 : 0) + (d_cbr_bytes ? scalar - 1 : 0) + 15) & ~(size_t)15);
  uint8_t *slots; uint32_t *sizes, *offs;
  // Shared slots (below) hold WHOLE tiles: a picture's last tile has room for all its spt slices even when fewer exist
  // (1080p: 16200 slices in 1013 tiles of 16 = room for 16208).  Rounds 3 - 5 sized the buffer by the slice count; the
  // 2 MiB rounding of large workspaces hid the n * 8 slots that were missing until a batch of 136 HD pictures ran the
  // compaction off the end of it (round 6: tools/probe/fault_bisect.py, tests/test_gpu_parity.py::test_shared_slots_hold_whole_tiles)
  const int spt_room = (gimg || d_cbr_bytes) ? 0 : vc2_pack_slices_per_tile(p);
  const size_t slot_count = spt_room ? (size_t)((ns + spt_room - 1) / spt_room) * spt_room : (size_t)ns;
  NEED(c, B_SLOTS, (size_t)n * slot_count * slot + 32, slots); // (+32: the compaction reads whole 16-byte pieces and the dword behind them)
  NEED(c, B_SIZES, (size_t)n * ns * 4, sizes);
  NEED(c, B_OFFS, (size_t)n * ns * 4, offs);
  p.slots = slots; p.slot_bytes = slot; p.sizes = sizes;
  if (d_cbr_bytes) { p.cbr_bytes = d_cbr_bytes; p.cbr_offsets = job.budgets.offs; }
  // VBR with several slices per wavefront of the packer (slices of up to 256 + 2 x 128 coefficients: HD pictures): the
  // slices of a pack workgroup share a slot, back to back -- sizes, offsets and the compaction are per workgroup (a
  // sixteenth or an eighth of the entries and copies, each as many times as long).  32 HD pictures: pack 0.221 -> 0.227 ms
  // (byte-aligned copy-out), compaction 0.075 -> 0.045.  With a wavefront per slice (UHD: four slices of ~290 bytes per
  // workgroup) the two sides cancel (0.375 + 0.087 against 0.387 + 0.065 ms per 16 pictures), with large slices (UHD-2,
  // scalar 8) it loses: one slot per slice there.
  const int spt = (gimg || d_cbr_bytes) ? 0 : vc2_pack_slices_per_tile(p);
  p.tile_slices = spt;
  vc2_launch_pack(c->L, p, n, c->stream);
  if (spt) {
    const int nt = (ns + spt - 1) / spt;
    vc2_launch_scan_sizes(c->L, sizes, offs, job.lens, nt, n, c->stream);
    vc2_launch_compact(c->L, slots, spt * slot, sizes, offs, job.payload, job.stride, nt, n, c->stream);
    return VC2HIP_OK;
  }
  vc2_launch_scan_sizes(c->L, sizes, offs, job.lens, ns, n, c->stream); // (CBR: the same offsets as the budgets'; sizes = budgets)
  vc2_launch_compact(c->L, slots, slot, sizes, offs, job.payload, job.stride, ns, n, c->stream);
  return VC2HIP_OK;
}

// ------------------------------------------------------------------------------------------
// fine-grained entry points (host planes; test / drop-in granularity)
// ------------------------------------------------------------------------------------------
static int one_plane_geom(Geom &g, int ph, int pw, int depth, int ys, int xs) {
  int phs[3] = {ph, 0, 0}, pws[3] = {pw, 0, 0};
  return make_geom(g, phs, pws, phs, pws, depth, ys, xs);
}

extern "C" int vc2hip_dwt_forward(vc2hip_ctx *c, const int32_t *in, int h, int w, int kernel, int depth,
                                  int32_t *out) {
  if (!c || !in || !out || h < 1 || w < 1 || depth < 1 || depth > VC2_MAX_DEPTH) return set_err(c, VC2HIP_EINVAL);
  if (kernel < 0 || kernel > 6) return set_err(c, VC2HIP_EINVAL, "invalid wavelet kernel");
  ENTER(c);
  const int ph = vc2hip_padded_size(h, depth), pw = vc2hip_padded_size(w, depth);
  Geom g;
  int rc = one_plane_geom(g, ph, pw, depth, ph >> depth, pw >> depth);
  if (rc) return set_err(c, rc);
  // waveletPad (WaveletTransform.cpp:79-94) on the host for this test-granularity entry point
  std::vector<int32_t> padded((size_t)ph * pw);
  for (int y = 0; y < ph; ++y)
    for (int x = 0; x < pw; ++x) padded[(size_t)y * pw + x] = in[(size_t)(y < h ? y : h - 1) * w + (x < w ? x : w - 1)];
  int32_t *d_plane, *d_store, *d_ll;
  const size_t pb = (size_t)ph * pw * 4;
  NEED(c, B_PLANE, pb, d_plane);
  NEED(c, B_STORE, pb, d_store);
  NEED(c, B_LL0, ll_bytes(g, 1) + 16, d_ll);
  LLPlanes ll;
  ll_layout(g, 1, d_ll, ll);
  HIPCHK(c, hipMemcpyAsync(d_plane, padded.data(), pb, hipMemcpyHostToDevice, c->stream));
  const void *src[3] = {d_plane, nullptr, nullptr};
  const RawPlane ss[3] = {{(long long)ph * pw, 0, 0, 0}, {}, {}};
  rc = run_forward(c, g, kernel, 1, src, ss, false, nullptr, records32(g, d_store), ll);
  if (rc) return rc;
  vc2_launch_store_to_plane(c->L, d_store, g.slice_coefs, 0, d_plane, ph, pw, depth, g.ys, g.xs, nullptr, nullptr, 0,
                            c->d_err, c->stream);
  HIPCHK(c, hipMemcpyAsync(out, d_plane, pb, hipMemcpyDeviceToHost, c->stream));
  return vc2hip_sync(c);
}

extern "C" int vc2hip_dwt_inverse(vc2hip_ctx *c, const int32_t *in, int ph, int pw, int kernel, int depth,
                                  int32_t *out, int h, int w) {
  if (!c || !in || !out || depth < 1 || depth > VC2_MAX_DEPTH || h < 1 || w < 1 || h > ph || w > pw) return set_err(c, VC2HIP_EINVAL);
  if (kernel < 0 || kernel > 6) return set_err(c, VC2HIP_EINVAL, "invalid wavelet kernel");
  if (ph % (1 << depth) || pw % (1 << depth)) return set_err(c, VC2HIP_EINVAL);
  ENTER(c);
  Geom g;
  int rc = one_plane_geom(g, ph, pw, depth, ph >> depth, pw >> depth);
  if (rc) return set_err(c, rc);
  int32_t *d_plane, *d_store, *d_ll;
  const size_t pb = (size_t)ph * pw * 4;
  NEED(c, B_PLANE, pb, d_plane);
  NEED(c, B_STORE, pb, d_store);
  NEED(c, B_LL0, ll_bytes(g, 1) + 16, d_ll);
  LLPlanes ll;
  ll_layout(g, 1, d_ll, ll);
  HIPCHK(c, hipMemcpyAsync(d_plane, in, pb, hipMemcpyHostToDevice, c->stream));
  vc2_launch_plane_to_store(c->L, d_plane, ph, pw, depth, g.ys, g.xs, d_store, g.slice_coefs, 0, c->stream);
  void *dst[3] = {d_plane, nullptr, nullptr};
  const RawPlane ds[3] = {{(long long)ph * pw, 0, 0, 0}, {}, {}};
  InverseJob job; // (coefficients in, int32 samples out: no matrix, no raw words)
  job.store = records32(g, d_store);
  job.dst = dst; job.dst_l = ds;
  rc = run_inverse(c, g, kernel, 1, job, ll);
  if (rc) return rc;
  std::vector<int32_t> full((size_t)ph * pw);
  HIPCHK(c, hipMemcpyAsync(full.data(), d_plane, pb, hipMemcpyDeviceToHost, c->stream));
  rc = vc2hip_sync(c);
  if (rc) return rc;
  for (int y = 0; y < h; ++y) memcpy(out + (size_t)y * w, full.data() + (size_t)y * pw, (size_t)w * 4); // resize(shape), :340
  return VC2HIP_OK;
}

// common body of quantise_np / dequantise_np / dequantise_ld
static int plane_quant_op(vc2hip_ctx *c, const int32_t *in, int ph, int pw, int depth, const int32_t *qidx, int ys,
                          int xs, const int32_t *qm, int32_t *out, int op /*0 quant,1 scale,2 scale+LD*/) {
  if (!c || !in || !out || !qidx || !qm) return set_err(c, VC2HIP_EINVAL);
  ENTER(c);
  Geom g;
  int rc = one_plane_geom(g, ph, pw, depth, ys, xs);
  if (rc) return set_err(c, rc);
  const size_t pb = (size_t)ph * pw * 4;
  const int ns = ys * xs, nb = 3 * depth + 1;
  int32_t *d_plane, *d_store, *d_q, *d_ll = nullptr;
  int *d_qm;
  NEED(c, B_PLANE, pb, d_plane);
  NEED(c, B_STORE, pb, d_store);
  NEED(c, B_QIDX, (size_t)ns * 4, d_q);
  NEED(c, B_QM, 256, d_qm);
  HIPCHK(c, hipMemcpyAsync(d_plane, in, pb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_q, qidx, (size_t)ns * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_qm, qm, (size_t)nb * 4, hipMemcpyHostToDevice, c->stream));
  vc2_launch_plane_to_store(c->L, d_plane, ph, pw, depth, ys, xs, d_store, g.slice_coefs, 0, c->stream);
  if (op == 0) {
    vc2_launch_quantise_store(c->L, d_store, ns, g.slice_coefs, g.c[0].sh * g.c[0].sw, 0, g.c[0].n0, d_q, d_qm, c->d_err, c->stream);
    vc2_launch_store_to_plane(c->L, d_store, g.slice_coefs, 0, d_plane, ph, pw, depth, ys, xs, d_q, d_qm, 0, c->d_err, c->stream);
  } else {
    vc2_launch_store_to_plane(c->L, d_store, g.slice_coefs, 0, d_plane, ph, pw, depth, ys, xs, d_q, d_qm, 1, c->d_err, c->stream);
  }
  const int llh = ph >> depth, llw = pw >> depth;
  if (op == 2) {
    NEED(c, B_LL0, (size_t)llh * llw * 4, d_ll);
    vc2_launch_ld_ll(c->L, d_store, 0, g.slice_coefs, 0, g.c[0].n0, llh, llw, ys, xs, d_q, qm[0], d_ll, 0, 1, c->d_err, c->stream);
  }
  HIPCHK(c, hipMemcpyAsync(out, d_plane, pb, hipMemcpyDeviceToHost, c->stream));
  std::vector<int32_t> llh_host;
  if (op == 2) {
    llh_host.resize((size_t)llh * llw);
    HIPCHK(c, hipMemcpyAsync(llh_host.data(), d_ll, llh_host.size() * 4, hipMemcpyDeviceToHost, c->stream));
  }
  rc = vc2hip_sync(c);
  if (rc) return rc;
  if (op == 2) {
    const int s = 1 << depth;
    for (int y = 0; y < llh; ++y)
      for (int x = 0; x < llw; ++x) out[(size_t)y * s * pw + (size_t)x * s] = llh_host[(size_t)y * llw + x];
  }
  return VC2HIP_OK;
}
extern "C" int vc2hip_quantise_np(vc2hip_ctx *c, const int32_t *coef, int ph, int pw, int depth, const int32_t *qidx,
                                  int ys, int xs, const int32_t *qm, int32_t *out) {
  return plane_quant_op(c, coef, ph, pw, depth, qidx, ys, xs, qm, out, 0);
}
extern "C" int vc2hip_dequantise_np(vc2hip_ctx *c, const int32_t *q, int ph, int pw, int depth, const int32_t *qidx,
                                    int ys, int xs, const int32_t *qm, int32_t *out) {
  return plane_quant_op(c, q, ph, pw, depth, qidx, ys, xs, qm, out, 1);
}
extern "C" int vc2hip_dequantise_ld(vc2hip_ctx *c, const int32_t *q, int ph, int pw, int depth, const int32_t *qidx,
                                    int ys, int xs, const int32_t *qm, int32_t *out) {
  return plane_quant_op(c, q, ph, pw, depth, qidx, ys, xs, qm, out, 2);
}

static int geom_from_abi(Geom &g, const vc2hip_geom *a) {
  int ph[3] = {a->luma_h, a->chroma_h, a->chroma_h}, pw[3] = {a->luma_w, a->chroma_w, a->chroma_w};
  return make_geom(g, ph, pw, ph, pw, a->depth, a->y_slices, a->x_slices);
}

// upload three planes and scatter them into the store
static int planes_to_store(vc2hip_ctx *c, const Geom &g, const int32_t *const pl[3], int32_t *d_store) {
  size_t mx = 0;
  for (int k = 0; k < 3; ++k) mx = std::max(mx, (size_t)g.c[k].ph * g.c[k].pw * 4);
  int32_t *d_plane;
  NEED(c, B_PLANE, mx * 3, d_plane);
  for (int k = 0; k < 3; ++k) {
    int32_t *dp = d_plane + (mx / 4) * k;
    HIPCHK(c, hipMemcpyAsync(dp, pl[k], (size_t)g.c[k].ph * g.c[k].pw * 4, hipMemcpyHostToDevice, c->stream));
    vc2_launch_plane_to_store(c->L, dp, g.c[k].ph, g.c[k].pw, g.depth, g.ys, g.xs, d_store, g.slice_coefs, g.c[k].coef_off, c->stream);
  }
  return VC2HIP_OK;
}
static int store_to_planes(vc2hip_ctx *c, const Geom &g, const int32_t *d_store, int32_t *const pl[3]) {
  size_t mx = 0;
  for (int k = 0; k < 3; ++k) mx = std::max(mx, (size_t)g.c[k].ph * g.c[k].pw * 4);
  int32_t *d_plane;
  NEED(c, B_PLANE, mx * 3, d_plane);
  for (int k = 0; k < 3; ++k) {
    int32_t *dp = d_plane + (mx / 4) * k;
    vc2_launch_store_to_plane(c->L, d_store, g.slice_coefs, g.c[k].coef_off, dp, g.c[k].ph, g.c[k].pw, g.depth, g.ys, g.xs,
                              nullptr, nullptr, 0, c->d_err, c->stream);
    HIPCHK(c, hipMemcpyAsync(pl[k], dp, (size_t)g.c[k].ph * g.c[k].pw * 4, hipMemcpyDeviceToHost, c->stream));
  }
  return VC2HIP_OK;
}

// The one owner of the context's budget tables (B_CBRB, B_CBRO, cbr_total) and of the key that says what they hold.
// Two slots, each with its own buffers, key and total under the same rule: slot 0 is every call's; slot 1 holds the OUTPUT's
// budgets of vc2hip_transcode_cbr_batch_dev, whose HQ_CBR input may claim its offsets from another budget's tables in the same
// call -- one slot would upload and wait in every such call, and could not be captured into a graph.
// HQ_CBR: the budgets of vc2hip_slice_bytes(ys, xs, compressed_bytes, scalar), each slice `prefix` bytes behind the one before.
// LD: scalar 1 and prefix LD_BUDGETS (EncodeStream.cpp:509-512, DecodeStream.cpp:312, :331-333) -- the offsets carry no prefix.
// Both are uploaded only when the key differs from the cached one or the buffer is gone: no copy and no wait in any later call.
// given: the caller's own budgets (the fine-grained int32 entry points; compressed_bytes and scalar are not looked at): always
// uploaded, and the cache is left invalid.  The key returns only behind a complete upload, so a failure on the way (an
// allocation, a copy) leaves no mode another mode's tables.  vc2hip_slice_bytes refuses ys, xs or scalar below 1 and nothing
// else; every caller's entry checks hold all three (make_geom / stream_cp_ok, encode_check / decode_check; LD passes 1).
enum { LD_BUDGETS = -7 };
static int budget_tables(vc2hip_ctx *c, int ys, int xs, int compressed_bytes, int scalar, int prefix, Budgets &b, const int32_t *given = nullptr,
                         int slot = 0) {
  const int ns = ys * xs;
  const int key[5] = {ys, xs, compressed_bytes, scalar, prefix};
  const int id_bytes = slot ? B_CBRB2 : B_CBRB, id_offs = slot ? B_CBRO2 : B_CBRO;
  int *const cached = c->cbr_key[slot];
  if (given || memcmp(key, cached, sizeof key) || !c->buf[id_bytes].p) {
    cached[0] = -1; // whatever was cached is overwritten
    std::vector<int32_t> made;
    if (!given) {
      made.resize(ns);
      if (int rc = vc2hip_slice_bytes(ys, xs, compressed_bytes, scalar, made.data())) return set_err(c, rc);
    }
    const int32_t *bytes = given ? given : made.data();
    std::vector<uint32_t> offs(ns);
    uint64_t run = 0;
    for (int i = 0; i < ns; ++i) { offs[i] = (uint32_t)run; run += (uint64_t)bytes[i] + (prefix == LD_BUDGETS ? 0 : prefix); }
    int32_t *db; uint32_t *dof;
    NEED(c, id_bytes, (size_t)ns * 4, db);
    NEED(c, id_offs, (size_t)ns * 4, dof);
    HIPCHK(c, hipMemcpyAsync(db, bytes, (size_t)ns * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dof, offs.data(), (size_t)ns * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the tables live on this function's stack)
    c->cbr_total[slot] = run;
    if (!given) memcpy(cached, key, sizeof key);
  }
  b = Budgets{(const int32_t *)c->buf[id_bytes].p, (const uint32_t *)c->buf[id_offs].p, c->cbr_total[slot]};
  return VC2HIP_OK;
}

extern "C" int vc2hip_hq_pack(vc2hip_ctx *c, const int32_t *y, const int32_t *u, const int32_t *v, const vc2hip_geom *ga,
                              const int32_t *qidx, int prefix, int scalar, const int32_t *cbr, uint8_t *out, size_t cap,
                              size_t *out_len) {
  if (!c || !y || !u || !v || !ga || !qidx || !out || !out_len || prefix < 0 || scalar < 1) return set_err(c, VC2HIP_EINVAL);
  ENTER(c);
  Geom g;
  int rc = geom_from_abi(g, ga);
  if (rc) return set_err(c, rc);
  const int ns = g.ys * g.xs;
  int32_t *d_store, *d_q; uint8_t *d_pay; unsigned long long *d_len;
  NEED(c, B_STORE, (size_t)ns * g.slice_coefs * 4, d_store);
  NEED(c, B_QIDX, (size_t)ns * 4, d_q);
  NEED(c, B_LENS, 64, d_len);
  const int32_t *pl[3] = {y, u, v};
  if ((rc = planes_to_store(c, g, pl, d_store))) return rc;
  HIPCHK(c, hipMemcpyAsync(d_q, qidx, (size_t)ns * 4, hipMemcpyHostToDevice, c->stream));
  size_t paycap = (size_t)ns * max_slice_bytes(prefix, scalar);
  PackJob job; // (no matrix: the planes are quantised)
  if (cbr) {
    if ((rc = budget_tables(c, g.ys, g.xs, 0, scalar, prefix, job.budgets, cbr))) return rc;
    paycap = job.budgets.total;
  }
  NEED(c, B_PAYLOAD, paycap + 64, d_pay);
  job.store = records32(g, d_store);
  job.qidx = d_q; job.prefix = prefix; job.scalar = scalar;
  job.payload = d_pay; job.stride = (long long)paycap; job.lens = d_len;
  if ((rc = run_pack(c, g, 1, job))) return rc;
  unsigned long long len = 0;
  HIPCHK(c, hipMemcpyAsync(&len, d_len, 8, hipMemcpyDeviceToHost, c->stream));
  if ((rc = vc2hip_sync(c))) return rc;
  if (len > cap) return set_err(c, VC2HIP_ECAP);
  HIPCHK(c, hipMemcpy(out, d_pay, len, hipMemcpyDeviceToHost));
  *out_len = (size_t)len;
  return VC2HIP_OK;
}

// slice offsets of one VBR payload already on the device
// claim (the HQ_CBR slice budgets, or none): the offsets are first claimed from the budgets and checked against the
// stream (vc2_launch_cbr_index); the general index only works if that fails
static int build_index(vc2hip_ctx *c, const uint8_t *d_pay, long long stride, const unsigned long long *d_lens, int n, int ns,
                       int prefix, int scalar, uint32_t **d_offs_out, const Budgets &claim = Budgets{}) {
  uint32_t *d_offs; void *ws;
  NEED(c, B_OFFS, (size_t)n * ns * 4, d_offs);
  const size_t wsb = vc2_slice_index_workspace(n, (size_t)stride, prefix, scalar);
  NEED(c, B_INDEX, wsb, ws);
  HIPCHK(c, hipMemsetAsync(d_offs, 0xFF, (size_t)n * ns * 4, c->stream)); // unreachable slices read past the payload
  unsigned *bad = nullptr;
  if (claim.bytes && c->allow_cbr_index) {
    bad = (unsigned *)((char *)c->d_err + 64); // (the error word's block: 256 bytes, the LD tables behind them)
    HIPCHK(c, hipMemsetAsync(bad, 0, sizeof(unsigned), c->stream));
  }
  vc2_prof_break(c->L);
  if (bad) vc2_launch_cbr_index(c->L, d_pay, stride, d_lens, claim.bytes, claim.offs, claim.total, d_offs, ns, prefix, scalar, n, bad, c->stream);
  vc2_launch_slice_index(c->L, d_pay, stride, d_lens, d_offs, ns, prefix, scalar, n, c->d_err, c->stream, ws, wsb, bad);
  *d_offs_out = d_offs;
  return VC2HIP_OK;
}

// The HQ slice reader's job.  Band planes, record heads, xs and the statistics word are the batch decoders' to add.
static void fill_unpack(UnpackParams &p, const Geom &g, const uint8_t *d_pay, long long stride, const unsigned long long *d_lens,
                        const uint32_t *d_offs, const Store &st, int32_t *d_q, int prefix, int scalar, unsigned *err) {
  memset(&p, 0, sizeof p);
  p.payload = d_pay; p.payload_stride = stride; p.lens = d_lens; p.offsets = d_offs;
  p.store = st.p; p.store_stride = st.stride; p.qidx = d_q;
  p.store16 = st.s16; p.store_wide = st.wide;
  p.n_slices = g.ys * g.xs; p.slice_coefs = g.slice_coefs;
  int n0[3];
  fill_comp_arrays(g, p.comp_n, p.comp_off, n0);
  p.prefix = prefix; p.scalar = scalar; p.err = err;
}
// The HQ_CBR index search's job (HQ_CAPPED measures with the same: CapParams::s); d_sb: the slice budgets
static void fill_cbr(CbrParams &p, const Geom &g, const Store &st, int32_t *d_q, const int32_t *d_sb, int scalar, const int32_t *qm,
                     bool general_only, unsigned *err) {
  memset(&p, 0, sizeof p);
  p.store = st.p; p.store_stride = st.stride; p.qidx = d_q; p.slice_bytes = d_sb;
  p.store16 = st.s16; p.store_wide = st.wide;
  p.n_slices = g.ys * g.xs; p.slice_coefs = g.slice_coefs;
  fill_comp_arrays(g, p.comp_n, p.comp_off, p.comp_n0);
  p.scalar = scalar; p.err = err;
  p.general_only = general_only;
  p.n_bands = 3 * g.depth + 1;
  for (int b = 0; b < p.n_bands; ++b) p.qmatrix[b] = qm[b];
}

extern "C" int vc2hip_hq_unpack(vc2hip_ctx *c, const uint8_t *in, size_t len, const vc2hip_geom *ga, int prefix, int scalar,
                                int32_t *y, int32_t *u, int32_t *v, int32_t *qidx, size_t *consumed) {
  if (!c || !in || !ga || !y || !u || !v || !qidx || prefix < 0 || scalar < 1) return set_err(c, VC2HIP_EINVAL);
  ENTER(c);
  Geom g;
  int rc = geom_from_abi(g, ga);
  if (rc) return set_err(c, rc);
  const int ns = g.ys * g.xs;
  int32_t *d_store, *d_q; uint8_t *d_pay; unsigned long long *d_len; uint32_t *d_offs;
  NEED(c, B_STORE, (size_t)ns * g.slice_coefs * 4, d_store);
  NEED(c, B_QIDX, (size_t)ns * 4, d_q);
  NEED(c, B_LENS, 64, d_len);
  const size_t stride = (len + 63) & ~(size_t)63;
  NEED(c, B_PAYLOAD, stride + 64, d_pay);
  unsigned long long l64 = len;
  HIPCHK(c, hipMemcpyAsync(d_pay, in, len, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_len, &l64, 8, hipMemcpyHostToDevice, c->stream));
  if ((rc = build_index(c, d_pay, (long long)stride, d_len, 1, ns, prefix, scalar, &d_offs))) return rc;
  UnpackParams p;
  fill_unpack(p, g, d_pay, (long long)stride, d_len, d_offs, records32(g, d_store), d_q, prefix, scalar, c->d_err);
  vc2_launch_unpack(c->L, p, 1, c->stream);
  int32_t *pl[3] = {y, u, v};
  if ((rc = store_to_planes(c, g, d_store, pl))) return rc;
  HIPCHK(c, hipMemcpyAsync(qidx, d_q, (size_t)ns * 4, hipMemcpyDeviceToHost, c->stream));
  uint32_t last_off = 0;
  HIPCHK(c, hipMemcpyAsync(&last_off, d_offs + ns - 1, 4, hipMemcpyDeviceToHost, c->stream));
  if ((rc = vc2hip_sync(c))) return rc;
  if (consumed) { // end of the last slice
    size_t pos = (size_t)last_off + prefix + 1;
    for (int k = 0; k < 3 && pos < len; ++k) pos += 1 + (size_t)in[pos] * scalar;
    *consumed = pos;
  }
  return VC2HIP_OK;
}

extern "C" int vc2hip_cbr_qindices(vc2hip_ctx *c, const int32_t *y, const int32_t *u, const int32_t *v, const vc2hip_geom *ga,
                                   const int32_t *qm, const int32_t *slice_bytes, int scalar, int32_t *qidx) {
  if (!c || !y || !u || !v || !ga || !qm || !slice_bytes || !qidx || scalar < 1) return set_err(c, VC2HIP_EINVAL);
  ENTER(c);
  Geom g;
  int rc = geom_from_abi(g, ga);
  if (rc) return set_err(c, rc);
  const int ns = g.ys * g.xs;
  int32_t *d_store, *d_q;
  NEED(c, B_STORE, (size_t)ns * g.slice_coefs * 4, d_store);
  NEED(c, B_QIDX, (size_t)ns * 4, d_q);
  const int32_t *pl[3] = {y, u, v};
  if ((rc = planes_to_store(c, g, pl, d_store))) return rc;
  Budgets b; // (the search reads the bytes alone; the offsets are uploaded beside them only because the owner keeps the pair whole)
  if ((rc = budget_tables(c, g.ys, g.xs, 0, scalar, 0, b, slice_bytes))) return rc;
  CbrParams p;
  fill_cbr(p, g, records32(g, d_store), d_q, b.bytes, scalar, qm, c->cbr_general, c->d_err);
  vc2_launch_cbr(c->L, p, 1, c->stream);
  HIPCHK(c, hipMemcpyAsync(qidx, d_q, (size_t)ns * 4, hipMemcpyDeviceToHost, c->stream));
  return vc2hip_sync(c);
}

static void fill_ld_unpack(LdUnpackParams &p, const Geom &g, const uint8_t *d_pay, long long stride, const Budgets &b,
                           const Store &st, int32_t *d_q, unsigned *err) { // (LD stores are int32 throughout)
  memset(&p, 0, sizeof p);
  p.payload = d_pay; p.payload_stride = stride; p.slice_bytes = b.bytes; p.offsets = b.offs;
  p.store = (int32_t *)st.p; p.store_stride = st.stride; p.qidx = d_q;
  p.n_slices = g.ys * g.xs; p.slice_coefs = g.slice_coefs;
  int n0[3];
  fill_comp_arrays(g, p.comp_n, p.comp_off, n0);
  p.err = err;
}

// LD: the quantised LL residuals of n pictures' slice records -> the DC-predicted, reconstructed LL planes of the deepest
// level (Quantisation.cpp:287-306).  One launch for the three components, or one each where a plane does not fit in LDS.
static void ld_restore_ll(vc2hip_ctx *c, const Geom &g, int n, const Store &st, const int32_t *d_q, int qm0, const LLPlanes &ll) {
  LdLl3Params lp;
  lp.store = (const int32_t *)st.p; lp.store_stride = st.stride; lp.slice_coefs = g.slice_coefs;
  lp.ys = g.ys; lp.xs = g.xs; lp.qidx = d_q; lp.qm0 = qm0; lp.err = c->d_err;
  for (int k = 0; k < 3; ++k) {
    lp.coef_off[k] = g.c[k].coef_off; lp.llh[k] = g.c[k].ph >> g.depth; lp.llw[k] = g.c[k].pw >> g.depth;
    lp.ll_plane[k] = (int32_t *)ll.p[g.depth][k]; lp.ll_stride[k] = ll.stride[g.depth][k];
  }
  if (vc2_launch_ld_ll3(c->L, lp, n, c->stream)) return;
  for (int k = 0; k < 3; ++k)
    vc2_launch_ld_ll(c->L, lp.store, lp.store_stride, g.slice_coefs, g.c[k].coef_off, g.c[k].n0, lp.llh[k], lp.llw[k], g.ys, g.xs, d_q, qm0,
                     lp.ll_plane[k], lp.ll_stride[k], n, c->d_err, c->stream);
}

extern "C" int vc2hip_ld_unpack(vc2hip_ctx *c, const uint8_t *in, size_t len, const vc2hip_geom *ga, const int32_t *slice_bytes,
                                int32_t *y, int32_t *u, int32_t *v, int32_t *qidx, size_t *consumed) {
  if (!c || !in || !ga || !slice_bytes || !y || !u || !v || !qidx) return set_err(c, VC2HIP_EINVAL);
  ENTER(c);
  Geom g;
  int rc = geom_from_abi(g, ga);
  if (rc) return set_err(c, rc);
  const int ns = g.ys * g.xs;
  int32_t *d_store, *d_q; uint8_t *d_pay; Budgets b;
  NEED(c, B_STORE, (size_t)ns * g.slice_coefs * 4, d_store);
  NEED(c, B_QIDX, (size_t)ns * 4, d_q);
  if ((rc = budget_tables(c, g.ys, g.xs, 0, 1, LD_BUDGETS, b, slice_bytes))) return rc;
  if (b.total > len) return set_err(c, VC2HIP_ESTREAM);
  NEED(c, B_PAYLOAD, len + 64, d_pay);
  HIPCHK(c, hipMemcpyAsync(d_pay, in, len, hipMemcpyHostToDevice, c->stream));
  LdUnpackParams p;
  fill_ld_unpack(p, g, d_pay, (long long)len, b, records32(g, d_store), d_q, c->d_err);
  vc2_launch_ld_unpack(c->L, p, 1, c->stream);
  int32_t *pl[3] = {y, u, v};
  if ((rc = store_to_planes(c, g, d_store, pl))) return rc;
  HIPCHK(c, hipMemcpyAsync(qidx, d_q, (size_t)ns * 4, hipMemcpyDeviceToHost, c->stream));
  if (consumed) *consumed = (size_t)b.total;
  return vc2hip_sync(c);
}

// ------------------------------------------------------------------------------------------
// LD encode
// ------------------------------------------------------------------------------------------
static int fill_ld_enc(vc2hip_ctx *c, LdEncParams &p, const Geom &g, const Store &st, int32_t *d_q, const int32_t *qm,
                       const LLPlanes &ll, const Budgets &b, int max_slice, uint8_t *d_pay, long long stride) {
  memset(&p, 0, sizeof p);
  const int ns = g.ys * g.xs;
  p.store = (int32_t *)st.p; p.store_stride = st.stride; p.qidx = d_q;
  p.slice_bytes = b.bytes; p.offsets = b.offs;
  for (int k = 0; k < 3; ++k) {
    p.restored[k] = (int32_t *)ll.p[g.depth][k]; p.restored_stride[k] = ll.stride[g.depth][k];
    p.ll_w[k] = g.c[k].pw >> g.depth;
    p.bh[k] = (g.c[k].ph >> g.depth) / g.ys; p.bw[k] = (g.c[k].pw >> g.depth) / g.xs;
  }
  p.ys = g.ys; p.xs = g.xs; p.n_slices = ns; p.slice_coefs = g.slice_coefs;
  p.diagonals = c->ld_diagonals;
  p.depth = g.depth;
  p.rs_ints = 0;
  for (int k = 0; k < 3; ++k) if (g.c[k].ph) p.rs_ints += (p.bh[k] + 1) * (p.bw[k] + 1);
  fill_comp_arrays(g, p.comp_n, p.comp_off, p.comp_n0);
  for (int b = 0; b < 3 * g.depth + 1; ++b) p.qmatrix[b] = qm ? qm[b] : 0;
  p.img_words = (max_slice + 3) / 4 + 2;
  p.payload = d_pay; p.payload_stride = stride; p.err = c->d_err;
  p.tab = (int *)((char *)c->d_err + 256);
  // what has to fit in LDS whatever the slice's size: the LL blocks with their halo (search) and one slice's bytes (writer)
  if (512 + (size_t)p.rs_ints * 4 > 160 * 1024 || (size_t)p.img_words * 4 > 160 * 1024)
    return set_err(c, VC2HIP_EINVAL, "slice too large for the LD encode kernels");
  if ((size_t)g.slice_coefs * 8 + 512 + (size_t)p.rs_ints * 4 > 160 * 1024) { // the coefficients do not: the search reads the store, its trials write a scratch array
    NEED(c, B_PLANE2, (size_t)((p.store_stride ? p.store_stride : 1)) * 4 * (size_t)std::max(1, c->ld_batch), p.scratch);
  }
  c->ld_batch = 1;
  return VC2HIP_OK;
}

/* quantise_transform (LD, DC-predicted LL band), Quantisation.cpp:358-367 over :213-234 */
extern "C" int vc2hip_quantise_ld(vc2hip_ctx *c, const int32_t *coef, int ph, int pw, int depth, const int32_t *qidx,
                                  int ys, int xs, const int32_t *qm, int32_t *out) {
  if (!c || !coef || !out || !qidx || !qm) return set_err(c, VC2HIP_EINVAL);
  ENTER(c);
  Geom g;
  int rc = one_plane_geom(g, ph, pw, depth, ys, xs);
  if (rc) return set_err(c, rc);
  const size_t pb = (size_t)ph * pw * 4;
  const int ns = ys * xs;
  int32_t *d_plane, *d_store, *d_q, *d_ll;
  NEED(c, B_PLANE, pb, d_plane);
  NEED(c, B_STORE, pb, d_store);
  NEED(c, B_QIDX, (size_t)ns * 4, d_q);
  NEED(c, B_LL0, ll_bytes(g, 1) + 16, d_ll);
  LLPlanes ll;
  ll_layout(g, 1, d_ll, ll);
  HIPCHK(c, hipMemcpyAsync(d_plane, coef, pb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_q, qidx, (size_t)ns * 4, hipMemcpyHostToDevice, c->stream));
  vc2_launch_plane_to_store(c->L, d_plane, ph, pw, depth, ys, xs, d_store, g.slice_coefs, 0, c->stream);
  LdEncParams p;
  if ((rc = fill_ld_enc(c, p, g, records32(g, d_store), d_q, qm, ll, Budgets{}, 0, nullptr, 0))) return rc;
  p.search = 0;
  vc2_launch_ld_quantise(c->L, p, 1, c->stream);
  vc2_launch_store_to_plane(c->L, d_store, g.slice_coefs, 0, d_plane, ph, pw, depth, ys, xs, nullptr, nullptr, 0, c->d_err, c->stream);
  HIPCHK(c, hipMemcpyAsync(out, d_plane, pb, hipMemcpyDeviceToHost, c->stream));
  return vc2hip_sync(c);
}

/* quantIndicesLD(coefficients, qMatrix, sliceBytes), EncodeStream.cpp:141-245.  y,u,v: TRANSFORM planes */
extern "C" int vc2hip_ld_qindices(vc2hip_ctx *c, const int32_t *y, const int32_t *u, const int32_t *v, const vc2hip_geom *ga,
                                  const int32_t *qm, const int32_t *slice_bytes, int32_t *qidx) {
  if (!c || !y || !u || !v || !ga || !qm || !slice_bytes || !qidx) return set_err(c, VC2HIP_EINVAL);
  ENTER(c);
  Geom g;
  int rc = geom_from_abi(g, ga);
  if (rc) return set_err(c, rc);
  const int ns = g.ys * g.xs;
  int32_t *d_store, *d_q, *d_ll; Budgets b;
  NEED(c, B_STORE, (size_t)ns * g.slice_coefs * 4, d_store);
  NEED(c, B_QIDX, (size_t)ns * 4, d_q);
  NEED(c, B_LL0, ll_bytes(g, 1) + 16, d_ll);
  LLPlanes ll;
  ll_layout(g, 1, d_ll, ll);
  const int32_t *pl[3] = {y, u, v};
  if ((rc = planes_to_store(c, g, pl, d_store))) return rc;
  if ((rc = budget_tables(c, g.ys, g.xs, 0, 1, LD_BUDGETS, b, slice_bytes))) return rc;
  LdEncParams p;
  if ((rc = fill_ld_enc(c, p, g, records32(g, d_store), d_q, qm, ll, b, 0, nullptr, 0))) return rc;
  p.search = 1;
  vc2_launch_ld_quantise(c->L, p, 1, c->stream);
  HIPCHK(c, hipMemcpyAsync(qidx, d_q, (size_t)ns * 4, hipMemcpyDeviceToHost, c->stream));
  return vc2hip_sync(c);
}

/* operator<<(ostream&, const Slices&) under sliceio::lowDelay(bytes), Slices.cpp:645-660 over :195-244.
 * y,u,v: QUANTISED planes (LL band as prediction residuals). */
extern "C" int vc2hip_ld_pack(vc2hip_ctx *c, const int32_t *y, const int32_t *u, const int32_t *v, const vc2hip_geom *ga,
                              const int32_t *qidx, const int32_t *slice_bytes, uint8_t *out, size_t cap, size_t *out_len) {
  if (!c || !y || !u || !v || !ga || !qidx || !slice_bytes || !out || !out_len) return set_err(c, VC2HIP_EINVAL);
  ENTER(c);
  Geom g;
  int rc = geom_from_abi(g, ga);
  if (rc) return set_err(c, rc);
  const int ns = g.ys * g.xs;
  int mx = 1;
  for (int i = 0; i < ns; ++i) { if (slice_bytes[i] < 1) return set_err(c, VC2HIP_EINVAL); mx = std::max(mx, slice_bytes[i]); }
  int32_t *d_store, *d_q; uint8_t *d_pay; Budgets b;
  NEED(c, B_STORE, (size_t)ns * g.slice_coefs * 4, d_store);
  NEED(c, B_QIDX, (size_t)ns * 4, d_q);
  const int32_t *pl[3] = {y, u, v};
  if ((rc = planes_to_store(c, g, pl, d_store))) return rc;
  HIPCHK(c, hipMemcpyAsync(d_q, qidx, (size_t)ns * 4, hipMemcpyHostToDevice, c->stream));
  if ((rc = budget_tables(c, g.ys, g.xs, 0, 1, LD_BUDGETS, b, slice_bytes))) return rc;
  const uint64_t total = b.total;
  if (total > cap) return set_err(c, VC2HIP_ECAP);
  NEED(c, B_PAYLOAD, total + 64, d_pay);
  LLPlanes ll;
  memset(&ll, 0, sizeof ll);
  LdEncParams p;
  if ((rc = fill_ld_enc(c, p, g, records32(g, d_store), d_q, nullptr, ll, b, mx, d_pay, (long long)total))) return rc;
  vc2_launch_ld_pack(c->L, p, 1, c->stream);
  if ((rc = vc2hip_sync(c))) return rc;
  HIPCHK(c, hipMemcpy(out, d_pay, total, hipMemcpyDeviceToHost));
  *out_len = (size_t)total;
  return VC2HIP_OK;
}

// ------------------------------------------------------------------------------------------
// fused picture path
// ------------------------------------------------------------------------------------------
// The raw words of a batch of pictures (vc2_raw_pic_offset).  fb: the format of the buffer's pictures; lay: the caller's sample
// layout of them (null: the file format).  fields == 1: the coded pictures are the buffer's.  fields == 2: they are the fields
// of the buffer's interleaved frames, in stream order: the first field of a frame is its even rows when top_first, else its
// odd rows -- the field addressing goes on top of the frame's layout.
static void raw_planes(const vc2hip_picture_format *fb, const vc2hip_sample_layout *lay, const void *base, int fields, int top_first,
                       const void *pl[3], RawPlane rl[3]) {
  RawLayout r;
  (void)resolve_layout(fb, lay, r); // (refused by the entry points: batch_layout)
  for (int k = 0; k < 3; ++k) {
    const bool second_first = fields == 2 && !top_first; // (the first field starts on the frame's row 1)
    pl[k] = (const uint8_t *)base + r.at[k] + (second_first ? r.pitch[k] : 0);
    rl[k].stride = (long long)r.stride;
    rl[k].pitch = fields * (int)r.pitch[k];
    rl[k].field_step = fields == 2 ? (top_first ? (int)r.pitch[k] : -(int)r.pitch[k]) : 0;
    rl[k].field_shift = fields == 2;
    rl[k].le = r.le; rl[k].lsb = r.lsb;
  }
}

// Where the transform's edge kernels find the raw words of one caller buffer: the buffer itself under the context's sample
// layout, or -- under a packed format -- the context's planar staging of it (semi-planar: the Y plane stays in the caller's
// buffer, only the chroma is staged).  An input is unpacked into the staging before the first launch reads it, an output
// packed from it behind the last launch that writes it (view_convert), on the context's stream.
struct RawView {
  const vc2hip_sample_layout *lay; // planar: the caller's layout (null: the file format) ...
  const void *base;                // ... of this buffer
  bool packed;
  PackedLayout pl;                 // packed: the caller's buffer
  uint8_t *stage;                  // the staging (null with a null buffer: planning only)
  size_t spitch[3], sat[3], sstride; // its rows, planes and pictures (semi-planar: [0] unused)
  int word_bytes, width, n;        // of the buffer's pictures
};
// fb: the format of the buffer's pictures (frames for the field calls), nbuf of them; which: B_PKIN / B_PKOUT
static int raw_view(vc2hip_ctx *c, const vc2hip_picture_format *fb, int nbuf, const void *base, int which, RawView &v) {
  memset(&v, 0, sizeof v);
  v.base = base;
  const vc2hip_packed_format *pf = active_packed(c);
  if (!pf) { v.lay = active_layout(c); return VC2HIP_OK; }
  if (const char *e = resolve_packed(fb, pf, v.pl)) return set_err(c, VC2HIP_EINVAL, e); // (refused at the entry points already)
  v.packed = true;
  v.word_bytes = fb->word_bytes; v.width = fb->width; v.n = nbuf;
  int ch, cw;
  chroma_dims(fb->height, fb->width, fb->chroma_format, &ch, &cw);
  const size_t py = ((size_t)fb->width * fb->word_bytes + 15) & ~(size_t)15, pc = ((size_t)cw * fb->word_bytes + 15) & ~(size_t)15;
  const bool y_staged = v.pl.packing == VC2HIP_PACKING_V210;
  v.spitch[0] = py; v.spitch[1] = v.spitch[2] = pc;
  v.sat[0] = 0; v.sat[1] = y_staged ? (size_t)fb->height * py : 0; v.sat[2] = v.sat[1] + (size_t)ch * pc;
  v.sstride = v.sat[2] + (size_t)ch * pc;
  if (base) NEED(c, which, (size_t)nbuf * v.sstride + 16, v.stage);
  return VC2HIP_OK;
}
// raw_planes for a view of pictures of format fb
static void view_planes(const RawView &v, const vc2hip_picture_format *fb, int fields, int top_first, const void *pl[3], RawPlane rl[3]) {
  if (!v.packed) { raw_planes(fb, v.lay, v.base, fields, top_first, pl, rl); return; }
  const bool v210 = v.pl.packing == VC2HIP_PACKING_V210;
  for (int k = 0; k < 3; ++k) {
    const bool in_place = !v210 && k == 0; // (the Y plane of a semi-planar picture: plane 0 of a layout in the caller's word form)
    const uint8_t *at = in_place ? (const uint8_t *)v.base + v.pl.at[0] : v.stage + v.sat[k];
    const size_t pitch = in_place ? v.pl.pitch[0] : v.spitch[k];
    const bool second_first = fields == 2 && !top_first;
    pl[k] = at + (second_first ? pitch : 0);
    rl[k].stride = (long long)(in_place ? v.pl.stride : v.sstride);
    rl[k].pitch = fields * (int)pitch;
    rl[k].field_step = fields == 2 ? (top_first ? (int)pitch : -(int)pitch) : 0;
    rl[k].field_shift = fields == 2;
    rl[k].le = v210 ? 1 : v.pl.le; rl[k].lsb = v210 ? 1 : v.pl.lsb;
  }
}
// pack: the staging -> the caller's buffer (an output); else the caller's buffer -> the staging (an input)
static void view_convert(vc2hip_ctx *c, const RawView &v, bool pack) {
  if (!v.packed || !v.stage) return;
  const bool v210 = v.pl.packing == VC2HIP_PACKING_V210;
  const int k = v210 ? 0 : 1; // the caller's plane the kernels convert
  PackedParams p;
  memset(&p, 0, sizeof p);
  p.packed = (uint8_t *)v.base + v.pl.at[k]; p.packed_stride = (long long)v.pl.stride; p.packed_pitch = (int)v.pl.pitch[k];
  for (int q = 0; q < 3; ++q) { p.plane[q] = v.stage + v.sat[q]; p.plane_pitch[q] = (int)v.spitch[q]; }
  p.plane_stride = (long long)v.sstride;
  p.rows = v.pl.rows[k];
  p.width = v210 ? v.width : (int)(v.pl.row[1] / (2 * (size_t)v.word_bytes));
  p.v210 = v210; p.word_bytes = v.word_bytes;
  p.vec = !(((size_t)v.base | v.pl.at[k] | v.pl.stride | v.pl.pitch[k]) & 15);
  vc2_launch_packed(c->L, p, pack, v.n, c->stream);
}

// The decoder's store for n pictures of g: the slice records, behind them the band planes of the finest levels and the
// record heads of the deep ones (planned by a dry run of run_inverse: nothing is launched).  decode_batch_common plans the
// store the slice decoders fill, encode_recon_batch_dev the one the requantise kernel fills for the same inverse kernels.
// job: the inverse transform the store is for (matrix, LL source, destination) -- its band planes, record heads and head
// level are set here; its store is the caller's to set once it is allocated.
struct DecoderLayout {
  BandPlanes bp;
  HeadSplit hs;
  long long sstride; // elements per picture
  unsigned tails;    // levels whose streaming kernel is the TAIL instantiation
};
static void plan_decoder_layout(vc2hip_ctx *c, const Geom &g, int kernel, int n, bool s16, bool plane_path, InverseJob &job, DecoderLayout &lay) {
  // Band planes (vc2hip_internal.h): the finest levels, as long as they go through the streaming inverse kernel, a
  // slice's block row in them is at least 4 coefficients (8: rows that keep 16-byte pieces aligned) and they are not
  // the level whose LL comes from the store.  16-bit store only (the int32 store is the fallback decoder's).
  BandPlanes &bp = lay.bp;
  HeadSplit &hs = lay.hs;
  memset(&lay, 0, sizeof lay);
  const int ns = g.ys * g.xs;
  long long sstride = record_stride(g); // elements per picture: slice records, then band planes
  InversePlan plan = {0, 0, 0};
  if (s16 && !plane_path && (c->allow_planes || c->allow_heads)) { // which kernel each level would run on
    LLPlanes none;
    memset(&none, 0, sizeof none);
    InverseJob dry = job;
    dry.store = Store{nullptr, nullptr, s16, sstride};
    (void)run_inverse(c, g, kernel, n, dry, none, &plan);
  }
  if (s16 && !plane_path && c->allow_planes) {
    const unsigned mask = plan.stream;
    lay.tails = plan.tail;
    for (int k = 0; k < 3; ++k) bp.from[k] = g.c[k].ph ? g.c[k].sh * g.c[k].sw : 0;
    for (int l = 0; l < VC2_BP_MAX && l < g.depth - 1 && (mask >> l & 1); ++l) {
      bool ok = true;
      for (int k = 0; k < 3 && ok; ++k) {
        const CompGeom &cg = g.c[k];
        if (!cg.ph) continue;
        const int bsh = (cg.sh >> l) / 2, bsw = (cg.sw >> l) / 2, ow = (cg.pw >> l) / 2;
        ok = bsh >= 1 && bsw >= 4 && (bsh & (bsh - 1)) == 0 && (bsw & (bsw - 1)) == 0 && ow % (bsw >= 8 ? 8 : 4) == 0 &&
             (bsh * bsw) % 8 == 0;
      }
      if (!ok) break;
      for (int k = 0; k < 3; ++k) {
        const CompGeom &cg = g.c[k];
        if (!cg.ph) continue;
        const int bsh = (cg.sh >> l) / 2, bsw = (cg.sw >> l) / 2;
        bp.np[k][l] = (cg.ph >> l) / 2; bp.ow[k][l] = (cg.pw >> l) / 2;
        bp.lbsh[k][l] = 31 - __builtin_clz(bsh); bp.lbsw[k][l] = 31 - __builtin_clz(bsw);
        bp.base[k][l] = sstride;
        sstride += ((long long)3 * bp.np[k][l] * bp.ow[k][l] + 7) & ~7ll;
        bp.from[k] -= 3 * bsh * bsw;
      }
      bp.levels = l + 1;
    }
    if (sstride >= (1ll << 31)) { memset(&bp, 0, sizeof bp); sstride = record_stride(g); } // 32-bit element offsets
  }
  // Record heads (HeadSplit, vc2hip_internal.h): the levels below the streaming ones, when all of them run on the tile
  // kernels, read their coefficients from dense per-component arrays behind the records (and band planes)
  if (s16 && !plane_path && c->allow_heads) {
    const unsigned smask = plan.stream, fmask = plan.fast;
    int ls = g.depth; // first level of the run of tile-kernel levels that reaches the deepest one
    while (ls > 0 && !(smask >> (ls - 1) & 1) && (fmask >> (ls - 1) & 1)) --ls;
    bool ok = ls >= 1 && ls < g.depth && ls >= bp.levels; // (level 0 keeps its bands where the final kernels expect them)
    for (int k = 0; k < 3 && ok; ++k) {
      if (!g.c[k].ph) continue;
      const int hn = (g.c[k].sh >> ls) * (g.c[k].sw >> ls);
      ok = hn >= 8 && hn % 8 == 0 && hn <= bp.from[k];
    }
    if (ok) {
      long long at = sstride;
      for (int k = 0; k < 3; ++k) {
        if (!g.c[k].ph) continue;
        hs.n[k] = (g.c[k].sh >> ls) * (g.c[k].sw >> ls);
        hs.base[k] = at;
        at += ((long long)ns * hs.n[k] + 7) & ~7ll;
      }
      if (at < (1ll << 31)) { sstride = at; job.head_level = ls; } else memset(&hs, 0, sizeof hs);
    }
  }
  job.bp = &bp;
  job.hs = hs.n[0] ? &hs : nullptr;
  lay.sstride = sstride;
}

// what vc2hip_encode_recon_batch_dev asks for beyond (or instead of) the payload
struct ReconOut {
  void *recon;     // the decoder's picture, or null
  uint64_t *sse;   // n x 3 sums of squared differences against d_raw, or null
  int32_t *qidx;   // n x slices, or null
};
static int encode_batch_common(vc2hip_ctx *c, const Geom &g, const void *d_raw, int fields, int top_first, int n,
                               const vc2hip_picture_format *fb, const vc2hip_picture_format *f, const vc2hip_coding_params *cp,
                               void *d_payload, size_t payload_stride, uint64_t *d_lens, const IndexOffsets &io, const ReconOut *ro = nullptr);
static int run_recon(vc2hip_ctx *c, const Geom &g, const vc2hip_coding_params *cp, int n, const vc2hip_picture_format *f,
                     const PackJob &job, const LdEncParams &lp, const LLPlanes &ll, const struct RawView &in, const ReconOut &ro);

// ---- the front of the six device batch calls -------------------------------------------------------------------------
// Every call refuses what it can see in its arguments here, before it records the fork event or enters the context: a
// refused batch call touches no stream, with one lane or several.  An entry point states its arguments once (batch_args),
// adds the refusals of its own, resolves the caller's layout for the pictures of its buffer (batch_layout), lists its
// buffers (BatchBuf) and hands the work to run_batch, whose callback calls encode_batch_common / decode_batch_common on
// the context or on a lane.  Those two check no argument again.
struct BatchArg {
  const void *p;
  unsigned align; // 16 (pictures, payload), 8 (lengths, squared errors) or 4 (indices) bytes
  bool optional;  // may be null
};
static int batch_args(vc2hip_ctx *c, int n, const vc2hip_picture_format *f, const vc2hip_coding_params *cp, size_t payload_stride,
                      std::initializer_list<BatchArg> args, const char *null_text = nullptr) {
  bool missing = !c || n < 1 || !f || !cp, misaligned = (payload_stride & 15) != 0;
  for (const BatchArg &a : args) {
    missing = missing || (!a.p && !a.optional);
    misaligned = misaligned || ((size_t)a.p & (a.align - 1));
  }
  if (missing) return set_err(c, VC2HIP_EINVAL, null_text);
  if (misaligned) return set_err(c, VC2HIP_EINVAL, "device buffers and the payload stride must be 16-byte aligned");
  if (cp->kernel < 0 || cp->kernel > 6) return set_err(c, VC2HIP_EINVAL, "invalid wavelet kernel");
  return matrix_depth_check(c, cp);
}
// what the three encoding calls refuse in cp; g: the coded picture's geometry
static int encode_check(vc2hip_ctx *c, const vc2hip_picture_format *f, const vc2hip_coding_params *cp, Geom &g) {
  const bool capped = cp->mode == VC2HIP_HQ_CAPPED || cp->mode == VC2HIP_HQ_CAPPED_FILL;
  if (cp->mode != VC2HIP_HQ_CONSTQ && cp->mode != VC2HIP_HQ_CBR && cp->mode != VC2HIP_LD && !capped) return set_err(c, VC2HIP_EINVAL);
  if (capped && (cp->q_index < 0 || cp->q_index > VC2_CAP_Q_TOP || cp->compressed_bytes < 1))
    return set_err(c, VC2HIP_EINVAL, cp->mode == VC2HIP_HQ_CAPPED ? "HQ_CAPPED: q_index 0 .. 115, compressed_bytes >= 1"
                                                                   : "HQ_CAPPED_FILL: q_index 0 .. 115, compressed_bytes >= 1");
  if (cp->mode != VC2HIP_LD && (cp->scalar < 1 || cp->prefix < 0)) return set_err(c, VC2HIP_EINVAL);
  const int rc = picture_geom(g, f, cp, false);
  return rc ? set_err(c, rc) : VC2HIP_OK;
}
// ---- per-slice index offsets (vc2hip_set_index_offsets) ------------------------------------------
extern "C" int vc2hip_set_index_offsets(vc2hip_ctx *c, const int8_t *d_offsets, size_t picture_stride) {
  if (!c) return VC2HIP_EINVAL;
  c->idx_offs = d_offsets;
  c->idx_offs_stride = d_offsets ? picture_stride : 0;
  return VC2HIP_OK;
}
// what the three encoding calls refuse under a map, behind encode_check (g: the coded picture's geometry)
static int offsets_check(vc2hip_ctx *c, const IndexOffsets &io, const vc2hip_coding_params *cp, const Geom &g) {
  if (!io.p) return VC2HIP_OK;
  if (cp->mode != VC2HIP_HQ_CONSTQ && cp->mode != VC2HIP_HQ_CAPPED && cp->mode != VC2HIP_HQ_CAPPED_FILL)
    return set_err(c, VC2HIP_EINVAL, "index offsets are set: only HQ_CONSTQ, HQ_CAPPED and HQ_CAPPED_FILL take them (vc2hip_set_index_offsets(ctx, NULL, 0) clears them)");
  if (cp->q_index < 0 || cp->q_index > VC2_CAP_Q_TOP) return set_err(c, VC2HIP_EINVAL, "index offsets are set: q_index 0 .. 115");
  if (io.stride && io.stride < (size_t)g.ys * g.xs)
    return set_err(c, VC2HIP_EINVAL, "index offsets: picture_stride must be 0 (one map for every picture) or at least y_slices * x_slices");
  return VC2HIP_OK;
}

// vc2hip_encode_batch_dev with the map stated: the context's for the entry point, none for the host-buffer and _begin calls
static int encode_batch_dev(vc2hip_ctx *c, const void *d_raw, int n, const vc2hip_picture_format *f, const vc2hip_coding_params *cp,
                            void *d_payload, size_t payload_stride, uint64_t *d_lens, const IndexOffsets &io) {
  if (int rc = batch_args(c, n, f, cp, payload_stride, {{d_raw, 16}, {d_payload, 16}, {d_lens, 8}})) return rc;
  RawLayout lay;
  if (int rc = batch_layout(c, f, lay)) return rc;
  Geom g;
  if (int rc = encode_check(c, f, cp, g)) return rc;
  if (int rc = offsets_check(c, io, cp, g)) return rc;
  const BatchBuf bufs[] = {{d_raw, lay.stride, false}, {d_payload, payload_stride, true}, {d_lens, 8, true}, {io.p, io.stride, false}};
  return run_batch(c, n, bufs, [&](vc2hip_ctx *l, int count, void *const *at) {
    return encode_batch_common(l, g, at[0], 1, 1, count, f, f, cp, at[1], payload_stride, (uint64_t *)at[2], {(const int8_t *)at[3], io.stride});
  });
}
extern "C" int vc2hip_encode_batch_dev(vc2hip_ctx *c, const void *d_raw, int n, const vc2hip_picture_format *f,
                                       const vc2hip_coding_params *cp, void *d_payload, size_t payload_stride,
                                       uint64_t *d_lens) {
  return encode_batch_dev(c, d_raw, n, f, cp, d_payload, payload_stride, d_lens, c ? IndexOffsets{c->idx_offs, c->idx_offs_stride} : IndexOffsets{nullptr, 0});
}

extern "C" int vc2hip_encode_recon_batch_dev(vc2hip_ctx *c, const void *d_raw, int n, const vc2hip_picture_format *f,
                                             const vc2hip_coding_params *cp, void *d_payload, size_t payload_stride, uint64_t *d_lens,
                                             void *d_recon, uint64_t *d_sse, int32_t *d_qidx) {
  if (int rc = batch_args(c, n, f, cp, payload_stride,
                          {{d_raw, 16}, {d_payload, 16, true}, {d_lens, 8, true}, {d_recon, 16, true}, {d_sse, 8, true}, {d_qidx, 4, true}})) return rc;
  if (!d_payload && !d_recon && !d_sse && !d_qidx) return set_err(c, VC2HIP_EINVAL, "no output asked for");
  if (d_sse && !d_recon) return set_err(c, VC2HIP_EINVAL, "d_sse needs d_recon");
  if ((d_payload != nullptr) != (payload_stride != 0) || (d_payload != nullptr) != (d_lens != nullptr))
    return set_err(c, VC2HIP_EINVAL, "d_payload, payload_stride and d_lens: all or none");
  RawLayout lay; // one layout for d_raw and d_recon
  if (int rc = batch_layout(c, f, lay)) return rc;
  Geom ge;
  if (int rc = encode_check(c, f, cp, ge)) return rc;
  const IndexOffsets io = {c->idx_offs, c->idx_offs_stride};
  if (int rc = offsets_check(c, io, cp, ge)) return rc;
  if (d_recon) {
    const size_t span = (size_t)(n - 1) * lay.stride + lay.extent; // (the file format: n * vc2hip_raw_picture_bytes)
    const uint8_t *raw8 = (const uint8_t *)d_raw, *rec8 = (const uint8_t *)d_recon;
    if (rec8 < raw8 + span && raw8 < rec8 + span)
      return set_err(c, VC2HIP_EINVAL, "d_recon overlaps d_raw (the squared error reads the input after the reconstruction is written)");
    if (f->chroma_bit_depth && f->chroma_bit_depth != f->bit_depth)
      return set_err(c, VC2HIP_EINVAL, "the decoder has one bit depth: chroma_bit_depth must be 0 or bit_depth with d_recon");
    Geom gd; // (the decoder derives the chroma planes from the padded luma plane, DecodeStream.cpp:483-498)
    if (picture_geom(gd, f, cp, true)) return set_err(c, VC2HIP_EINVAL);
    for (int k = 0; k < 3; ++k)
      if (gd.c[k].ph != ge.c[k].ph || gd.c[k].pw != ge.c[k].pw)
        return set_err(c, VC2HIP_EINVAL, "the decoder's padded chroma planes differ from the encoder's: no decoder shows this picture");
  }
  const BatchBuf bufs[] = {{d_raw, lay.stride, false}, {d_payload, payload_stride, true}, {d_lens, 8, true},
                           {d_recon, lay.stride, true}, {d_sse, 24, true}, {d_qidx, (size_t)ge.ys * ge.xs * 4, true},
                           {io.p, io.stride, false}};
  return run_batch(c, n, bufs, [&](vc2hip_ctx *l, int count, void *const *at) {
    const ReconOut ro = {at[3], (uint64_t *)at[4], (int32_t *)at[5]};
    return encode_batch_common(l, ge, at[0], 1, 1, count, f, f, cp, at[1], payload_stride, (uint64_t *)at[2], {(const int8_t *)at[6], io.stride}, &ro);
  });
}

// n coded pictures of geometry g and sample format f -> payload slots.  fb: the format of the pictures in d_raw, which are
// the coded pictures (fields 1) or the interleaved frames whose fields they are (fields 2, n / 2 frames: raw_planes).
// ro (vc2hip_encode_recon_batch_dev): d_payload may be null -- no slice coder runs then -- and run_recon follows the coder.
// The arguments are the entry point's, checked there.
static int encode_batch_common(vc2hip_ctx *c, const Geom &g, const void *d_raw, int fields, int top_first, int n,
                               const vc2hip_picture_format *fb, const vc2hip_picture_format *f, const vc2hip_coding_params *cp,
                               void *d_payload, size_t payload_stride, uint64_t *d_lens, const IndexOffsets &io, const ReconOut *ro) {
  ENTER(c);
  int rc;
  const int ns = g.ys * g.xs;
  int32_t qm[VC2_MAX_BANDS];
  if ((rc = effective_matrix(c, cp, qm))) return rc;
  const bool s16 = cp->mode != VC2HIP_LD && use_store16(c, g, cp->kernel);
  int32_t *d_store, *d_ll, *d_q, *d_storew = nullptr, *d_llw = nullptr;
  NEED(c, B_STORE, (size_t)n * ns * g.slice_coefs * 4, d_store); // 16-bit elements use the first half
  NEED(c, B_LL0, ll_bytes(g, n) + 16, d_ll);
  if (s16) { // touched only by values outside 16 bits
    NEED(c, B_STOREW, (size_t)n * ns * g.slice_coefs * 4, d_storew);
    NEED(c, B_LLW, ll_bytes(g, n) + 16, d_llw);
  }
  NEED(c, B_QIDX, (size_t)n * ns * 4, d_q);
  const Store st = {d_store, d_storew, s16, record_stride(g)};
  LLPlanes ll;
  ll_layout(g, n, d_ll, s16 ? 2 : 4, d_llw, ll);
  const void *src[3]; RawPlane ss[3];
  RawView in;
  if ((rc = raw_view(c, fb, n / fields, d_raw, B_PKIN, in))) return rc;
  view_convert(c, in, false);
  view_planes(in, fb, fields, top_first, src, ss);
  if (needs_plane_path(c, g, cp->kernel)) { // (a slice beyond any LDS tile: HQ and LD alike -- the store is int32 then)
    if ((rc = plane_forward(c, g, cp->kernel, n, src, ss, f, d_store))) return rc;
  } else if ((rc = run_forward(c, g, cp->kernel, n, src, ss, true, f, st, ll))) return rc;
  const bool ld = cp->mode == VC2HIP_LD, cbr = cp->mode == VC2HIP_HQ_CBR;
  Budgets b = {};
  if (ld) rc = budget_tables(c, g.ys, g.xs, cp->compressed_bytes, 1, LD_BUDGETS, b);
  else if (cbr) rc = budget_tables(c, g.ys, g.xs, cp->compressed_bytes, cp->scalar, cp->prefix, b);
  if (rc) return rc;
  // a slot holds the budgets' sum, or whatever a slice's three length bytes can describe
  const size_t slot_bytes = b.bytes ? (size_t)b.total : vc2hip_max_payload_bytes(f, cp);
  if (d_payload && payload_stride < slot_bytes) return set_err(c, VC2HIP_ECAP);
  LdEncParams lp;
  if (ld) { // EncodeStream.cpp:141-245, :195-244
    c->ld_batch = n;
    if ((rc = fill_ld_enc(c, lp, g, st, d_q, qm, ll, b, cp->compressed_bytes / ns + 5, (uint8_t *)d_payload,
                          (long long)payload_stride))) return rc;
    lp.search = 1;
    vc2_launch_ld_quantise(c->L, lp, n, c->stream);
    if (d_payload) {
      vc2_launch_ld_pack(c->L, lp, n, c->stream);
      vc2_launch_fill_u64(c->L, (unsigned long long *)d_lens, b.total, (size_t)n, c->stream);
    }
  } else if (cbr) {
    CbrParams p;
    fill_cbr(p, g, st, d_q, b.bytes, cp->scalar, qm, c->cbr_general, c->d_err);
    vc2_launch_cbr(c->L, p, n, c->stream);
  } else if (cp->mode == VC2HIP_HQ_CAPPED || cp->mode == VC2HIP_HQ_CAPPED_FILL) {
    // one index per picture, found on the device (vc2hip_cap.h); HQ_CAPPED_FILL: then q_i - 1 in as
    // many slices as the cap's spare bytes pay for (section 28: the cost buffer switches the third round and the fill on)
    CapParams p;
    memset(&p, 0, sizeof p);
    NEED(c, B_CAPTAB, (size_t)n * VC2_CAP_ROW * 8, p.table);
    if (cp->mode == VC2HIP_HQ_CAPPED_FILL) NEED(c, B_CAPCOST, (size_t)n * ns * 4, p.cost);
    HIPCHK(c, hipMemsetAsync(p.table, 0, (size_t)n * VC2_CAP_ROW * 8, c->stream));
    fill_cbr(p.s, g, st, d_q, b.bytes, cp->scalar, qm, c->cap_general, c->d_err); // (no budgets: the cap is the picture's)
    p.prefix = cp->prefix; p.floor = cp->q_index; p.cap = (unsigned long long)cp->compressed_bytes;
    p.offs = io.p; p.offs_stride = (long long)io.stride; // (the base b_i is searched, slice s measured and coded at e_s(b_i))
    vc2_launch_cap(c->L, p, n, c->stream);
  } else if (io.p) {
    vc2_launch_q_offsets(c->L, d_q, io.p, (long long)io.stride, cp->q_index, ns, n, c->stream);
  } else {
    // quantIndicesConstQ, EncodeStream.cpp:128-138
    vc2_launch_fill_i32(c->L, d_q, cp->q_index, (size_t)n * ns, c->stream);
  }
  PackJob job; // what the coder is handed: run_pack codes it (LD's slices are written above), run_recon decodes it
  job.store = st; job.qidx = d_q; job.qm = qm;
  job.prefix = cp->prefix; job.scalar = cp->scalar; job.budgets = b;
  job.payload = (uint8_t *)d_payload; job.stride = (long long)payload_stride; job.lens = (unsigned long long *)d_lens;
  if (d_payload && !ld && (rc = run_pack(c, g, n, job))) return rc;
  return ro ? run_recon(c, g, cp, n, f, job, lp, ll, in, *ro) : VC2HIP_OK;
}

// A squared-error job over the pictures of a and b, which lie in one layout: the sample words here, the components by sse_comp
static void sse_job(SseParams &p, const vc2hip_picture_format *f, int le, int lsb, const void *a, const void *b, size_t pic_bytes, uint64_t *sse) {
  memset(&p, 0, sizeof p);
  p.a = (const uint8_t *)a; p.b = (const uint8_t *)b; p.pic_bytes = (long long)pic_bytes;
  p.word_bytes = f->word_bytes; p.shift = lsb ? 0 : 8 * f->word_bytes - f->bit_depth;
  p.mask = f->bit_depth < 32 ? (1u << f->bit_depth) - 1 : ~0u;
  p.le = le;
  p.sse = (unsigned long long *)sse;
}
// component k of the job: its first row `at` bytes into a picture, its rows `pitch` bytes apart
static void sse_comp(SseParams &p, int k, const CompGeom &cg, size_t at, size_t pitch) {
  const long long row = (long long)cg.w * p.word_bytes;
  const bool tight = (long long)pitch == row; // one run of bytes: the kernel's "one row"
  p.comp_at[k] = (long long)at;
  p.rows[k] = tight ? 1 : cg.h;
  p.row_bytes[k] = tight ? row * cg.h : row;
  p.pitch[k] = (long long)pitch;
}

// What follows the slice coder in vc2hip_encode_recon_batch_dev: the indices, the decoder's picture from the quantised
// coefficients (no payload is read: DESIGN.md section 12), the squared error.  HQ: d_store holds transform coefficients,
// which k_requantise turns into the decoder's store; LD: vc2_launch_ld_quantise left quantised values with LL residuals in
// it, which is what the decoder's slice reader leaves.  job: the slice coder's, with no payload where none was written --
// the coder's checks are made here then; lp: LD's search job (set for LD pictures only).
static int run_recon(vc2hip_ctx *c, const Geom &g, const vc2hip_coding_params *cp, int n, const vc2hip_picture_format *f,
                     const PackJob &job, const LdEncParams &lp, const LLPlanes &ll, const RawView &in, const ReconOut &ro) {
  const int ns = g.ys * g.xs;
  const Store &st = job.store;
  const int32_t *const qm = job.qm, *const d_q = job.qidx;
  const bool s16 = st.s16, ld = cp->mode == VC2HIP_LD, check = !job.payload;
  int rc;
  if (ro.qidx) HIPCHK(c, hipMemcpyAsync(ro.qidx, d_q, (size_t)n * ns * 4, hipMemcpyDeviceToDevice, c->stream));
  const void *dstc[3]; RawPlane ds[3];
  RawView out;
  if ((rc = raw_view(c, f, n, ro.recon, B_PKOUT, out))) return rc;
  view_planes(out, f, 1, 1, dstc, ds);
  void *dst[3] = {(void *)dstc[0], (void *)dstc[1], (void *)dstc[2]};
  const bool plane_path = needs_plane_path(c, g, cp->kernel);
  InverseJob inv; // the decoder's inverse transform of the store the branches below leave
  inv.qidx = d_q; inv.qm = qm;
  inv.dst = dst; inv.dst_l = ds; inv.f = f;
  DecoderLayout lay; // (HQ)
  if (ld) {
    if (check) vc2_launch_ld_check(c->L, lp, n, c->stream);
    if (ro.recon) ld_restore_ll(c, g, n, st, d_q, qm[0], ll);
    inv.store = st; inv.ll_ready = true;
  } else if (ro.recon || check) {
    // the decoder's layout, as decode_batch_common plans it for the same pictures (16-bit band planes: the byte form
    // follows the statistics of a context's previous decode batch, which this call neither reads nor changes)
    plan_decoder_layout(c, g, cp->kernel, n, s16, plane_path, inv, lay);
    int32_t *d_rs = nullptr, *d_rsw = nullptr;
    if (ro.recon) {
      NEED(c, B_RSTORE, (size_t)n * (size_t)lay.sstride * (s16 ? 2 : 4), d_rs);
      if (s16) NEED(c, B_RSTOREW, (size_t)n * (size_t)lay.sstride * 4, d_rsw);
    }
    RequantParams p;
    memset(&p, 0, sizeof p);
    p.src = st.p; p.src_wide = st.wide; p.src_stride = st.stride;
    p.dst = d_rs; p.dst_wide = d_rsw; p.dst_stride = lay.sstride;
    p.store16 = s16; p.qidx = d_q; p.n_slices = ns; p.slice_coefs = g.slice_coefs; p.xs = g.xs;
    fill_comp_arrays(g, p.comp_n, p.comp_off, p.comp_n0);
    p.n_bands = 3 * g.depth + 1;
    for (int i = 0; i < p.n_bands; ++i) p.qmatrix[i] = qm[i];
    p.bp = lay.bp; p.hs = lay.hs;
    p.check = check; p.scalar = cp->scalar; p.cbr_bytes = job.budgets.bytes; p.err = c->d_err;
    vc2_launch_requantise(c->L, p, n, c->stream);
    inv.store = Store{d_rs, d_rsw, s16, lay.sstride};
  }
  if (ro.recon) {
    if (plane_path) rc = plane_inverse(c, g, cp->kernel, n, (const int32_t *)inv.store.p, d_q, qm, dst, ds, f, ld ? &ll : nullptr);
    else rc = run_inverse(c, g, cp->kernel, n, inv, ll);
    if (rc) return rc;
    view_convert(c, out, true);
  }
  if (!ro.sse) return VC2HIP_OK;
  HIPCHK(c, hipMemsetAsync(ro.sse, 0, (size_t)n * 3 * 8, c->stream));
  vc2_prof_break(c->L);
  SseParams p;
  if (out.packed) { // the two stagings (semi-planar: the Y planes where they are, in a launch of their own)
    const bool v210 = out.pl.packing == VC2HIP_PACKING_V210;
    const int le = v210 ? 1 : out.pl.le, lsb = v210 ? 1 : out.pl.lsb;
    sse_job(p, f, le, lsb, in.stage, out.stage, out.sstride, ro.sse);
    for (int k = v210 ? 0 : 1; k < 3; ++k) sse_comp(p, k, g.c[k], out.sat[k], out.spitch[k]);
    vc2_launch_squared_error(c->L, p, n, c->stream);
    if (v210) return VC2HIP_OK;
    sse_job(p, f, le, lsb, in.base, out.base, out.pl.stride, ro.sse);
    sse_comp(p, 0, g.c[0], out.pl.at[0], out.pl.pitch[0]);
  } else {
    RawLayout rl;
    (void)resolve_layout(f, active_layout(c), rl); // (refused at the entry point)
    sse_job(p, f, rl.le, rl.lsb, in.base, ro.recon, rl.stride, ro.sse);
    for (int k = 0; k < 3; ++k) sse_comp(p, k, g.c[k], rl.at[k], rl.pitch[k]);
  }
  vc2_launch_squared_error(c->L, p, n, c->stream);
  return VC2HIP_OK;
}

// HQ_CBR pictures on the decoding side: the caller says CBR, so the budgets predict the slice offsets (the claim that
// vc2_launch_cbr_index verifies).  The budget tables of cp; none where cp is not HQ_CBR, the context never claims
// (VC2HIP_FLAG_NO_CBR_INDEX) or the tables could not be made: the general index then works alone.
static Budgets cbr_claim_tables(vc2hip_ctx *c, const Geom &g, const vc2hip_coding_params *cp) {
  Budgets b = {};
  if (cp->mode == VC2HIP_HQ_CBR && cp->compressed_bytes > 0 && c->allow_cbr_index)
    (void)budget_tables(c, g.ys, g.xs, cp->compressed_bytes, cp->scalar, cp->prefix, b); // (a failure leaves b empty)
  return b;
}

// One byte per band-plane coefficient for this batch?  What the previous batch of this context looked like decides (its
// lengths and its escape count arrive through pinned memory behind an event: no wait here): small coefficients <=> few
// payload bits per sample.  The planes keep their places and their wide elements: only the bytes of a plane's narrow
// elements halve.  levels, tails: of the batch's band planes (DecoderLayout).
static bool choose_bytes8(vc2hip_ctx *c, bool capturing, int levels, unsigned tails) {
  // (the context's FIRST look is waited for -- once, at its second batch, while the first is all the GPU has to do
  // anyway: a caller that never synchronises between batches would otherwise keep the 16-bit planes for as long as it
  // runs ahead of the GPU; every later look is only taken when it has arrived.  Never on a caller's stream
  // (vc2hip_create_on_stream): that caller may be capturing a graph or deliberately running ahead of the GPU -- there
  // the look is only ever queried, and VC2HIP_FLAG_PLANES8_ALWAYS / _NEVER make the choice deterministic: include/vc2hip.h.
  // The lanes of such a context follow the same rule.  During a capture the look is not even queried: the form a
  // captured call is planned with is the one the context had when the capture began)
  if (c->stat_pending && !c->stat_seen && !c->follows_caller) (void)hipEventSynchronize(c->stat_ev);
  if (c->stat_pending && !capturing && hipEventQuery(c->stat_ev) == hipSuccess) {
    c->stat_pending = false;
    c->stat_seen = true;
    double bytes = 0;
    for (int k = 0; k < c->stat_n; ++k) bytes += (double)c->h_stat[1 + k];
    const double bits = c->stat_n ? 8.0 * bytes / (c->stat_n * c->stat_samples) : 99.0;
    // (pieces of eight coefficients; counted over ALL pictures of the batch, not only the stat_n whose lengths were copied)
    const double esc = (double)c->h_stat[0] * 8.0 / (std::max(1, c->stat_n_total) * c->stat_samples);
#ifdef VC2HIP_ABLATE
    if (getenv("VC2HIP_PLANES8_DEBUG")) fprintf(stderr, "planes8: previous batch %d pictures, %.2f payload bits per sample, %s planes, escape pieces %.4f%%\n", c->stat_n, bits, c->stat_was8 ? "byte" : "16-bit", 100 * esc);
#endif
    if (c->stat_was8 && esc > 0.005) c->planes8_on = false;       // more than 0.5 % of the pieces carried an escape
    else if (!c->stat_was8 || esc < 0.002) c->planes8_on = bits < (c->planes8_on ? 6.5 : 6.0);
  }
  bool b8 = c->planes8_mode == 1 || (c->planes8_mode == 0 && c->planes8_on);
  for (int l = 0; l < levels; ++l) if (tails >> l & 1) b8 = false; // (the TAIL instantiations read 16-bit planes only)
  return b8;
}
// The HQ slice reader's launch, and where the next call's choice is open this batch's escape count and payload lengths for
// it.  samples: of one coded picture
static int unpack_and_look(vc2hip_ctx *c, const UnpackParams &p, int n, bool capturing, double samples) {
  // (no look while the stream is being captured into a graph: the copies and the event would become graph nodes and the
  // event could never be queried)
  const bool look = p.bp.levels && c->planes8_mode == 0 && !c->stat_pending && !capturing;
  if (look) HIPCHK(c, hipMemsetAsync(c->d_stat, 0, 8, c->stream));
  vc2_launch_unpack(c->L, p, n, c->stream);
  if (!look) return VC2HIP_OK;
  c->stat_n = std::min(n, 60);
  c->stat_n_total = n;
  c->stat_samples = samples;
  c->stat_was8 = p.bp.bytes8 != 0;
  HIPCHK(c, hipMemcpyAsync(c->h_stat, c->d_stat, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->h_stat + 1, p.lens, (size_t)c->stat_n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(c->stat_ev, c->stream));
  c->stat_pending = true;
  return VC2HIP_OK;
}

// n coded pictures in payload slots -> the pictures of d_raw_out, whose format is fb: the coded pictures (fields 1), the
// interleaved frames whose fields they are (fields 2, n / 2 frames), or -- drop > 0 -- the pictures at 1 / 2^drop size.
// g: the geometry the level kernels run on; f: the sample format.  The arguments are the entry point's, checked there.
//
// A reduced picture (vc2hip_decode_reduced_batch_dev): without its `drop` finest levels the coded
// picture IS a picture of depth - drop levels whose planes and slices are 2^drop times smaller each way, on the same
// slice grid, with the first 3 (depth - drop) + 1 entries of the quantisation matrix (it is ordered coarse to fine).
// g is that picture's: store layout, band planes, record heads and level kernels are planned for it as for any other.
// What is left of the coded one: where a slice's bytes are (the index kernels walk length bytes, and the slice decoders
// find a component by them, read its first sh * sw coefficients and leave), and the low-pass gain of the dropped levels,
// which the launch that writes the raw words takes out (LevelParams::norm_shift).
static int decode_batch_common(vc2hip_ctx *c, const Geom &g, const void *d_payload, size_t payload_stride, const uint64_t *d_lens, int n,
                               const vc2hip_picture_format *fb, const vc2hip_picture_format *f, const vc2hip_coding_params *cp,
                               void *d_raw_out, bool ld, int fields = 1, int top_first = 1, int drop = 0) {
  ENTER(c);
  int rc;
  const int ns = g.ys * g.xs;
  int32_t qm[VC2_MAX_BANDS];
  if ((rc = effective_matrix(c, cp, qm))) return rc;
  const int norm_shift = drop * (cp->kernel == VC2HIP_HAAR0 ? 0 : cp->kernel == VC2HIP_FIDELITY ? 2 : 1);
  const bool s16 = !ld && use_store16(c, g, cp->kernel);
  const void *dstc[3]; RawPlane ds[3];
  RawView out;
  if ((rc = raw_view(c, fb, n / fields, d_raw_out, B_PKOUT, out))) return rc;
  view_planes(out, fb, fields, top_first, dstc, ds);
  void *dst[3] = {(void *)dstc[0], (void *)dstc[1], (void *)dstc[2]};
  const bool plane_path = needs_plane_path(c, g, cp->kernel);
  InverseJob inv; // (its store and indices follow their allocation)
  inv.qm = qm; inv.ll_ready = ld;
  inv.norm_shift = norm_shift; inv.level_base = drop;
  inv.dst = dst; inv.dst_l = ds; inv.f = f;
  DecoderLayout lay;
  plan_decoder_layout(c, g, cp->kernel, n, s16, plane_path, inv, lay);
  BandPlanes &bp = lay.bp;
  long long sstride = lay.sstride;
  // Is the stream being captured into a graph?  Asked of every context a caller's stream can pull into its capture: one
  // made on that stream, and the lanes of one (their own streams join the capture at the fork event).
  bool capturing = false;
  if (c->follows_caller && !ld) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    capturing = hipStreamIsCapturing(c->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
  }
  if (bp.levels) bp.bytes8 = choose_bytes8(c, capturing, bp.levels, lay.tails);
  int32_t *d_store, *d_ll, *d_q, *d_storew = nullptr, *d_llw = nullptr;
  {
    static const int pad = vc2_tune_int("VC2HIP_DEC_STORE_PAD", 0); // (experiment: elements between the pictures' stores; a multiple of 8)
    if (s16 && pad > 0 && sstride + pad < (1ll << 31)) sstride += pad & ~7;
  }
  NEED(c, B_STORE, std::max((size_t)n * ns * g.slice_coefs * 4, (size_t)n * (size_t)sstride * 2), d_store); // (16-bit elements: records, band planes and record heads)
  NEED(c, B_LL0, ll_bytes(g, n) + 16, d_ll);
  if (s16) {
    NEED(c, B_STOREW, (size_t)n * sstride * 4, d_storew);
    NEED(c, B_LLW, ll_bytes(g, n) + 16, d_llw);
  }
  NEED(c, B_QIDX, (size_t)n * ns * 4, d_q);
  const Store st = {d_store, d_storew, s16, sstride};
  LLPlanes ll;
  ll_layout(g, n, d_ll, s16 ? 2 : 4, d_llw, ll);
  if (!ld) {
    uint32_t *d_offs;
    if ((rc = build_index(c, (const uint8_t *)d_payload, (long long)payload_stride, (const unsigned long long *)d_lens, n, ns,
                          cp->prefix, cp->scalar, &d_offs, cbr_claim_tables(c, g, cp)))) return rc;
    UnpackParams p;
    fill_unpack(p, g, (const uint8_t *)d_payload, (long long)payload_stride, (const unsigned long long *)d_lens, d_offs, st, d_q,
                cp->prefix, cp->scalar, c->d_err);
    p.bp = bp; p.hs = lay.hs; p.xs = g.xs;
    c->last_plane_bits = bp.levels ? (bp.bytes8 ? 8 : 16) : 0;
    p.stats = c->d_stat;
    double samples = 0;
    for (int k = 0; k < 3; ++k) samples += (double)g.c[k].h * g.c[k].w * (1 << (2 * drop)); // (the payload is the coded picture's)
    if ((rc = unpack_and_look(c, p, n, capturing, samples))) return rc;
  } else {
    Budgets b;
    if ((rc = budget_tables(c, g.ys, g.xs, cp->compressed_bytes, 1, LD_BUDGETS, b))) return rc;
    if (b.total > payload_stride) return set_err(c, VC2HIP_ESTREAM);
    LdUnpackParams p;
    fill_ld_unpack(p, g, (const uint8_t *)d_payload, (long long)payload_stride, b, st, d_q, c->d_err);
    // slices whose luma length exceeds the slice (corrupt pictures): flag, serial walk, second pass (LdUnpackParams)
    unsigned *d_shifted; uint32_t *d_starts;
    NEED(c, B_SIZES, (size_t)n * 4, d_shifted);
    NEED(c, B_OFFS, (size_t)n * ns * 4, d_starts);
    int flag_fill = 0;
#ifdef VC2HIP_ABLATE
    if (getenv("VC2HIP_DEBUG_LD_REDO")) flag_fill = 1; // every picture takes the walk and the second pass (tests of that path on valid streams)
#endif
    HIPCHK(c, hipMemsetAsync(d_shifted, flag_fill, (size_t)n * 4, c->stream));
    vc2_prof_break(c->L);
    p.lens = (const unsigned long long *)d_lens; p.shifted = d_shifted; p.starts = d_starts;
    vc2_launch_ld_unpack(c->L, p, n, c->stream);
    vc2_launch_ld_walk(c->L, p, n, c->stream);
    p.redo = 1;
    vc2_launch_ld_unpack(c->L, p, n, c->stream);
    ld_restore_ll(c, g, n, st, d_q, qm[0], ll);
  }
  inv.store = st; inv.qidx = d_q;
  if (plane_path) rc = plane_inverse(c, g, cp->kernel, n, d_store, d_q, qm, dst, ds, f, ld ? &ll : nullptr, norm_shift, drop);
  else rc = run_inverse(c, g, cp->kernel, n, inv, ll);
  if (!rc) view_convert(c, out, true);
  return rc;
}

extern "C" int vc2hip_band_plane_bits(const vc2hip_ctx *c) { return c ? c->last_plane_bits : 0; }

// ------------------------------------------------------------------------------------------
// VC-2 streams in device memory (vc2hip_stream.hip)
// ------------------------------------------------------------------------------------------
namespace {
struct HeaderBits { // MSB-first writer of DataUnit.cpp's BitWriter
  uint8_t *out;
  size_t cap, pos = 0;
  unsigned cache = 0;
  int cached = 0;
  void bit(unsigned b) {
    cache = (cache << 1) | (b & 1);
    if (++cached == 8) { if (pos < cap) out[pos] = (uint8_t)cache; ++pos; cache = 0; cached = 0; }
  }
  void uvlc(uint32_t v) { // interleaved exp-Golomb (VLC.cpp:21-52)
    const unsigned long long x = (unsigned long long)v + 1;
    int top = 63;
    while (!(x >> top & 1)) --top;
    for (int i = top - 1; i >= 0; --i) { bit(0); bit((unsigned)(x >> i) & 1); }
    bit(1);
  }
  void align() { while (cached) bit(0); }
};
bool stream_cp_ok(const vc2hip_coding_params *cp) {
  if (!cp || cp->kernel < 0 || cp->kernel > 6 || cp->depth < 0 || cp->y_slices < 1 || cp->x_slices < 1) return false;
  if (cp->mode == VC2HIP_LD) return cp->compressed_bytes > 0;
  return (cp->mode == VC2HIP_HQ_CONSTQ || cp->mode == VC2HIP_HQ_CBR || cp->mode == VC2HIP_HQ_CAPPED || cp->mode == VC2HIP_HQ_CAPPED_FILL) && cp->prefix >= 0 && cp->scalar >= 1;
}
// what the transform parameters carry after the slice counts: prefix, scalar (HQ) or the slice-bytes fraction in lowest
// terms (LD: utils::rationalise(pictureBytes, slices), EncodeStream.cpp:263)
void stream_ab(const vc2hip_coding_params *cp, uint32_t *a, uint32_t *b) {
  if (cp->mode != VC2HIP_LD) { *a = (uint32_t)cp->prefix; *b = (uint32_t)cp->scalar; return; }
  const int ns = cp->y_slices * cp->x_slices, g = gcd_i(cp->compressed_bytes, ns);
  *a = (uint32_t)(cp->compressed_bytes / g);
  *b = (uint32_t)(ns / g);
}
} // namespace

extern "C" int vc2hip_picture_header_qm(const vc2hip_coding_params *cp, int major_version, uint32_t picture_number,
                                        const int32_t *matrix, int depth, uint8_t *out, size_t cap, size_t *len) {
  if (!stream_cp_ok(cp) || major_version < 1 || !len || (cap && !out)) return VC2HIP_EINVAL;
  if (matrix) {
    if (depth != cp->depth || depth < 1 || depth > VC2_MAX_DEPTH) return VC2HIP_EINVAL;
    for (int i = 0; i < 3 * depth + 1; ++i) if (matrix[i] < 0 || matrix[i] > 255) return VC2HIP_EINVAL;
  }
  uint32_t a, b;
  stream_ab(cp, &a, &b);
  HeaderBits w{out, cap};
  for (int i = 24; i >= 0; i -= 8) for (int k = 7; k >= 0; --k) w.bit(picture_number >> (i + k)); // DataUnit.cpp: putBytes(4)
  w.uvlc((uint32_t)cp->kernel);
  w.uvlc((uint32_t)cp->depth);
  if (major_version >= 3) { w.bit(0); w.bit(0); } // asym_transform_index_flag, asym_transform_flag
  w.uvlc((uint32_t)cp->x_slices);
  w.uvlc((uint32_t)cp->y_slices);
  w.uvlc(a);
  w.uvlc(b);
  w.bit(matrix ? 1 : 0); // custom_quant_matrix, then its entries: LL, then HL, LH, HH per level from the coarsest (DataUnit.cpp:1403)
  if (matrix) for (int i = 0; i < 3 * depth + 1; ++i) w.uvlc((uint32_t)matrix[i]);
  w.align();
  *len = w.pos;
  return w.pos > cap ? VC2HIP_ECAP : VC2HIP_OK;
}
extern "C" int vc2hip_picture_header(const vc2hip_coding_params *cp, int major_version, uint32_t picture_number, uint8_t *out,
                                     size_t cap, size_t *len) {
  return vc2hip_picture_header_qm(cp, major_version, picture_number, nullptr, 0, out, cap, len);
}

// The inverse of vc2hip_picture_header_qm on the host: the bit syntax k_stream_walk reads (vc2hip_stream.hip).  The two differ
// in what they do with the values: the walk compares 32-bit fields with the caller's cp and takes an LD fraction in any terms;
// this function has to return them in a vc2hip_coding_params, whose members are ints, so a slice count, prefix, scalar or LD
// numerator / denominator of 2^31 or more is VC2HIP_ESYNTAX here (include/vc2hip.h says so).
extern "C" int vc2hip_parse_picture_header(const uint8_t *bytes, size_t len, int major_version, int is_ld, vc2hip_coding_params *cp_out,
                                           int32_t *matrix_out, int matrix_cap, int *entries_out, size_t *consumed) {
  if (!bytes || !cp_out || !entries_out || major_version < 1 || matrix_cap < 0 || (matrix_cap && !matrix_out)) return VC2HIP_EINVAL;
  size_t pos = 32; // bits; the picture number
  bool over = len < 4;
  auto bit = [&]() -> unsigned {
    if ((pos >> 3) >= len) { over = true; return 1; } // (ones past the end: every code below ends)
    const unsigned v = bytes[pos >> 3] >> (7 - (pos & 7)) & 1;
    ++pos;
    return v;
  };
  auto uvlc = [&]() -> uint32_t {
    unsigned long long v = 1;
    for (int n = 0; !bit(); ++n) {
      if (n == 32) { over = true; break; }
      v = (v << 1) | bit();
    }
    return (uint32_t)(v - 1);
  };
  const uint32_t kernel = uvlc(), depth = uvlc();
  bool asym = false;
  if (major_version >= 3) {
    if (bit()) asym |= uvlc() != kernel; // asym_transform_index_flag: wavelet_index_ho
    if (bit()) asym |= uvlc() != 0;      // asym_transform_flag: dwt_depth_ho
  }
  const uint32_t xs = uvlc(), ys = uvlc(), a = uvlc(), b = uvlc();
  const bool custom = bit() && !over;
  if (over || asym || kernel > 6 || depth > 30 || (xs | ys | a | b) >> 31) return VC2HIP_ESYNTAX;
  int entries = 0;
  if (custom) {
    if (depth > VC2_MAX_DEPTH) return VC2HIP_ESYNTAX;
    entries = 3 * (int)depth + 1;
    for (int i = 0; i < entries; ++i) {
      const uint32_t m = uvlc();
      if (over || m > 255) return VC2HIP_ESYNTAX;
      if (i < matrix_cap) matrix_out[i] = (int32_t)m;
    }
  }
  memset(cp_out, 0, sizeof *cp_out);
  cp_out->kernel = (int)kernel; cp_out->depth = (int)depth; cp_out->x_slices = (int)xs; cp_out->y_slices = (int)ys;
  if (is_ld) { // the slice-bytes fraction a / b: the picture's bytes when b divides a * slices
    const unsigned long long num = (unsigned long long)a * xs * ys;
    if (!b || num % b || num / b > 0x7FFFFFFFull) return VC2HIP_ESYNTAX;
    cp_out->mode = VC2HIP_LD; cp_out->compressed_bytes = (int)(num / b);
  } else {
    cp_out->mode = VC2HIP_HQ_CONSTQ; cp_out->prefix = (int)a; cp_out->scalar = (int)b;
  }
  *entries_out = entries;
  if (consumed) *consumed = (pos + 7) >> 3;
  return entries > matrix_cap ? VC2HIP_ECAP : VC2HIP_OK;
}

extern "C" int vc2hip_stream_write_dev(vc2hip_ctx *c, const void *d_payload, size_t payload_stride, const uint64_t *d_lens, int n,
                                       const vc2hip_coding_params *cp, const vc2hip_stream_params *sp, uint8_t *d_stream,
                                       size_t cap, uint64_t *d_stream_len) {
  if (!c || !d_payload || !d_lens || n < 1 || !cp || !sp || !d_stream || !d_stream_len) return set_err(c, VC2HIP_EINVAL);
  if (((size_t)d_payload | payload_stride | (size_t)d_stream) & 15 || ((size_t)d_lens | (size_t)d_stream_len) & 7)
    return set_err(c, VC2HIP_EINVAL, "device buffers and the payload stride must be 16-byte aligned");
  if (sp->major_version < 1) return set_err(c, VC2HIP_EINVAL, "major_version must be at least 1");
  if (int rc = matrix_depth_check(c, cp)) return rc;
  StreamWriteParams p;
  memset(&p, 0, sizeof p);
  size_t hl = 0; // (a set matrix is written, the default included: set means written)
  if (vc2hip_picture_header_qm(cp, sp->major_version, sp->first_picture_number, c->qm_depth ? c->qm : nullptr, c->qm_depth, p.hdr,
                               sizeof p.hdr, &hl))
    return set_err(c, VC2HIP_EINVAL);
  ENTER(c);
  NEED(c, B_UNITS, (size_t)n * 8, p.unit_off);
  p.payload = (const uint8_t *)d_payload; p.payload_stride = (long long)payload_stride;
  p.lens = (const unsigned long long *)d_lens;
  p.stream = d_stream; p.cap = cap; p.stream_len = (unsigned long long *)d_stream_len;
  p.err = c->d_err;
  p.n = n; p.hdr_len = (int)hl; p.code = cp->mode == VC2HIP_LD ? 0xC8 : 0xE8; p.eos = sp->end_of_sequence != 0;
  p.first_picture_number = sp->first_picture_number; p.prev_parse_offset = sp->prev_parse_offset;
  vc2_launch_stream_layout(c->L, p, c->stream);
  vc2_launch_stream_copy(c->L, p, c->stream);
  return VC2HIP_OK;
}

extern "C" int vc2hip_stream_write_fragments_dev(vc2hip_ctx *c, const void *d_payload, size_t payload_stride, const uint64_t *d_lens,
                                                 int n, const vc2hip_coding_params *cp, const vc2hip_stream_params *sp,
                                                 int fragment_length, uint8_t *d_stream, size_t cap, uint64_t *d_stream_len,
                                                 uint64_t *d_unit_offsets, size_t unit_cap, uint64_t *d_unit_count) {
  if (!c || !d_payload || !d_lens || n < 1 || !cp || !sp || !d_stream || !d_stream_len) return set_err(c, VC2HIP_EINVAL);
  if (((size_t)d_payload | payload_stride | (size_t)d_stream) & 15 ||
      ((size_t)d_lens | (size_t)d_stream_len | (size_t)d_unit_offsets | (size_t)d_unit_count) & 7)
    return set_err(c, VC2HIP_EINVAL, "device buffers and the payload stride must be 16-byte aligned");
  if (sp->major_version < 3) return set_err(c, VC2HIP_EINVAL, "fragments need major_version 3 or above");
  if (fragment_length < 1 || fragment_length > 65535) return set_err(c, VC2HIP_EINVAL, "fragment_length must be 1 ... 65535");
  if ((d_unit_offsets != nullptr) != (d_unit_count != nullptr) || (d_unit_offsets != nullptr) != (unit_cap != 0))
    return set_err(c, VC2HIP_EINVAL, "d_unit_offsets, unit_cap and d_unit_count: all three or none");
  if (!stream_cp_ok(cp) || cp->x_slices > 65535 || cp->y_slices > 65535 || (long long)cp->x_slices * cp->y_slices > (1 << 24))
    return set_err(c, VC2HIP_EINVAL, "slice counts beyond a fragment's 16-bit slice offsets, or more than 2^24 slices");
  if (payload_stride >= (1ull << 32)) return set_err(c, VC2HIP_EINVAL, "payload_stride must be below 4 GiB");
  if (int rc = matrix_depth_check(c, cp)) return rc;
  FragParams p;
  memset(&p, 0, sizeof p);
  uint8_t hdr[VC2_STREAM_HDR_MAX];
  size_t hl = 0;
  if (vc2hip_picture_header_qm(cp, sp->major_version, 0, c->qm_depth ? c->qm : nullptr, c->qm_depth, hdr, sizeof hdr, &hl) || hl < 4)
    return set_err(c, VC2HIP_EINVAL);
  p.tp_len = (int)hl - 4; // the transform parameters: the header without its picture number
  memcpy(p.tp, hdr + 4, (size_t)p.tp_len);
  ENTER(c);
  const int ns = cp->y_slices * cp->x_slices;
  int rc;
  p.hq = cp->mode != VC2HIP_LD;
  if (p.hq) {
    uint32_t *d_offs;
    if ((rc = build_index(c, (const uint8_t *)d_payload, (long long)payload_stride, (const unsigned long long *)d_lens, n, ns,
                          cp->prefix, cp->scalar, &d_offs))) return rc;
    p.offs = d_offs; p.offs_stride = ns;
  } else { // the per-slice budget table the LD coder uses (vc2hip_encode_batch_dev / decode_batch_dev)
    Budgets b;
    if ((rc = budget_tables(c, cp->y_slices, cp->x_slices, cp->compressed_bytes, 1, LD_BUDGETS, b))) return rc;
    p.offs = b.offs; p.offs_stride = 0; p.ld_total = b.total;
  }
  NEED(c, B_FRAGS, (size_t)n * ns * sizeof(uint4), p.table);
  char *pic;
  NEED(c, B_FRAGPIC, (size_t)n * 32, pic);
  p.meta = (uint4 *)pic; p.pic_base = (unsigned long long *)(pic + (size_t)n * 16); p.unit_base = p.pic_base + n;
  if (!vc2_frag_cut_lds(ns)) NEED(c, B_FRAGJUMP, (size_t)n * vc2_frag_jump_bytes(ns), p.jump);
  p.payload = (const uint8_t *)d_payload; p.payload_stride = (long long)payload_stride;
  p.lens = (const unsigned long long *)d_lens;
  p.prefix = cp->prefix; p.scalar = cp->scalar;
  p.n = n; p.ns = ns; p.xs = cp->x_slices; p.fragment_length = (unsigned)fragment_length;
  p.stream = d_stream; p.cap = cap; p.stream_len = (unsigned long long *)d_stream_len;
  p.unit_offsets = (unsigned long long *)d_unit_offsets; p.unit_cap = unit_cap; p.unit_count = (unsigned long long *)d_unit_count;
  p.err = c->d_err;
  p.code = p.hq ? 0xEC : 0xCC; p.eos = sp->end_of_sequence != 0;
  p.first_picture_number = sp->first_picture_number; p.prev_parse_offset = sp->prev_parse_offset;
  vc2_launch_frag_cut(c->L, p, c->stream);
  vc2_launch_frag_layout(c->L, p, c->stream);
  vc2_launch_frag_copy(c->L, p, c->stream);
  return VC2HIP_OK;
}

extern "C" int vc2hip_stream_read_dev(vc2hip_ctx *c, const uint8_t *d_stream, size_t len, int n, const vc2hip_coding_params *cp,
                                      const vc2hip_stream_params *sp, void *d_payload, size_t payload_stride, uint64_t *d_lens,
                                      uint32_t *d_picture_numbers, uint64_t *d_consumed) {
  if (!c || !d_stream || n < 1 || !cp || !sp || !d_payload || !d_lens) return set_err(c, VC2HIP_EINVAL);
  if (((size_t)d_payload | payload_stride) & 15 || ((size_t)d_lens | (size_t)d_consumed) & 7 || (size_t)d_picture_numbers & 3)
    return set_err(c, VC2HIP_EINVAL, "device buffers and the payload stride must be 16-byte aligned");
  if (!stream_cp_ok(cp) || sp->major_version < 0 || payload_stride >= (1ull << 32)) return set_err(c, VC2HIP_EINVAL);
  if (int rc = matrix_depth_check(c, cp)) return rc;
  StreamReadParams p;
  memset(&p, 0, sizeof p);
  // The context's effective matrix, against which the walk holds every picture's: its own entries, or -- custom_quant_matrix
  // clear -- the default of its wavelet and depth, which are cp's by then (flagless_ok says whether that default is ours).
  // Beyond depth 7 there is no matrix to set or to compare: pictures without one pass, pictures with one are refused.
  if (cp->depth <= VC2_MAX_DEPTH) {
    int32_t qm[VC2_MAX_BANDS], dflt[VC2_MAX_BANDS];
    if (int rc = effective_matrix(c, cp, qm)) return rc;
    if (vc2hip_quant_matrix(cp->kernel, cp->depth, dflt)) return set_err(c, VC2HIP_EINVAL);
    p.qm_entries = 3 * cp->depth + 1;
    p.flagless_ok = 1;
    for (int b = 0; b < p.qm_entries; ++b) { p.qmatrix[b] = qm[b]; p.flagless_ok = p.flagless_ok && qm[b] == dflt[b]; }
  } else p.flagless_ok = 1;
  ENTER(c);
  p.seg_cap = cp->y_slices * cp->x_slices + 1; // a picture unit is one segment, a fragment holds at least one slice
  NEED(c, B_SEGS, (size_t)n * p.seg_cap * sizeof(StreamSeg), p.segs);
  NEED(c, B_UNITS, (size_t)n * sizeof(uint2), p.meta);
  p.stream = d_stream; p.len = len; p.n = n; p.major_version = sp->major_version;
  p.kernel = cp->kernel; p.depth = cp->depth; p.ys = cp->y_slices; p.xs = cp->x_slices; p.ld = cp->mode == VC2HIP_LD;
  stream_ab(cp, &p.a, &p.b);
  p.payload = (uint8_t *)d_payload; p.payload_stride = (long long)payload_stride;
  p.lens = (unsigned long long *)d_lens; p.picture_numbers = d_picture_numbers; p.consumed = (unsigned long long *)d_consumed;
  p.err = c->d_err;
  vc2_launch_stream_walk(c->L, p, c->stream);
  vc2_launch_stream_gather(c->L, p, c->stream);
  return VC2HIP_OK;
}

extern "C" int vc2hip_dwt_launches(const vc2hip_ctx *c, vc2hip_dwt_launch *out, int cap) {
  if (!c || cap < 0 || (cap && !out)) return VC2HIP_EINVAL;
  const int n = (int)c->dwt_rec.size();
  for (int i = 0; i < n && i < cap; ++i) out[i] = c->dwt_rec[i];
  return n;
}

// what the three decoding calls refuse in cp; g: the coded picture's geometry
static int decode_check(vc2hip_ctx *c, const vc2hip_picture_format *f, const vc2hip_coding_params *cp, const uint64_t *d_lens, bool ld, Geom &g) {
  if (!ld && (!d_lens || cp->scalar < 1 || cp->prefix < 0)) return set_err(c, VC2HIP_EINVAL);
  const int rc = picture_geom(g, f, cp, true);
  return rc ? set_err(c, rc) : VC2HIP_OK;
}

// vc2hip_decode_batch_dev, and the one picture of the host-buffer calls (ld: the call's, whatever cp->mode says)
static int decode_batch(vc2hip_ctx *c, const void *d_payload, size_t payload_stride, const uint64_t *d_lens, int n,
                        const vc2hip_picture_format *f, const vc2hip_coding_params *cp, void *d_raw_out, bool ld) {
  if (int rc = batch_args(c, n, f, cp, payload_stride, {{d_raw_out, 16}, {d_payload, 16}, {d_lens, 8, true}})) return rc;
  Geom g;
  if (int rc = decode_check(c, f, cp, d_lens, ld, g)) return rc;
  RawLayout lay;
  if (int rc = batch_layout(c, f, lay)) return rc;
  const BatchBuf bufs[] = {{d_payload, payload_stride, false}, {d_lens, 8, false}, {d_raw_out, lay.stride, true}};
  return run_batch(c, n, bufs, [&](vc2hip_ctx *l, int count, void *const *at) {
    return decode_batch_common(l, g, at[0], payload_stride, (const uint64_t *)at[1], count, f, f, cp, at[2], ld);
  });
}
extern "C" int vc2hip_decode_batch_dev(vc2hip_ctx *c, const void *d_payload, size_t payload_stride, const uint64_t *d_lens,
                                       int n, const vc2hip_picture_format *f, const vc2hip_coding_params *cp, void *d_raw_out) {
  return decode_batch(c, d_payload, payload_stride, d_lens, n, f, cp, d_raw_out, cp && cp->mode == VC2HIP_LD);
}

// vc2hip_transcode_batch_dev (include/vc2hip.h): slots in, coarser slots out, through the coefficient
// store and no further.  The decoder's slice index and slice reader leave the quantised coefficients in the store as
// slice records; k_transcode_scale dequantises the slices that end at a coarser index; the encoder's slice coder
// quantises and writes them (run_pack: every one of its forms, as encode_batch_common runs it).  No transform runs.
// The capped form finds each picture's index first (transcode_measure / transcode_pick over the payload, two rounds).
static int transcode_batch_common(vc2hip_ctx *c, const Geom &g, const void *d_in, size_t stride_in, const uint64_t *d_lens_in, int n,
                                  const vc2hip_coding_params *cp, const vc2hip_transcode_params *tp, void *d_out, size_t stride_out,
                                  uint64_t *d_lens_out, int32_t *d_qidx) {
  ENTER(c);
  int rc;
  const int ns = g.ys * g.xs;
  int32_t qm[VC2_MAX_BANDS];
  if ((rc = effective_matrix(c, cp, qm))) return rc;
  const bool s16 = use_store16(c, g, cp->kernel);
  const long long sstride = (long long)ns * g.slice_coefs;
  TranscodeParams p;
  memset(&p, 0, sizeof p);
  int32_t *d_store, *d_storew = nullptr, *d_q;
  NEED(c, B_STORE, (size_t)n * sstride * 4, d_store);
  if (s16) NEED(c, B_STOREW, (size_t)n * sstride * 4, d_storew);
  NEED(c, B_QIDX, (size_t)n * ns * 4, d_q);
  NEED(c, B_TCLEN, (size_t)n * ns * 4, p.qpack);
  NEED(c, B_TCQ, (size_t)n * 4, p.qpic);
  if (tp->cap_bytes > 0) NEED(c, B_CAPTAB, (size_t)n * VC2_CAP_ROW * 8, p.table);
  const Store st = {d_store, d_storew, s16, sstride};
  uint32_t *d_offs;
  if ((rc = build_index(c, (const uint8_t *)d_in, (long long)stride_in, (const unsigned long long *)d_lens_in, n, ns, cp->prefix,
                        cp->scalar, &d_offs, cbr_claim_tables(c, g, cp)))) return rc;
  UnpackParams u;
  fill_unpack(u, g, (const uint8_t *)d_in, (long long)stride_in, (const unsigned long long *)d_lens_in, d_offs, st, d_q, cp->prefix,
              cp->scalar, c->d_err);
  u.xs = g.xs; u.stats = c->d_stat;
  vc2_launch_unpack(c->L, u, n, c->stream);

  p.in = u.payload; p.in_stride = u.payload_stride; p.in_lens = u.lens; p.in_offs = d_offs;
  p.store = d_store; p.store_wide = d_storew; p.store16 = s16; p.store_stride = sstride;
  p.slice_coefs = g.slice_coefs; p.qs = d_q; p.qidx_out = d_qidx;
  p.n_slices = ns;
  fill_comp_arrays(g, p.comp_n, p.comp_off, p.comp_n0);
  p.prefix = cp->prefix; p.scalar = cp->scalar;
  p.target = tp->q_index; p.capped = tp->cap_bytes > 0; p.cap = (unsigned long long)tp->cap_bytes;
  p.qm_min = qm[0];
  for (int b = 0; b < 3 * g.depth + 1; ++b) { p.qmatrix[b] = qm[b]; p.qm_min = std::min(p.qm_min, (int)qm[b]); }
  p.err = c->d_err;
  if (p.capped) {
    HIPCHK(c, hipMemsetAsync(p.table, 0, (size_t)n * VC2_CAP_ROW * 8, c->stream));
    for (p.round = 0; p.round < 2; ++p.round) {
      vc2_launch_transcode_measure(c->L, p, n, c->stream);
      vc2_launch_transcode_pick(c->L, p, n, c->stream);
    }
  }
  vc2_launch_transcode_scale(c->L, p, n, c->stream);
  PackJob job; // (no budgets: the output is a VBR payload whatever coded the input)
  job.store = st; job.qidx = p.qpack; job.qm = qm;
  job.prefix = cp->prefix; job.scalar = cp->scalar;
  job.payload = (uint8_t *)d_out; job.stride = (long long)stride_out; job.lens = (unsigned long long *)d_lens_out;
  return run_pack(c, g, n, job);
}

extern "C" int vc2hip_transcode_batch_dev(vc2hip_ctx *c, const void *d_payload_in, size_t payload_stride_in, const uint64_t *d_lens_in,
                                          int n, const vc2hip_picture_format *f, const vc2hip_coding_params *cp,
                                          const vc2hip_transcode_params *tp, void *d_payload_out, size_t payload_stride_out,
                                          uint64_t *d_lens_out, int32_t *d_qidx) {
  if (int rc = batch_args(c, n, f, cp, payload_stride_in,
                          {{d_payload_in, 16}, {d_lens_in, 8}, {d_payload_out, 16}, {d_lens_out, 8}, {d_qidx, 4, true}})) return rc;
  if (!tp) return set_err(c, VC2HIP_EINVAL);
  if (payload_stride_out & 15) return set_err(c, VC2HIP_EINVAL, "device buffers and the payload stride must be 16-byte aligned");
  if (cp->mode != VC2HIP_HQ_CONSTQ && cp->mode != VC2HIP_HQ_CBR && cp->mode != VC2HIP_HQ_CAPPED && cp->mode != VC2HIP_HQ_CAPPED_FILL)
    return set_err(c, VC2HIP_EINVAL, "transcode_batch_dev: HQ pictures only");
  if (tp->q_index < 0 || tp->q_index > VC2_CAP_Q_TOP || tp->cap_bytes < 0)
    return set_err(c, VC2HIP_EINVAL, "transcode_batch_dev: q_index 0 .. 115, cap_bytes >= 0");
  Geom g;
  if (int rc = decode_check(c, f, cp, d_lens_in, false, g)) return rc;
  const uint8_t *in8 = (const uint8_t *)d_payload_in, *out8 = (const uint8_t *)d_payload_out;
  if (out8 < in8 + (size_t)n * payload_stride_in && in8 < out8 + (size_t)n * payload_stride_out)
    return set_err(c, VC2HIP_EINVAL, "transcode_batch_dev: the output slots overlap the input slots");
  // (the output is a VBR payload whatever coded the input: under an HQ_CBR cp the bound is still what three length bytes a
  // slice can describe, not the budget -- slot bytes no encoder wrote may ask for all of it, and the slice coder clamps nothing)
  if (payload_stride_out < vc2hip_max_payload_bytes(f, cp) || payload_stride_out < (size_t)g.ys * g.xs * max_slice_bytes(cp->prefix, cp->scalar))
    return set_err(c, VC2HIP_ECAP);
  const BatchBuf bufs[] = {{d_payload_in, payload_stride_in, false}, {d_lens_in, 8, false}, {d_payload_out, payload_stride_out, true},
                           {d_lens_out, 8, true}, {d_qidx, (size_t)g.ys * g.xs * 4, true}};
  return run_batch(c, n, bufs, [&](vc2hip_ctx *l, int count, void *const *at) {
    return transcode_batch_common(l, g, at[0], payload_stride_in, (const uint64_t *)at[1], count, cp, tp, at[2], payload_stride_out,
                                  (uint64_t *)at[3], (int32_t *)at[4]);
  });
}

// vc2hip_transcode_cbr_batch_dev (include/vc2hip.h): slots in, HQ_CBR slots out, through the coefficient
// store and no further.  The slice index and the slice reader at cp_in's prefix and scalar; k_transcode_fit keeps the slices
// that fit cp_out's budgets as they are and dequantises the others; the HQ_CBR search over those alone; the slice coder in its
// CBR form at cp_out's prefix and scalar; k_transcode_settle for d_qidx and the order of the refusals.  No transform runs.
// Two budget tables may be alive at once: an HQ_CBR input's claim (slot 0) and the output's budgets (slot 1).
static int transcode_cbr_batch_common(vc2hip_ctx *c, const Geom &g, const void *d_in, size_t stride_in, const uint64_t *d_lens_in, int n,
                                      const vc2hip_coding_params *cp_in, const vc2hip_coding_params *cp_out, void *d_out,
                                      size_t stride_out, uint64_t *d_lens_out, int32_t *d_qidx) {
  ENTER(c);
  int rc;
  const int ns = g.ys * g.xs;
  int32_t qm[VC2_MAX_BANDS];
  if ((rc = effective_matrix(c, cp_in, qm))) return rc;
  Budgets out_b;
  if ((rc = budget_tables(c, g.ys, g.xs, cp_out->compressed_bytes, cp_out->scalar, cp_out->prefix, out_b, nullptr, 1))) return rc;
  if (stride_out < out_b.total) return set_err(c, VC2HIP_ECAP); // (what vc2hip_encode_batch_dev asks under cp_out; before any launch)
  const bool s16 = use_store16(c, g, cp_in->kernel);
  const long long sstride = record_stride(g);
  TranscodeParams p;
  memset(&p, 0, sizeof p);
  int32_t *d_store, *d_storew = nullptr, *d_q;
  NEED(c, B_STORE, (size_t)n * sstride * 4, d_store);
  if (s16) NEED(c, B_STOREW, (size_t)n * sstride * 4, d_storew);
  NEED(c, B_QIDX, (size_t)n * ns * 4, d_q);
  NEED(c, B_TCLEN, (size_t)n * ns * 4, p.qpack);
  const Store st = {d_store, d_storew, s16, sstride};
  uint32_t *d_offs;
  if ((rc = build_index(c, (const uint8_t *)d_in, (long long)stride_in, (const unsigned long long *)d_lens_in, n, ns, cp_in->prefix,
                        cp_in->scalar, &d_offs, cbr_claim_tables(c, g, cp_in)))) return rc;
  UnpackParams u;
  fill_unpack(u, g, (const uint8_t *)d_in, (long long)stride_in, (const unsigned long long *)d_lens_in, d_offs, st, d_q, cp_in->prefix,
              cp_in->scalar, c->d_err);
  u.xs = g.xs; u.stats = c->d_stat;
  vc2_launch_unpack(c->L, u, n, c->stream);

  p.store = d_store; p.store_wide = d_storew; p.store16 = s16; p.store_stride = sstride;
  p.slice_coefs = g.slice_coefs; p.qs = d_q; p.qidx_out = d_qidx;
  p.n_slices = ns;
  fill_comp_arrays(g, p.comp_n, p.comp_off, p.comp_n0);
  p.prefix = cp_out->prefix; p.scalar = cp_out->scalar;
  p.out_budgets = out_b.bytes; p.out_scalar = cp_out->scalar;
  p.qm_min = qm[0];
  for (int b = 0; b < 3 * g.depth + 1; ++b) { p.qmatrix[b] = qm[b]; p.qm_min = std::min(p.qm_min, (int)qm[b]); }
  p.err = c->d_err;
  vc2_launch_transcode_fit(c->L, p, n, c->stream);
  CbrParams s;
  fill_cbr(s, g, st, p.qpack, out_b.bytes, cp_out->scalar, qm, c->cbr_general, c->d_err);
  vc2_launch_cbr_marked(c->L, s, n, c->stream);
  PackJob job;
  job.store = st; job.qidx = p.qpack; job.qm = qm;
  job.prefix = cp_out->prefix; job.scalar = cp_out->scalar; job.budgets = out_b;
  job.payload = (uint8_t *)d_out; job.stride = (long long)stride_out; job.lens = (unsigned long long *)d_lens_out;
  if ((rc = run_pack(c, g, n, job))) return rc;
  vc2_launch_transcode_settle(c->L, p, n, c->stream);
  return VC2HIP_OK;
}

extern "C" int vc2hip_transcode_cbr_batch_dev(vc2hip_ctx *c, const void *d_payload_in, size_t payload_stride_in, const uint64_t *d_lens_in,
                                              int n, const vc2hip_picture_format *f, const vc2hip_coding_params *cp_in,
                                              const vc2hip_coding_params *cp_out, void *d_payload_out, size_t payload_stride_out,
                                              uint64_t *d_lens_out, int32_t *d_qidx) {
  if (int rc = batch_args(c, n, f, cp_in, payload_stride_in,
                          {{d_payload_in, 16}, {d_lens_in, 8}, {d_payload_out, 16}, {d_lens_out, 8}, {d_qidx, 4, true}})) return rc;
  if (!cp_out) return set_err(c, VC2HIP_EINVAL);
  if (payload_stride_out & 15) return set_err(c, VC2HIP_EINVAL, "device buffers and the payload stride must be 16-byte aligned");
  if (cp_in->mode != VC2HIP_HQ_CONSTQ && cp_in->mode != VC2HIP_HQ_CBR && cp_in->mode != VC2HIP_HQ_CAPPED && cp_in->mode != VC2HIP_HQ_CAPPED_FILL)
    return set_err(c, VC2HIP_EINVAL, "transcode_cbr_batch_dev: HQ pictures only");
  if (cp_out->mode != VC2HIP_HQ_CBR) return set_err(c, VC2HIP_EINVAL, "transcode_cbr_batch_dev: cp_out must be HQ_CBR");
  if (cp_out->kernel != cp_in->kernel || cp_out->depth != cp_in->depth || cp_out->y_slices != cp_in->y_slices || cp_out->x_slices != cp_in->x_slices)
    return set_err(c, VC2HIP_EINVAL, "transcode_cbr_batch_dev: cp_out must have cp_in's kernel, depth and slice counts");
  if (cp_out->compressed_bytes < 1 || cp_out->scalar < 1 || cp_out->prefix < 0)
    return set_err(c, VC2HIP_EINVAL, "transcode_cbr_batch_dev: cp_out needs compressed_bytes >= 1, scalar >= 1, prefix >= 0");
  Geom g;
  if (int rc = decode_check(c, f, cp_in, d_lens_in, false, g)) return rc;
  const uint8_t *in8 = (const uint8_t *)d_payload_in, *out8 = (const uint8_t *)d_payload_out;
  if (out8 < in8 + (size_t)n * payload_stride_in && in8 < out8 + (size_t)n * payload_stride_out)
    return set_err(c, VC2HIP_EINVAL, "transcode_cbr_batch_dev: the output slots overlap the input slots");
  const BatchBuf bufs[] = {{d_payload_in, payload_stride_in, false}, {d_lens_in, 8, false}, {d_payload_out, payload_stride_out, true},
                           {d_lens_out, 8, true}, {d_qidx, (size_t)g.ys * g.xs * 4, true}};
  return run_batch(c, n, bufs, [&](vc2hip_ctx *l, int count, void *const *at) {
    return transcode_cbr_batch_common(l, g, at[0], payload_stride_in, (const uint64_t *)at[1], count, cp_in, cp_out, at[2],
                                      payload_stride_out, (uint64_t *)at[3], (int32_t *)at[4]);
  });
}

// Pictures at 1 / 2^drop_levels size (include/vc2hip.h): f and cp are the CODED picture's; the split over lanes is by
// pictures, as the full decoder's, with the smaller pictures' size in the output
extern "C" int vc2hip_decode_reduced_batch_dev(vc2hip_ctx *c, const void *d_payload, size_t payload_stride, const uint64_t *d_lens,
                                               int n, const vc2hip_picture_format *f, const vc2hip_coding_params *cp, int drop_levels,
                                               void *d_raw_out) {
  if (int rc = batch_args(c, n, f, cp, payload_stride, {{d_raw_out, 16}, {d_payload, 16}, {d_lens, 8, true}})) return rc;
  if (drop_levels < 1 || drop_levels >= cp->depth)
    return set_err(c, VC2HIP_EINVAL, "decode_reduced_batch_dev: drop_levels must be 1 ... depth - 1 (one transform level at least is kept)");
  if (cp->kernel == VC2HIP_DAUB97)
    return set_err(c, VC2HIP_EINVAL, "decode_reduced_batch_dev: Daub97's low-pass gain per level (about 3.03) is no power of two, so a shift cannot normalise its reduced pictures");
  const bool ld = cp->mode == VC2HIP_LD;
  Geom g;
  if (int rc = decode_check(c, f, cp, d_lens, ld, g)) return rc;
  int h[3], w[3], ph[3], pw[3];
  for (int k = 0; k < 3; ++k) {
    const CompGeom &cg = g.c[k];
    if ((cg.h | cg.w) & ((1 << drop_levels) - 1))
      return set_err(c, VC2HIP_EINVAL, "decode_reduced_batch_dev: every component's width and height must be a multiple of 2^drop_levels");
    h[k] = cg.h >> drop_levels; w[k] = cg.w >> drop_levels; ph[k] = cg.ph >> drop_levels; pw[k] = cg.pw >> drop_levels;
  }
  // the picture the kept levels make (decode_batch_common), and the format of the pictures in d_raw_out
  if (int rc = make_geom(g, ph, pw, h, w, cp->depth - drop_levels, cp->y_slices, cp->x_slices)) return set_err(c, rc);
  vc2hip_picture_format fr = *f;
  fr.width = f->width >> drop_levels; fr.height = f->height >> drop_levels;
  RawLayout lay;
  if (int rc = batch_layout(c, &fr, lay)) return rc;
  const BatchBuf bufs[] = {{d_payload, payload_stride, false}, {d_lens, 8, false}, {d_raw_out, lay.stride, true}};
  return run_batch(c, n, bufs, [&](vc2hip_ctx *l, int count, void *const *at) {
    return decode_batch_common(l, g, at[0], payload_stride, (const uint64_t *)at[1], count, &fr, f, cp, at[2], ld, 1, 1, drop_levels);
  });
}

// Field pictures of interleaved frames (include/vc2hip.h): a field has the frame's format at half its height, so the
// frame's luma and chroma heights must be even (as the host tools require of an interlaced frame: host/Frame.cpp).
// An item of the two calls is a frame: two payload slots and two lengths.
static int field_format(vc2hip_ctx *c, const vc2hip_picture_format *frame, vc2hip_picture_format *field) {
  int ch, cw;
  chroma_dims(frame->height, frame->width, frame->chroma_format, &ch, &cw);
  if (frame->height < 2 || frame->height % 2 || ch % 2)
    return set_err(c, VC2HIP_EINVAL, "field pictures need a frame whose luma and chroma heights are even (4:2:0: a multiple of 4)");
  *field = *frame;
  field->height = frame->height / 2;
  return VC2HIP_OK;
}

extern "C" int vc2hip_encode_fields_batch_dev(vc2hip_ctx *c, const void *d_frames, int n_frames, const vc2hip_picture_format *frame_fmt,
                                              int top_field_first, const vc2hip_coding_params *cp, void *d_payload,
                                              size_t payload_stride, uint64_t *d_lens) {
  if (int rc = batch_args(c, n_frames, frame_fmt, cp, payload_stride, {{d_frames, 16}, {d_payload, 16}, {d_lens, 8}},
                          "encode_fields_batch_dev: a null argument or fewer than one frame")) return rc;
  vc2hip_picture_format ff;
  if (int rc = field_format(c, frame_fmt, &ff)) return rc;
  RawLayout lay; // (the FRAME's)
  if (int rc = batch_layout(c, frame_fmt, lay)) return rc;
  Geom g;
  if (int rc = encode_check(c, &ff, cp, g)) return rc;
  const IndexOffsets io = {c->idx_offs, c->idx_offs_stride}; // by coded picture: a frame is two maps, in slot order
  if (int rc = offsets_check(c, io, cp, g)) return rc;
  const BatchBuf bufs[] = {{d_frames, lay.stride, false}, {d_payload, 2 * payload_stride, true}, {d_lens, 16, true}, {io.p, 2 * io.stride, false}};
  return run_batch(c, n_frames, bufs, [&](vc2hip_ctx *l, int count, void *const *at) {
    return encode_batch_common(l, g, at[0], 2, top_field_first != 0, 2 * count, frame_fmt, &ff, cp, at[1], payload_stride, (uint64_t *)at[2],
                               {(const int8_t *)at[3], io.stride});
  });
}

extern "C" int vc2hip_decode_fields_batch_dev(vc2hip_ctx *c, const void *d_payload, size_t payload_stride, const uint64_t *d_lens,
                                              int n_frames, const vc2hip_picture_format *frame_fmt, int top_field_first,
                                              const vc2hip_coding_params *cp, void *d_frames_out) {
  if (int rc = batch_args(c, n_frames, frame_fmt, cp, payload_stride, {{d_frames_out, 16}, {d_payload, 16}, {d_lens, 8, true}},
                          "decode_fields_batch_dev: a null argument or fewer than one frame")) return rc;
  vc2hip_picture_format ff;
  if (int rc = field_format(c, frame_fmt, &ff)) return rc;
  const bool ld = cp->mode == VC2HIP_LD;
  Geom g;
  if (int rc = decode_check(c, &ff, cp, d_lens, ld, g)) return rc;
  RawLayout lay; // (the FRAME's)
  if (int rc = batch_layout(c, frame_fmt, lay)) return rc;
  const BatchBuf bufs[] = {{d_payload, 2 * payload_stride, false}, {d_lens, 16, false}, {d_frames_out, lay.stride, true}};
  return run_batch(c, n_frames, bufs, [&](vc2hip_ctx *l, int count, void *const *at) {
    return decode_batch_common(l, g, at[0], payload_stride, (const uint64_t *)at[1], 2 * count, frame_fmt, &ff, cp, at[2], ld, 2,
                               top_field_first != 0);
  });
}

extern "C" int vc2hip_encode_picture_hq(vc2hip_ctx *c, const void *raw, const vc2hip_picture_format *f,
                                        const vc2hip_coding_params *cp, uint8_t *payload, size_t cap, size_t *len,
                                        int32_t *qidx_out) {
  if (!c || !raw || !f || !cp || !payload || !len) return set_err(c, VC2HIP_EINVAL);
  if (int rc = matrix_depth_check(c, cp)) return rc;
  ENTER(c);
  const size_t rb = vc2hip_raw_picture_bytes(f), pcap = (vc2hip_max_payload_bytes(f, cp) + 15) & ~(size_t)15;
  uint8_t *d_raw, *d_pay; unsigned long long *d_len;
  NEED(c, B_RAW, rb + 64, d_raw);
  NEED(c, B_PAYLOAD, pcap + 64, d_pay);
  NEED(c, B_LENS, 64, d_len);
  HIPCHK(c, hipMemcpyAsync(d_raw, raw, rb, hipMemcpyHostToDevice, c->stream));
  const LayoutBypass file_format(c); // (the host-buffer calls keep the file format)
  int rc = encode_batch_dev(c, d_raw, 1, f, cp, d_pay, pcap, (uint64_t *)d_len, {nullptr, 0}); // (no index offsets: a device-batch feature)
  if (rc) return rc;
  unsigned long long l = 0;
  HIPCHK(c, hipMemcpyAsync(&l, d_len, 8, hipMemcpyDeviceToHost, c->stream));
  if (qidx_out)
    HIPCHK(c, hipMemcpyAsync(qidx_out, c->buf[B_QIDX].p, (size_t)cp->y_slices * cp->x_slices * 4, hipMemcpyDeviceToHost, c->stream));
  if ((rc = vc2hip_sync(c))) return rc;
  if (l > cap) return set_err(c, VC2HIP_ECAP);
  HIPCHK(c, hipMemcpy(payload, d_pay, l, hipMemcpyDeviceToHost));
  *len = (size_t)l;
  return VC2HIP_OK;
}

extern "C" int vc2hip_encode_picture_ld(vc2hip_ctx *c, const void *raw, const vc2hip_picture_format *f,
                                        const vc2hip_coding_params *cp, uint8_t *payload, size_t cap, size_t *len,
                                        int32_t *qidx_out) {
  if (!cp || cp->mode != VC2HIP_LD) return set_err(c, VC2HIP_EINVAL);
  return vc2hip_encode_picture_hq(c, raw, f, cp, payload, cap, len, qidx_out);
}

static int decode_picture_host(vc2hip_ctx *c, const uint8_t *payload, size_t len, const vc2hip_picture_format *f,
                               const vc2hip_coding_params *cp, void *raw_out, bool ld) {
  if (!c || !payload || !f || !cp || !raw_out) return set_err(c, VC2HIP_EINVAL);
  if (int rc = matrix_depth_check(c, cp)) return rc;
  ENTER(c);
  const size_t rb = vc2hip_raw_picture_bytes(f);
  const size_t stride = (len + 63) & ~(size_t)63;
  uint8_t *d_raw, *d_pay; unsigned long long *d_len;
  NEED(c, B_RAW, rb + 64, d_raw);
  NEED(c, B_PAYLOAD, stride + 64, d_pay);
  NEED(c, B_LENS, 64, d_len);
  unsigned long long l64 = len;
  HIPCHK(c, hipMemcpyAsync(d_pay, payload, len, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_len, &l64, 8, hipMemcpyHostToDevice, c->stream));
  const LayoutBypass file_format(c); // (the host-buffer calls keep the file format)
  int rc = decode_batch(c, d_pay, stride, (const uint64_t *)d_len, 1, f, cp, d_raw, ld);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(raw_out, d_raw, rb, hipMemcpyDeviceToHost, c->stream));
  return vc2hip_sync(c);
}
extern "C" int vc2hip_decode_picture_hq(vc2hip_ctx *c, const uint8_t *payload, size_t len, const vc2hip_picture_format *f,
                                        const vc2hip_coding_params *cp, void *raw_out) {
  return decode_picture_host(c, payload, len, f, cp, raw_out, false);
}
extern "C" int vc2hip_decode_picture_ld(vc2hip_ctx *c, const uint8_t *payload, size_t len, const vc2hip_picture_format *f,
                                        const vc2hip_coding_params *cp, void *raw_out) {
  return decode_picture_host(c, payload, len, f, cp, raw_out, true);
}

// ------------------------------------------------------------------------------------------
// pipelined picture calls (include/vc2hip.h): two pictures in flight per context
// ------------------------------------------------------------------------------------------
extern "C" void *vc2hip_host_alloc(size_t bytes) {
  void *p = nullptr;
  return hipHostMalloc(&p, bytes ? bytes : 1) == hipSuccess ? p : nullptr;
}
extern "C" void vc2hip_host_free(void *p) { if (p) (void)hipHostFree(p); }

static int flight_begin(vc2hip_ctx *c, bool encode, vc2hip_ctx::Flight **out, int *ticket) {
  if (!ticket) return set_err(c, VC2HIP_EINVAL);
  HIPCHK(c, hipSetDevice(c->device));
  vc2hip_ctx::Flight &f = c->flight[c->flight_next];
  if (f.open) return set_err(c, VC2HIP_EINVAL, "too many pictures in flight (VC2HIP_MAX_INFLIGHT): end the oldest ticket first");
  if (!f.lane) {
    const int rc = vc2hip_create(c->device, &f.lane);
    if (rc) return set_err(c, rc, "cannot create a stream for a picture in flight");
  }
  if (!f.h_len) HIPCHK(c, hipHostMalloc((void **)&f.h_len, 64)); // (its own test: a failure here must not leave a lane without it)
  f.open = true;
  f.encode = encode;
  *ticket = c->flight_next;
  c->flight_next = (c->flight_next + 1) % VC2HIP_MAX_INFLIGHT;
  *out = &f;
  return VC2HIP_OK;
}

extern "C" int vc2hip_encode_picture_begin(vc2hip_ctx *c, const void *raw, const vc2hip_picture_format *f,
                                           const vc2hip_coding_params *cp, uint8_t *payload, size_t cap, int32_t *qidx_out,
                                           int *ticket) {
  if (!c || !raw || !f || !cp || !payload) return set_err(c, VC2HIP_EINVAL);
  int rc = matrix_depth_check(c, cp);
  if (rc) return rc;
  vc2hip_ctx::Flight *fl;
  if ((rc = flight_begin(c, true, &fl, ticket))) return rc;
  vc2hip_ctx *l = fl->lane;
  inherit_matrix(l, c);
  fl->payload = payload; fl->cap = cap;
  const size_t rb = vc2hip_raw_picture_bytes(f), pcap = (vc2hip_max_payload_bytes(f, cp) + 15) & ~(size_t)15;
  uint8_t *d_raw, *d_pay; unsigned long long *d_len;
  auto fail = [&](int code) { fl->open = false; return set_err(c, code, l->err.c_str()); };
  if ((rc = need(l, B_RAW, rb + 64, (void **)&d_raw)) || (rc = need(l, B_PAYLOAD, pcap + 64, (void **)&d_pay)) ||
      (rc = need(l, B_LENS, 64, (void **)&d_len))) return fail(rc);
  if (hipMemcpyAsync(d_raw, raw, rb, hipMemcpyHostToDevice, l->stream) != hipSuccess) return fail(VC2HIP_EHIP);
  if ((rc = encode_batch_dev(l, d_raw, 1, f, cp, d_pay, pcap, (uint64_t *)d_len, {nullptr, 0}))) return fail(rc);
  if (hipMemcpyAsync(fl->h_len, d_len, 8, hipMemcpyDeviceToHost, l->stream) != hipSuccess) return fail(VC2HIP_EHIP);
  if (qidx_out && // (from vc2hip_host_alloc like every buffer of a _begin call: a pageable destination makes the call block)
      hipMemcpyAsync(qidx_out, l->buf[B_QIDX].p, (size_t)cp->y_slices * cp->x_slices * 4, hipMemcpyDeviceToHost, l->stream) != hipSuccess)
    return fail(VC2HIP_EHIP);
  return VC2HIP_OK;
}

extern "C" int vc2hip_encode_picture_end(vc2hip_ctx *c, int ticket, size_t *len) {
  if (!c || ticket < 0 || ticket >= VC2HIP_MAX_INFLIGHT || !len || !c->flight[ticket].open || !c->flight[ticket].encode)
    return set_err(c, VC2HIP_EINVAL);
  vc2hip_ctx::Flight &fl = c->flight[ticket];
  vc2hip_ctx *l = fl.lane;
  fl.open = false;
  int rc = vc2hip_sync(l); // the picture's stream: lengths are on the host, error flags read
  if (rc) return set_err(c, rc, l->err.c_str());
  const unsigned long long n = *fl.h_len;
  if (n > fl.cap) return set_err(c, VC2HIP_ECAP);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(fl.payload, l->buf[B_PAYLOAD].p, n, hipMemcpyDeviceToHost, l->stream)); // exactly the coded bytes
  HIPCHK(c, hipStreamSynchronize(l->stream));
  *len = (size_t)n;
  return VC2HIP_OK;
}

extern "C" int vc2hip_decode_picture_begin(vc2hip_ctx *c, const uint8_t *payload, size_t len, const vc2hip_picture_format *f,
                                           const vc2hip_coding_params *cp, void *raw_out, int *ticket) {
  if (!c || !payload || !f || !cp || !raw_out) return set_err(c, VC2HIP_EINVAL);
  int rc = matrix_depth_check(c, cp);
  if (rc) return rc;
  vc2hip_ctx::Flight *fl;
  if ((rc = flight_begin(c, false, &fl, ticket))) return rc;
  vc2hip_ctx *l = fl->lane;
  inherit_matrix(l, c);
  const size_t rb = vc2hip_raw_picture_bytes(f), stride = (len + 63) & ~(size_t)63;
  uint8_t *d_raw, *d_pay; unsigned long long *d_len;
  auto fail = [&](int code) { fl->open = false; return set_err(c, code, l->err.c_str()); };
  if ((rc = need(l, B_RAW, rb + 64, (void **)&d_raw)) || (rc = need(l, B_PAYLOAD, stride + 64, (void **)&d_pay)) ||
      (rc = need(l, B_LENS, 64, (void **)&d_len))) return fail(rc);
  *fl->h_len = len;
  if (hipMemcpyAsync(d_pay, payload, len, hipMemcpyHostToDevice, l->stream) != hipSuccess ||
      hipMemcpyAsync(d_len, fl->h_len, 8, hipMemcpyHostToDevice, l->stream) != hipSuccess) return fail(VC2HIP_EHIP);
  if ((rc = decode_batch(l, d_pay, stride, (const uint64_t *)d_len, 1, f, cp, d_raw, cp->mode == VC2HIP_LD))) return fail(rc);
  if (hipMemcpyAsync(raw_out, d_raw, rb, hipMemcpyDeviceToHost, l->stream) != hipSuccess) return fail(VC2HIP_EHIP);
  return VC2HIP_OK;
}

extern "C" int vc2hip_decode_picture_end(vc2hip_ctx *c, int ticket) {
  if (!c || ticket < 0 || ticket >= VC2HIP_MAX_INFLIGHT || !c->flight[ticket].open || c->flight[ticket].encode)
    return set_err(c, VC2HIP_EINVAL);
  vc2hip_ctx::Flight &fl = c->flight[ticket];
  fl.open = false;
  const int rc = vc2hip_sync(fl.lane);
  return rc ? set_err(c, rc, fl.lane->err.c_str()) : VC2HIP_OK;
}
