// Internal declarations shared by the libvc2hip translation units (not installed).
//
// Device data layout (DESIGN.md "Data layout in HBM"):
//   * sample planes        : raw planar words exactly as in the file (big-endian, MSB justified)
//   * LL planes            : one compact row-major int32 plane per wavelet level and component
//   * coefficient store    : [picture][slice][component][band][row][col] int32 -- every slice's
//                            coefficients already in the order the slice coder emits them, so the
//                            pack / unpack kernels stream 4 KiB-contiguous records and the DWT
//                            kernels write / gather whole band blocks of a slice contiguously.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/vc2hip.h"

#define VC2_MAX_DEPTH 7
#define VC2_MAX_BANDS (3 * VC2_MAX_DEPTH + 1)

// device-side error flags (OR-ed into ctx->d_err by kernels)
enum : unsigned {
  VC2_DEVERR_QINDEX = 1u << 0,     // adjusted quantiser index > 119
  VC2_DEVERR_SCALAR = 1u << 1,     // slice component needs > 255*scalar bytes
  VC2_DEVERR_CBR_TOOBIG = 1u << 2, // CBR: V component does not fit the slice
  VC2_DEVERR_CBR_LEN = 1u << 3,    // CBR: V length byte > 255
  VC2_DEVERR_CODE32 = 1u << 4,     // |coef| > 65534
  VC2_DEVERR_STREAM = 1u << 5,     // slice data runs past the payload
  VC2_DEVERR_LD_TOOBIG = 1u << 6,
  VC2_DEVERR_HANDOFF = 1u << 7,    // LD index search: a row waited in vain for the row above (single-launch form)
  VC2_DEVERR_CAP = 1u << 8,        // stream calls: a unit past the stream's cap, a payload past its slot
  VC2_DEVERR_SYNTAX = 1u << 9,     // stream read: the walk stopped (reason and byte offset in the error block, VC2_ERRBLK_*)
};
// the error block (ctx->d_err, 256 bytes before the LD tables): word 0 the flags above, then
#define VC2_ERRBLK_SYNTAX_AT 8      // uint64: byte offset of the stream syntax error
#define VC2_ERRBLK_SYNTAX_WHY 16    // uint32: its reason (VC2_SYN_*)
#define VC2_ERRBLK_COPY 32          // bytes vc2hip_sync copies back
enum {
  VC2_SYN_PREFIX = 1, VC2_SYN_CODE, VC2_SYN_PAST_END, VC2_SYN_NEXT_ZERO, VC2_SYN_FEWER, VC2_SYN_PARAMS, VC2_SYN_QUANT_MATRIX,
  VC2_SYN_ASYMMETRIC, VC2_SYN_NO_VERSION, VC2_SYN_FRAGMENT,
  VC2_SYN_SLICE_TOO_LONG, // fragment writer: a slice of more than 65535 bytes (VC2_ERRBLK_SYNTAX_AT holds the picture's index)
  VC2_SYN_QM_ENTRY,       // a quantisation matrix entry above 255 (VC2_SYN_QUANT_MATRIX: the picture's matrix is not the context's)
  VC2_SYN_COUNT
};

struct CompGeom {
  int h, w;     // picture plane (unpadded)
  int ph, pw;   // padded plane
  int sh, sw;   // slice size in samples (ph / ys, pw / xs)
  int coef_off; // first coefficient of this component inside a slice record
  int n0;       // coefficients of one slice in the LL band: (sh >> depth) * (sw >> depth)
};

struct Geom {
  CompGeom c[3];
  int depth, ys, xs;
  int slice_coefs; // coefficients per slice record (all three components)
};

// offset of band `band` (0 = LL, then HL,LH,HH per level, coarsest first) inside a component
// record whose LL block has n0 coefficients: level L bands hold n0 * 4^(L-1) each.
__host__ __device__ inline int band_offset(int n0, int band) {
  if (band == 0) return 0;
  const int L = (band - 1) / 3 + 1, kind = (band - 1) % 3;
  // n0 * (1 + 3 * (4^(L-1) - 1) / 3) = n0 * 4^(L-1)
  return n0 * ((1 << (2 * (L - 1))) * (1 + kind));
}
// band index of coefficient j (coding order) of a component record
__host__ __device__ inline int band_of_index(int j, int n0) {
  const int m = j / n0;
  if (m == 0) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
  const int lg = 31 - __clz(m);
#else
  const int lg = 31 - __builtin_clz((unsigned)m);
#endif
  const int L = lg / 2 + 1;
  return 3 * (L - 1) + (m >> (2 * (L - 1)));
}

struct QuantTables {
  int32_t qf[120];
  int32_t off[120];
  // exact unsigned division by qf (Granlund-Montgomery): n / qf = (t + ((n - t) >> 1)) >> (l - 1),
  // t = mulhi(magic, n); valid for every 32-bit n when qf > 0 (indices 0..115)
  uint32_t magic[120];
  int32_t shift[120];
  float inv4[120]; // the smallest float >= 4 / qf (k_cbr_search_reg)
};

// ------------------------------------------------------------------------------------------
// kernel parameter blocks
// ------------------------------------------------------------------------------------------
struct LevelParams {
  // input of a forward level / output of an inverse level
  void *plane[3];             // FIRST/FINAL: raw sample words, else LL_l plane (ST elements)
  long long plane_stride[3];  // per picture, in bytes (raw) or elements (int32); field pictures (field_shift): per frame
  int raw_pitch[3];           // FIRST/FINAL: bytes from one raw row to the next (pic_w * word_bytes; field pictures: two frame rows)
  int field_step[3];          // FIRST/FINAL, field pictures: bytes from the first field's row 0 to the second field's (+-one frame row)
  int field_shift;            // FIRST/FINAL: 1 = picture pic is field pic & 1 of frame pic >> 1 (plane[c]: the first field), 0 = progressive
  void *ll[3];                // LL_{l+1} plane, ST elements (forward: output unless LAST; inverse: input)
  long long ll_stride[3];     // per picture, elements
  void *store;                // coefficient store (int32_t or int16_t elements: the kernels' ST parameter)
  long long store_stride;     // per picture, elements
  int32_t *store_wide;        // int16 store: values outside 16 bits, same element index (vc2hip_store.h)
  int32_t *plane_wide[3];     // the same for the level planes (not FIRST / FINAL) ...
  int32_t *ll_wide[3];        // ... and the LL_{l+1} planes
  const int32_t *qidx;        // inverse: per-slice quantiser indices, n_pictures * ys * xs
  int in_h[3], in_w[3];       // plane size at this level (padded >> level)
  int pic_h[3], pic_w[3];     // FIRST/FINAL: unpadded picture size
  int fh[3], fw[3];           // slice footprint at this level, samples
  int tsy[3], tsx[3];         // slices per tile
  int tiles_y[3], tiles_x[3];
  int coef_off[3];
  int band_off[3];            // offset of this level's HL band inside a component record
  int band_n[3];              // coefficients per band block (bsh * bsw)
  int band;                   // band index of HL at this level (for the quant matrix)
  int ys, xs, slice_coefs;
  int rec_stride[3];          // tile kernels (vc2hip_dwt_fast.hip): elements from one slice's coefficients of a component to the next
                              // slice's -- slice_coefs in the slice records, HeadSplit::n[c] in the record heads
  int word_bytes, sample_shift, sample_offset; // raw sample format (luma; the decoder's one format)
  int sample_shift_c, sample_offset_c;         // FIRST: the chroma words' (EncodeStream -c: its own depth)
  // The caller's sample layout (vc2hip_set_sample_layout).  A sample is sample_bits bits of its word
  // from bit sample_shift up (MSB-justified words: 8 * word_bytes - depth; LSB-justified: 0); FIRST ignores every other bit.
  int sample_bits, sample_bits_c;              // FIRST: the depth of the luma / chroma words
  unsigned sample_mask, sample_mask_c;         // FIRST: (1 << sample_bits) - 1 (all ones at 32 bits)
  int sample_le;                               // the words are little-endian (the byte loops; one-byte words: no effect)
  // 16-bit words, two per dword: the v_perm selectors of the byte order.  perm_rd: perm(w, w, perm_rd) has the first word of the
  // dword w in its low half; perm_wr: perm(b, a, perm_wr) is the low halves of a (first) and b as the layout's words.
  unsigned perm_rd, perm_wr;
  int clip_lo, clip_hi;
  int ll_from_store;          // inverse, coarsest level: LL comes from store band 0 (dequantised)
  int ll_to_store;            // forward, last level: LL goes to store band 0
  int dequant;                // inverse: apply scale() to store values
  unsigned *err;              // device error flags
  int debug_skip;             // -DVC2HIP_ABLATE builds only (tools/ablate_*.py): 1 no loads, 2 no lifting, 4 no stores
  int qmatrix[VC2_MAX_BANDS];
  // streaming kernels (vc2hip_dwt_stream.hip), set by vc2_stream_level_applicable
  int st_strips[3], st_segs[3]; // wavefronts across / down a plane (segments: whole rows of slices)
  int st_out[3];                // chunks (8 samples) a strip owns
  int st_llps[3];               // log2 chunks per slice
  int st_tail;                  // some plane's pair count is not a multiple of four: the TAIL instantiation
  int st_prio;                  // > 0: wavefronts take turns at the highest issue priority, a new turn every 2^st_prio row pairs
  int st_segmax, st_npic;       // most segments of any component; pictures of the launch (the kernels' work-item numbering)
  int st_lds;                   // dynamic LDS bytes of ONE wavefront (a workgroup holds VC2_STREAM_WG_WAVES of them)
  // inverse, streaming kernels: element offset (from the picture's store) of this level's HL band plane, LH and HH behind
  // it, when the decoder keeps the level's bands as planes (BandPlanes below); -1: in the slice records
  long long bp_base[3];
  int bp8;                      // those planes hold one byte per coefficient (BandPlanes::bytes8)
  // FINAL, reduced pictures (vc2hip_decode_reduced_batch_dev): the low-pass gain of the dropped levels leaves before the
  // clip, x = (x + (1 << (norm_shift - 1))) >> norm_shift; 0: the full decoder (the test is wave-uniform)
  int norm_shift;
};
// the normalisation of a reduced picture's samples (LevelParams::norm_shift); n > 0
__device__ __forceinline__ int vc2_norm(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// The one mapping from a picture of a batch to its raw words (every FIRST / FINAL address, both directions): progressive
// pictures lie pic * stride apart; field pictures (field_shift 1) are fields of interleaved frames, picture pic the field
// pic & 1 of frame pic >> 1, the second field field_step bytes from the first.  A field's rows are raw_pitch (two frame
// rows) apart, so the two fields of a frame never share a byte.  field_step is +-one frame row: a multiple of 16 bytes
// wherever the rows are (the 16-byte raw loads and stores of every kernel require that of the rows), so the second
// field's base keeps every alignment the first one has.
__host__ __device__ __forceinline__ long long vc2_raw_pic_offset(long long stride, int field_step, int field_shift, int pic) {
  return (long long)(pic >> field_shift) * stride + (long long)(pic & field_shift) * field_step;
}
__host__ __device__ __forceinline__ long long vc2_raw_pic_offset(const LevelParams &p, int comp, int pic) {
  return vc2_raw_pic_offset(p.plane_stride[comp], p.field_step[comp], p.field_shift, pic);
}

// the raw words of one component of a batch, as LevelParams holds them (plane_stride, raw_pitch, field_step, field_shift)
struct RawPlane {
  long long stride;
  int pitch, field_step, field_shift;
  int le, lsb; // the words' byte order and justification (vc2hip_sample_layout; 0, 0: the file format)
};
#define VC2_PERM_RD_BE 0x02030001u
#define VC2_PERM_RD_LE 0x03020100u
#define VC2_PERM_WR_BE 0x04050001u
#define VC2_PERM_WR_LE 0x05040100u
// one raw word of wb bytes in the layout's byte order (the element-wise paths of every FIRST / FINAL form)
__device__ __forceinline__ unsigned vc2_load_word(const uint8_t *q, int wb, int le) {
  unsigned u = 0;
  if (le) for (int b = 0; b < wb; ++b) u |= (unsigned)q[b] << (8 * b);
  else for (int b = 0; b < wb; ++b) u = (u << 8) | q[b];
  return u;
}
__device__ __forceinline__ void vc2_store_word(uint8_t *q, unsigned u, int wb, int le) {
  for (int b = 0; b < wb; ++b) q[b] = (uint8_t)(u >> (8 * (le ? b : wb - 1 - b)));
}

// Two consecutive levels in one launch (vc2hip_dwt_pair.hip): `a` is the finer level exactly as the one-level kernels see
// it (its st_* fields describe the wavefronts: a lane holds 8 samples of level a's input plane), `b` the level below it
// (fill_level of level + 1: the same lanes hold 4 samples of ITS input, which never leave the registers).
struct PairParams {
  LevelParams a, b;
  int spl[3];        // slices per lane: 1, or 2 when a slice footprint at level a is 4 samples wide (then st_llps = 0)
  int img_b;         // LDS images of level b: byte offset behind level a's (forward)
  int grp_a;         // forward: slice rows per burst of stores = images of level a (a power of two); level b has grp_a + 1
  int sz_a, sz_b;    // forward: elements of one image of level a / b
  int ring_ll, n_ll; // forward: byte offset and rows (a power of two) of the ring of level b's LL rows
  int ss_a[3], ss_b[3]; // forward: elements from one slice's run to the next in the LDS images (padded against bank conflicts)
  int piece_a[3], piece_b[3]; // forward: bytes per flush piece (16, 8 or 4)
};

// Tuning knobs (lanes per slice, wavefronts per workgroup, segments per strip ...) are compile-time decisions of the
// release library; the environment can override them only in the -DVC2HIP_ABLATE build (A/B measurements on one box).
#include <stdlib.h>
#ifdef VC2HIP_ABLATE
static inline int vc2_tune_int(const char *name, int def) { const char *e = getenv(name); return e ? atoi(e) : def; }
#else
static inline int vc2_tune_int(const char *, int def) { return def; }
#endif

// Work-skipping switches for the timing experiments of tools/ablate_*.py exist only in a library built with
// -DVC2HIP_ABLATE (the tools build their own); the release kernels carry no such test.
#ifdef VC2HIP_ABLATE
#define VC2_SKIP(p, bit) (((p).debug_skip & (bit)) != 0)
#else
#define VC2_SKIP(p, bit) false
#endif

struct PackParams {
  const void *store;          // int32_t or int16_t elements (store16)
  const int32_t *store_wide;
  int store16;
  long long store_stride;
  const int32_t *qidx;        // n_pictures * n_slices (ConstQ: filled by host)
  int n_slices, slice_coefs;
  int comp_n[3], comp_off[3], comp_n0[3];
  int depth;
  int prefix, scalar;
  int qmatrix[VC2_MAX_BANDS];
  // VBR: fixed-stride slots + sizes; CBR: direct
  uint8_t *slots;             // n_pictures * n_slices * slot_bytes
  int slot_bytes;
  uint32_t *sizes;            // n_pictures * n_slices (tile_slices: n_pictures * workgroups per picture)
  int tile_slices;            // > 0: the slices of a pack workgroup (that many) share a slot of tile_slices * slot_bytes, back to back
  const int32_t *cbr_bytes;   // per slice (one picture's worth, shared), NULL => VBR
  const uint32_t *cbr_offsets;
  uint8_t *payload;
  long long payload_stride;
  unsigned *err;
  int quantise;               // 0: store already holds quantised values (fine-grained API)
  int big_lut;                // set by the launcher: LDS holds subband tables for components of up to 2048 coefficients
  float inv_scalar;           // set by the launcher: the smallest float >= 1 / scalar
  union {
    unsigned char band_lut[768]; // set by the launcher: subband of a coefficient index, 512 luma + 256 chroma entries
    unsigned lane16[200];        // k_hq_pack16 / k_hq_pack16w (vc2hip_pack16.h): per lane, the matrix entries of its coefficients; head / body sizes
  };
  int debug_skip;             // timing experiments only (VC2HIP_DEBUG_PACK): 1 no code writes, 2 no copy-out
  // single-pass VBR: slice offsets by decoupled look-back over workgroup tiles (4 slices each).
  // lookback: per picture [0] = tile ticket, [1 + t] = status of tile t: flag (2 bits) << 62 | bytes
  unsigned long long *lookback;
  long long lookback_stride;  // u64 words per picture
  unsigned long long *lens;   // per picture payload length (written by the last tile)
};

// Decode side only: the bands of the finest levels -- those the streaming inverse kernels read -- are kept as whole
// planes behind the slice records instead of inside them.  The inverse transform then reads every band row with fully
// coalesced loads (lanes = neighbouring columns) where the slice records give it 8 or 16 bytes per slice at slice-record
// distance; the slice decoder, whose lanes are neighbouring slices, writes a band row piece per lane, also contiguous.
// (The encoder keeps slice records throughout: its transform is not bound by the store writes.)
constexpr int VC2_BP_MAX = 3;
struct BandPlanes {
  int levels;                       // finest levels kept as planes (0: none)
  int bytes8;                       // round 5: a plane element is ONE BYTE (quantised coefficients are small; -128 = escape: the value is in
                                    // the wide array at the element's index, like the 16-bit sentinel's).  A plane that starts at element
                                    // `base` of the picture's store keeps its start; element e of it lives at byte 2 * base + (e - base).
  int from[3];                      // first coefficient of a component record that lives in a plane
  long long base[3][VC2_BP_MAX];    // element offset, from the picture's store, of band 1 (HL) of level l; LH, HH follow
  int ow[3][VC2_BP_MAX], np[3][VC2_BP_MAX];     // width / height of a band plane
  int lbsh[3][VC2_BP_MAX], lbsw[3][VC2_BP_MAX]; // log2 of a slice's block in it
};

// Record heads: the coefficients of the DEEP levels (those below the streaming kernels: LL and the bands of levels >= Ls) are
// the first head_n[c] coefficients of every component record -- 8 to 64 bytes per component at slice-record distance, and
// the tile kernels of those levels fetched (wrote) a whole 128-byte line for each (3.6 - 7 x their bytes, rocprofv3
// FETCH_SIZE).  With a head split they live in one dense array per component instead: [slice][coefficient]; inside a
// slice the order is that of the record, so the deep levels see a coefficient store with rec_stride[c] = n[c] and
// coef_off[c] = base[c].
struct HeadSplit {
  int n[3];            // coefficients of a component record that live in the head (0: no split); multiples of 8
  long long base[3];   // element offset, from the picture's store, of the component's head array: [slice][n[c]]
};

struct UnpackParams {
  const uint8_t *payload;
  long long payload_stride;
  const unsigned long long *lens; // per picture
  const uint32_t *offsets;    // n_pictures * n_slices slice start offsets
  void *store;                // int32_t or int16_t elements (store16)
  int32_t *store_wide;
  int store16;
  long long store_stride;
  int32_t *qidx;
  int n_slices, slice_coefs;
  int comp_n[3], comp_off[3];
  int prefix, scalar;
  unsigned *err;
  BandPlanes bp;
  HeadSplit hs;
  int xs;                     // slices across
  unsigned long long *stats;  // [0]: pieces that carried an escape from a byte plane (k_hq_unpack16<true>; feedback for the next batch's layout)
  int debug_skip;             // timing experiments only (VC2HIP_DEBUG_UNPACK, -DVC2HIP_ABLATE): 1 stream reads from a hot 16 KiB window, 2 no stores
};

struct CbrParams {
  const void *store;          // int32_t or int16_t elements (store16)
  const int32_t *store_wide;
  int store16;
  long long store_stride;
  int32_t *qidx;
  const int32_t *slice_bytes;
  int n_slices, slice_coefs;
  int comp_n[3], comp_off[3], comp_n0[3];
  int scalar;
  int n_bands;
  int qmatrix[VC2_MAX_BANDS];
  unsigned *err;
  int only_marked;            // set by the launcher: search only the slices whose index is VC2_CBR_MARK (1: a small grid walks the
                              // picture for the few there are; 2: a wavefront per slice, as many may be marked as not)
  int clamp_refused;          // set by vc2_launch_cbr_marked: a slice the general kernel refuses at its first trial is left at
                              // 119 + qm_min, not 127 -- the slice coder behind the search then raises no error of its own
  int general_only;           // VC2HIP_FLAG_CBR_GENERAL: no register kernel (tests, A/B)
  float inv_scalar;           // set by the launcher
  int qm_min;                 // set by the launcher: the smallest matrix entry
  union {
    unsigned char band_lut[768]; // set by the launcher: subband of a coefficient index, 512 luma + 256 chroma entries
    unsigned lane8[72];          // k_cbr_search16 (vc2hip_cbr16.h): per lane the matrix entries of its runs and head; [64..67] head / run counts
  };
};
#define VC2_CBR_MARK 0x7FFFFFFF

// HQ_CAPPED (vc2hip_cap.h): one index per picture, the smallest of floor .. VC2_CAP_Q_TOP whose
// ConstQ payload is at most cap bytes.  Two rounds of measure + pick over a per-picture table of VC2_CAP_ROW u64 words:
//   [0 .. 14]  round 1: the picture's payload bytes at floor + 8 k (a candidate that cannot be coded: >= VC2_CAP_NOFIT)
//   [16 .. 22] round 2: the same at base + 1 + j, j < count
//   [24] base, [25] count, [26] the index if none of round 2 fits (written by the first pick)
//   [27] q_i, [28] fill: 1 where the picture left the floor and fits at q_i, [29] spare = cap - L(q_i)
//              (written by the second pick: what HQ_CAPPED_FILL's third round and k_cap_fill read)
#define VC2_CAP_Q_TOP 115
#define VC2_CAP_ROW 32
#define VC2_CAP_R2 16
#define VC2_CAP_BASE 24
#define VC2_CAP_COUNT 25
#define VC2_CAP_ELSE 26
#define VC2_CAP_QI 27
#define VC2_CAP_FILL 28
#define VC2_CAP_SPARE 29
#define VC2_CAP_NOFIT (1ull << 40)
#define VC2_CAP_NOCOST 0xFFFFFFFFu // HQ_CAPPED_FILL: the slice cannot be coded at q_i - 1
struct CapParams {
  CbrParams s;                // store, geometry, matrix as the HQ_CBR search has them; qidx: the marks of the handed-back slices, then the result
  unsigned long long *table;  // n_pictures * VC2_CAP_ROW, zero before the first round
  unsigned long long cap;
  int prefix, floor;
  int round;                  // 0 / 1; 2: HQ_CAPPED_FILL's per-slice round
  unsigned *cost;             // HQ_CAPPED_FILL (null otherwise): n_pictures * n_slices, len_s(q_i - 1) - len_s(q_i) or VC2_CAP_NOCOST
  const int8_t *offs;         // vc2hip_set_index_offsets (null: none, the kernels without a map run): slice s of picture i reads
  long long offs_stride;      // offs[i * offs_stride + s]; 0: one map for every picture.  Any alignment
};

// ------------------------------------------------------------------------------------------
// launchers (implemented in the kernel TUs)
// ------------------------------------------------------------------------------------------
struct Launcher; // profiling hook, defined in vc2hip_api.hip
// Every kernel launch goes through VC2_LAUNCH between vc2_prof_begin / vc2_prof_end.  With profiling on it carries
// its own start / stop events (hipExtLaunchKernelGGL: the timestamps of the dispatch packet itself, no extra packets
// on the stream between kernels); off, the events are null and it is a plain launch.
void vc2_prof_pair(Launcher &L, hipEvent_t *a, hipEvent_t *b);
#define VC2_LAUNCH(L, kernel, grid, block, lds, s, ...)                                        \
  do {                                                                                         \
    hipEvent_t vc2_ev_a_, vc2_ev_b_;                                                           \
    vc2_prof_pair(L, &vc2_ev_a_, &vc2_ev_b_);                                                  \
    hipExtLaunchKernelGGL(kernel, grid, block, lds, s, vc2_ev_a_, vc2_ev_b_, 0, __VA_ARGS__);  \
  } while (0)

// Raise a kernel's dynamic-LDS limit to `bytes`, once per (kernel, device): the attribute belongs to the
// function on the CURRENT device, and one process may drive several GPUs (the tools' --gpus N).
void vc2_allow_lds(const void *kernel, size_t bytes);

void vc2_upload_tables(const QuantTables &t, hipStream_t s);
int vc2_launch_forward_level(Launcher &L, int kernel, bool first, const LevelParams &p, int n_pictures,
                             hipStream_t s); // generic kernels: int32 store and planes only
int vc2_launch_inverse_level(Launcher &L, int kernel, bool final_level, const LevelParams &p,
                             int n_pictures, hipStream_t s);
size_t vc2_level_lds_bytes(int kernel, const LevelParams &p);

void vc2_launch_pack(Launcher &L, const PackParams &p, int n_pictures, hipStream_t s);
int vc2_pack_slices_per_tile(const PackParams &p);
bool vc2_pack_one_pass_default(const PackParams &p); // VBR slices coded by k_hq_pack16: look-back, no slots
void vc2_launch_scan_sizes(Launcher &L, const uint32_t *sizes, uint32_t *offsets,
                           unsigned long long *totals, int n_slices, int n_pictures, hipStream_t s);
void vc2_launch_compact(Launcher &L, const uint8_t *slots, int slot_bytes, const uint32_t *sizes,
                        const uint32_t *offsets, uint8_t *payload, long long payload_stride,
                        int n_slices, int n_pictures, hipStream_t s);
void vc2_launch_cbr(Launcher &L, const CbrParams &p, int n_pictures, hipStream_t s);
void vc2_launch_cap(Launcher &L, const CapParams &p, int n_pictures, hipStream_t s);
// HQ_CONSTQ under vc2hip_set_index_offsets: qidx[i, s] = min(max(base + offs[i * offs_stride + s], 0), VC2_CAP_Q_TOP)
void vc2_launch_q_offsets(Launcher &L, int32_t *qidx, const int8_t *offs, long long offs_stride, int base, int n_slices,
                          int n_pictures, hipStream_t s);
void vc2_launch_unpack(Launcher &L, const UnpackParams &p, int n_pictures, hipStream_t s);
void vc2_launch_cbr_index(Launcher &L, const uint8_t *payload, long long stride, const unsigned long long *lens, const int32_t *budget,
                          const uint32_t *cbr_offs, unsigned long long total, uint32_t *offsets, int n_slices, int prefix, int scalar,
                          int n_pictures, unsigned *bad, hipStream_t s);
void vc2_launch_slice_index(Launcher &L, const uint8_t *payload, long long payload_stride,
                            const unsigned long long *lens, uint32_t *offsets, int n_slices,
                            int prefix, int scalar, int n_pictures, unsigned *err, hipStream_t s,
                            void *workspace, size_t workspace_bytes, const unsigned *skip = nullptr);
size_t vc2_slice_index_workspace(int n_pictures, size_t max_payload, int prefix, int scalar);

// layout conversion for the fine-grained API (interleaved in-place plane <-> coefficient store)
void vc2_launch_plane_to_store(Launcher &L, const int32_t *plane, int ph, int pw, int depth, int ys,
                               int xs, int32_t *store, int slice_coefs, int coef_off, hipStream_t s);
void vc2_launch_store_to_plane(Launcher &L, const int32_t *store, int slice_coefs, int coef_off,
                               int32_t *plane, int ph, int pw, int depth, int ys, int xs,
                               const int32_t *qidx, const int *qmatrix, int mode /*0 copy,1 scale*/,
                               unsigned *err, hipStream_t s);
void vc2_launch_quantise_store(Launcher &L, int32_t *store, int n_slices, int slice_coefs, int comp_n,
                               int comp_off, int n0, const int32_t *qidx, const int *qmatrix,
                               unsigned *err, hipStream_t s);
// LD: DC-predicted reconstruction of the LL band of one component (Quantisation.cpp:287-306)
struct LdLl3Params {
  const int32_t *store;
  long long store_stride;
  int slice_coefs, coef_off[3], llh[3], llw[3], ys, xs;
  const int32_t *qidx;
  int qm0;
  int32_t *ll_plane[3];
  long long ll_stride[3];
  unsigned *err;
};
bool vc2_launch_ld_ll3(Launcher &L, const LdLl3Params &p, int n_pictures, hipStream_t s); // false: a plane does not fit in LDS (use vc2_launch_ld_ll)
void vc2_launch_ld_ll(Launcher &L, const int32_t *store, long long store_stride, int slice_coefs,
                      int coef_off, int n0, int llh, int llw, int ys, int xs, const int32_t *qidx,
                      int qm0, int32_t *ll_plane, long long ll_stride, int n_pictures, unsigned *err,
                      hipStream_t s);
struct LdUnpackParams {
  const uint8_t *payload;
  long long payload_stride;
  const int32_t *slice_bytes; // per slice
  const uint32_t *offsets;    // per slice (prefix sums of slice_bytes)
  int32_t *store;
  long long store_stride;
  int32_t *qidx;
  int n_slices, slice_coefs;
  int comp_n[3], comp_off[3];
  unsigned *err;
  // A slice whose luma length field exceeds the slice (corrupt data; also what the reference's decoder makes of its own
  // interlaced LD streams, DecodeStream.cpp:331): the reference reads that many bits from the stream (Slices.cpp:246-303),
  // so every later slice of the picture starts late.  The first pass decodes at the nominal offsets and raises the
  // picture's flag when it meets such a slice; a serial walk then finds the true starts of a flagged picture and a second
  // pass decodes it again from those (both return at once for pictures without the flag).
  const unsigned long long *lens; // per picture: payload bytes the decoder may look at (null: payload_stride)
  unsigned *shifted;              // per picture: flag (null: no such handling, slices stay at their nominal offsets)
  uint32_t *starts;               // per picture x slice: true start offsets of a flagged picture
  int redo;                       // the second pass
};
void vc2_launch_ld_unpack(Launcher &L, const LdUnpackParams &p, int n_pictures, hipStream_t s);
void vc2_launch_ld_walk(Launcher &L, const LdUnpackParams &p, int n_pictures, hipStream_t s);

// LD encode: quantiser search / DC-predicted quantisation (one launch per slice anti-diagonal) and
// the slice writer
struct LdEncParams {
  int32_t *store;             // in: transform coefficients; out: quantised (LL as prediction residuals)
  int32_t *scratch;           // slices too large for LDS: the trials' quantised values, same shape as the store (null: such slices are refused)
  long long store_stride;
  int32_t *qidx;              // n_pictures * n_slices; written when search != 0
  const int32_t *slice_bytes; // per slice
  const uint32_t *offsets;    // per slice (prefix sums of slice_bytes)
  int32_t *restored[3];       // reconstructed LL planes (scratch), ll_h x ll_w per picture
  long long restored_stride[3];
  int ll_w[3];
  int bh[3], bw[3];           // LL block of one slice
  int ys, xs, n_slices, slice_coefs;
  int comp_n[3], comp_off[3], comp_n0[3];
  int depth;
  int rs_ints;                // LDS ints per wavefront for the LL blocks with their halo: sum of (bh + 1) * (bw + 1)
  int qmatrix[VC2_MAX_BANDS];
  int search;
  int diagonals;              // VC2HIP_FLAG_LD_DIAGONALS: one launch per slice anti-diagonal instead of the single-launch search
  int *tab;                   // device scratch for the search tables (LD_TAB_INTS ints)
  int img_words;              // LDS words of one slice image (pack)
  uint8_t *payload;
  long long payload_stride;
  unsigned *err;
  int debug_dead_row;         // -DVC2HIP_ABLATE builds only: the workgroup of this slice row of picture 0 exits at once (hand-over failure test)
};
void vc2_launch_ld_quantise(Launcher &L, const LdEncParams &p, int n_pictures, hipStream_t s);
void vc2_launch_ld_pack(Launcher &L, const LdEncParams &p, int n_pictures, hipStream_t s);

// The picture the decoder will show, without a payload (vc2hip_recon.hip; vc2hip_encode_recon_batch_dev)
// HQ: the encoder's slice records (transform coefficients) -> quantised values in the decoder's layout (slice records, band
// planes, record heads: what the inverse level kernels read and dequantise).  16-bit elements on both sides, or int32 on both.
struct RequantParams {
  const void *src;            // the encoder's store: int16_t (store16) or int32_t elements
  const int32_t *src_wide;
  long long src_stride;       // per picture, elements
  void *dst;                  // the decoder-layout store, same element type (null: the checks only)
  int32_t *dst_wide;
  long long dst_stride;
  int store16;
  const int32_t *qidx;        // n_pictures * n_slices
  int n_slices, slice_coefs, xs;
  int comp_n[3], comp_off[3], comp_n0[3];
  int n_bands;
  int qmatrix[VC2_MAX_BANDS];
  BandPlanes bp;              // 16-bit planes only (bytes8 == 0)
  HeadSplit hs;
  // check != 0 (no payload was asked for): what the slice coder would have found -- a code beyond 32 bits, a component
  // beyond 255 * scalar bytes, an HQ_CBR slice whose V component does not fit (k_hq_pack / k_hq_pack16: comp_len, cbr_v)
  int check, scalar;
  const int32_t *cbr_bytes;   // HQ_CBR: per slice budgets; null: VBR
  unsigned *err;
  int grp_log2;               // set by the launcher: log2 of the lanes that share a slice record
};
void vc2_upload_tables_recon(const QuantTables &t, hipStream_t s);
void vc2_launch_requantise(Launcher &L, const RequantParams &p, int n_pictures, hipStream_t s);
// LD without a payload: the checks of the slice writer (k_ld_pack) on the quantised store
void vc2_launch_ld_check(Launcher &L, const LdEncParams &p, int n_pictures, hipStream_t s);
// sums of squared sample differences of two raw buffers, per picture and component: sse[3 * pic + comp] += ...
struct SseParams {
  const uint8_t *a, *b;       // n pictures each, in one layout; both 16-byte aligned
  long long pic_bytes;        // from one picture's base to the next
  long long comp_at[3];       // a component's first row inside a picture
  long long row_bytes[3], pitch[3]; // its rows: bytes of one, bytes from one to the next.  Tight rows are handed over as ONE row
  int rows[3];                // of rows * row_bytes bytes; several rows: each starts on a 16-byte boundary (the layout's rule)
  int word_bytes, shift;      // sample = (word >> shift) & mask, the word in the layout's byte order
  unsigned mask;
  int le;
  unsigned long long *sse;
};
void vc2_launch_squared_error(Launcher &L, const SseParams &p, int n_pictures, hipStream_t s);

// Coded pictures to a coarser index without leaving the coefficient domain (vc2hip_transcode.hip;
// vc2hip_transcode_batch_dev).  Slice s of picture i ends at max(its own index, q_i); a slice that
// keeps its index keeps its coefficient values.  q_i is the call's target, or with a cap the smallest index of
// target .. VC2_CAP_Q_TOP whose output is at most cap bytes, found in two rounds over the HQ_CAPPED table layout
// (VC2_CAP_ROW words per picture; the table holds the sum of the components' bytes, the pick adds the slice headers).
struct TranscodeParams {
  const uint8_t *in;              // input slots
  long long in_stride;
  const unsigned long long *in_lens;
  const uint32_t *in_offs;        // n_pictures * n_slices slice starts of the input (the decoder's slice index)
  // the context's coefficient store after the decoder's slice reader: slice records, no band planes, no record heads
  void *store;                    // int16_t (store16) or int32_t elements
  int32_t *store_wide;            // store16: the escapes
  int store16;
  long long store_stride;         // per picture, elements
  int slice_coefs, comp_off[3];
  const int32_t *qs;              // n_pictures * n_slices: the input slices' indices, as the reader left them
  int32_t *qpack;                 // n_pictures * n_slices: what the slice coder is handed (k_transcode_scale)
  int32_t *qidx_out;              // n_pictures * n_slices: the indices the output slices carry; may be null
  unsigned long long *table;      // capped: n_pictures * VC2_CAP_ROW, zero before the first round
  int32_t *qpic;                  // capped: n_pictures chosen indices
  int n_slices;
  int comp_n[3], comp_n0[3];
  int prefix, scalar;
  int target;                     // tp->q_index
  int capped;
  unsigned long long cap;
  int round;                      // measure / pick: 0 and 1, the two rounds of the capped search
  int qmatrix[VC2_MAX_BANDS];
  int qm_min;                     // the smallest matrix entry: a slice's index q is refused when q - qm_min > 119, as the decoder refuses it
  unsigned *err;
  // vc2hip_transcode_cbr_batch_dev: the output's budgets, one picture's worth, and its size scalar
  const int32_t *out_budgets;
  int out_scalar;
};
void vc2_upload_tables_transcode(const QuantTables &t, hipStream_t s);
void vc2_launch_transcode_measure(Launcher &L, const TranscodeParams &p, int n_pictures, hipStream_t s);
void vc2_launch_transcode_pick(Launcher &L, const TranscodeParams &p, int n_pictures, hipStream_t s);
void vc2_launch_transcode_scale(Launcher &L, const TranscodeParams &p, int n_pictures, hipStream_t s);
// To a per-slice byte budget (vc2hip_transcode_cbr_batch_dev): between the slice reader and the HQ_CBR search.  A slice whose
// values fit its budget as they are is KEPT (qpack: its index - 256, the coder's identity); every other slice is
// dequantised in place and marked for the search (qpack: VC2_CBR_MARK, which vc2_launch_cbr_marked replaces).
void vc2_launch_transcode_fit(Launcher &L, const TranscodeParams &p, int n_pictures, hipStream_t s);
// Behind the slice coder: d_qidx from qpack, and the order of the composition's refusals (the reader's comes first)
void vc2_launch_transcode_settle(Launcher &L, const TranscodeParams &p, int n_pictures, hipStream_t s);
// The HQ_CBR search (vc2_launch_cbr's general kernel) over the slices whose index is VC2_CBR_MARK and no other
void vc2_launch_cbr_marked(Launcher &L, const CbrParams &p, int n_pictures, hipStream_t s);

// packed and semi-planar pictures <-> planar staging (vc2hip_packed.hip, vc2hip_set_packed_format)
struct PackedParams {
  uint8_t *packed;            // the caller's buffer: picture 0's first v210 row / first row of its UV plane
  long long packed_stride;    // bytes per picture
  int packed_pitch;           // bytes from one of those rows to the next
  uint8_t *plane[3];          // staging planes of picture 0 (the UV kernels use [1] and [2]); rows start on 16-byte boundaries
  long long plane_stride;     // bytes per picture
  int plane_pitch[3];
  int rows;                   // rows of the caller's plane
  int width;                  // v210: luma samples of a row; UV: word pairs of a row (the chroma width)
  int v210;                   // 1: the v210 kernels, 0: the UV kernels at word_bytes 1 or 2
  int word_bytes;
  int vec;                    // UV: every row of the caller's plane starts on a 16-byte boundary (16-byte pieces)
};
// pack: staging -> the caller's buffer; else the caller's buffer -> staging
void vc2_launch_packed(Launcher &L, const PackedParams &p, bool pack, int n_pictures, hipStream_t s);

// VC-2 stream I/O (vc2hip_stream.hip)
// Picture header bytes the write kernels carry.  The longest vc2hip_picture_header_qm writes: 4 bytes of picture number; wavelet
// and depth (at most 5 + 7 bits for 0 .. 6 and 0 .. 7 with a matrix); two flags; slice counts, prefix / numerator and scalar /
// denominator, four codes of at most 63 bits (values below 2^31); the matrix flag; 22 entries of at most 17 bits (0 .. 255):
// 12 + 2 + 252 + 1 + 374 = 641 bits = 81 bytes, 85 in all.
#define VC2_STREAM_HDR_MAX 96
struct StreamWriteParams {
  const uint8_t *payload;           // slots
  long long payload_stride;
  const unsigned long long *lens;   // n payload lengths
  unsigned long long *unit_off;     // workspace: n unit offsets
  uint8_t *stream;
  unsigned long long cap;
  unsigned long long *stream_len;
  unsigned *err;
  int n, hdr_len, code, eos;
  uint32_t first_picture_number, prev_parse_offset;
  uint8_t hdr[VC2_STREAM_HDR_MAX]; // picture header of picture 0 (its number in bytes 0-3 is replaced per picture)
};
struct StreamSeg { unsigned long long src; uint32_t dst, len; }; // payload bytes [dst, dst + len) are stream bytes [src, ...)
struct StreamReadParams {
  const uint8_t *stream;
  unsigned long long len;
  int n, major_version;
  int kernel, depth, ys, xs, ld;    // what every picture must carry
  uint32_t a, b;                    // HQ: prefix, scalar.  LD: the slice-bytes fraction in lowest terms
  int qmatrix[VC2_MAX_BANDS];       // the context's effective matrix: what a picture's own matrix must equal, entry by entry
  int qm_entries;                   // 3 * depth + 1; 0: depth beyond 7, a picture with a matrix is refused
  int flagless_ok;                  // that matrix is the default of (kernel, depth): pictures without a matrix of their own pass
  StreamSeg *segs;                 // workspace: n * seg_cap
  uint2 *meta;                      // workspace: per picture {segments, payload bytes}
  int seg_cap;
  uint8_t *payload;                 // slots
  long long payload_stride;
  unsigned long long *lens;
  uint32_t *picture_numbers;        // may be null
  unsigned long long *consumed;     // may be null
  unsigned *err;
};
// fragmented pictures (vc2hip_stream_write_fragments_dev)
#define VC2_FRAG_HEADER 25 // parse info, picture number, data length, slice count, slice offset x and y
struct FragParams {
  const uint8_t *payload;           // slots
  long long payload_stride;
  const unsigned long long *lens;   // n payload lengths
  const uint32_t *offs;             // slice start bytes: HQ offs[k * ns + i] (the decoder's slice index), LD offs[i] (the budget table's)
  long long offs_stride;            // ns (HQ) or 0 (LD)
  unsigned long long ld_total;      // LD: the table's sum
  int hq, prefix, scalar;
  int n, ns, xs;
  unsigned fragment_length;
  uint4 *table;                     // workspace: n * ns fragments {first slice, first payload byte, bytes, slices}
  uint4 *meta;                      // workspace: per picture {slice fragments, payload bytes, bytes of the last fragment, 0}
  unsigned long long *pic_base;     // workspace: n stream offsets of the pictures' parameters fragments
  unsigned long long *unit_base;    // workspace: n indices of those units in the stream
  unsigned *jump;                   // workspace of the cut when a picture's slices do not fit LDS, else null
  uint8_t *stream;
  unsigned long long cap;
  unsigned long long *stream_len;
  unsigned long long *unit_offsets; // may be null
  unsigned long long unit_cap;
  unsigned long long *unit_count;   // may be null
  unsigned *err;
  int code, eos, tp_len;
  uint32_t first_picture_number, prev_parse_offset;
  uint8_t tp[VC2_STREAM_HDR_MAX];   // transform parameters
};
size_t vc2_frag_cut_lds(int ns);        // dynamic LDS of the cut, 0: the slices do not fit (FragParams::jump)
size_t vc2_frag_jump_bytes(int ns);     // that workspace, per picture
void vc2_launch_frag_cut(Launcher &L, const FragParams &p, hipStream_t s);
void vc2_launch_frag_layout(Launcher &L, const FragParams &p, hipStream_t s);
void vc2_launch_frag_copy(Launcher &L, const FragParams &p, hipStream_t s);
void vc2_launch_stream_layout(Launcher &L, const StreamWriteParams &p, hipStream_t s);
void vc2_launch_stream_copy(Launcher &L, const StreamWriteParams &p, hipStream_t s);
void vc2_launch_stream_walk(Launcher &L, const StreamReadParams &p, hipStream_t s);
void vc2_launch_stream_gather(Launcher &L, const StreamReadParams &p, hipStream_t s);
