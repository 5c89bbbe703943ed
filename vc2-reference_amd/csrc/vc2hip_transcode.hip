// Coded HQ pictures to a coarser quantiser index without leaving the coefficient domain
// (vc2hip_transcode_batch_dev).
//
// Slice s of picture i ends at q' = max(its own index, q_i).  A slice with q' == its own index keeps its coefficient
// values (no arithmetic); every other coefficient becomes quant(scale(c, q_s), q') with the default matrix, per band
// max(q - matrix[band], 0), as everywhere.  The output is a plain HQ VBR payload at the same prefix and scalar.
//
// The call is the decoder's slice index and slice reader (vc2hip_slices.hip, unchanged), one kernel of this file, and the
// encoder's slice coder (unchanged):
//   hq_unpack          quantised coefficients into the context's store as slice records, every slice's index beside them
//   transcode_scale    coefficient-parallel: the slices that end at a coarser index are dequantised in place, scale(c, q_s);
//                      the coder then quantises at q' -- quant(scale(c, q_s), q').  Kept slices stay as they are and go to
//                      the coder under q_s - 256, which writes q_s and quantises by the identity (see the kernel)
//   hq_pack (...)      the slice coder on the store: lengths, offsets, d_lens, the payload, ESCALAR / ECODE32
// The capped form finds each picture's index before that, from the payload:
//   transcode_measure  one lane per slice component (64 slices x Y, U, V per workgroup): a table-driven decode by the
//                      decoder's own look-up table (vc2_unpack_lut_host), requantised for up to 15 candidate indices at
//                      once, bits through the last non-zero coefficient -> the picture's bytes per candidate
//   transcode_pick     the picture's index from the table of candidate lengths, two rounds (vc2hip_cap.h's rule)
// The measuring reader is bounded to the component, bits past the bound read as 1; every input address is clamped to
// min(d_lens[i], stride).
// To a per-slice byte budget (vc2hip_transcode_cbr_batch_dev) the same reader is followed by
//   transcode_fit      one wavefront per slice: the bytes the slice's values need as they are; a slice that fits its HQ_CBR
//                      budget is kept (q_s - 256 again), every other one is dequantised in place and marked
//   cbr_search (...)   the encoder's HQ_CBR search over the marked slices alone (vc2_launch_cbr_marked, vc2hip_slices.hip)
//   hq_pack (...)      the slice coder in its CBR form, at the output's prefix and scalar
//   transcode_settle   d_qidx, and the reader's refusal ahead of what the coders made of a broken picture
#include "vc2hip_internal.h"
#include "vc2hip_store.h"

#include <algorithm>

void vc2_prof_begin(Launcher &L, const char *name, hipStream_t s);
void vc2_prof_end(Launcher &L, hipStream_t s);

const unsigned *vc2_unpack_lut_host(); // vc2hip_slices.hip: the decoder's look-up table of the next 10 stream bits

__constant__ QuantTables c_qt;
namespace {
constexpr int TC_LUT_BITS = 10, TC_LUT_N = 1 << TC_LUT_BITS; // (the table's size there: UNP_LUT_BITS)
__device__ unsigned g_tc_lut[TC_LUT_N];
}
void vc2_upload_tables_transcode(const QuantTables &t, hipStream_t s) {
  (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(c_qt), &t, sizeof t, 0, hipMemcpyHostToDevice, s);
  (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_tc_lut), vc2_unpack_lut_host(), sizeof(unsigned) * TC_LUT_N, 0, hipMemcpyHostToDevice, s);
}

namespace {

// Quantisation.cpp:86-95
__device__ __forceinline__ int tc_scale_c(int v, int qf, int off) {
  const unsigned mag = v < 0 ? 0u - (unsigned)v : (unsigned)v;
  int a = (int)(mag * (unsigned)qf);
  if (a > 0) a = (int)((unsigned)a + (unsigned)off);
  a = (int)((unsigned)a + 2u);
  a /= 4;
  return v < 0 ? (int)(0u - (unsigned)a) : a;
}
// Quantisation.cpp:69-76: |v| << 2 divided by the factor, by its exact reciprocal inside the reference's domain
__device__ __forceinline__ int tc_quant_c(int v, int qf, unsigned mg, int sh) {
  const unsigned mag = v < 0 ? 0u - (unsigned)v : (unsigned)v;
  const int a = (int)(mag << 2);
  const unsigned t = __umulhi(mg, (unsigned)a);
  int q = (int)((t + (((unsigned)a - t) >> 1)) >> sh);
  // (outside that domain the literal division, under a wave-uniform test as quant_core of vc2hip_slices.hip has it)
  const bool slow = !(qf > 1 && a >= 0);
  if (__any(slow)) { if (slow) q = a / qf; }
  return v < 0 ? (int)(0u - (unsigned)q) : q;
}
__device__ __forceinline__ int tc_quant(int v, int aq) { return tc_quant_c(v, c_qt.qf[aq], c_qt.magic[aq], c_qt.shift[aq]); }

// The requantiser's constants of the subband a lane is in.  A component's coefficients come coarsest band first, so the
// band of coefficient j never falls as j grows: the constants are fetched once per band (3 * depth + 1 times a component),
// not once per coefficient, and the serial decode loop carries no dependent table load.
struct TcBand {
  int end = 0;    // first coefficient beyond the band
  int band = -1;
  int m = 0;      // the matrix entry
  int qf_in = 4, off_in = 1;             // scale() at the slice's own index
  __device__ __forceinline__ void seek(int j, int n0, const int *qmatrix, int qs) {
    if (j < end) return;
    while (j >= end && band < VC2_MAX_BANDS - 1) { ++band; end = band_offset(n0, band + 1); }
    m = qmatrix[band];
    const int ai = max(qs - m, 0);
    qf_in = c_qt.qf[ai]; off_in = c_qt.off[ai];
  }
};
// SignedVLC(v).numOfBits(), VLC.cpp:78-85
__device__ __forceinline__ int tc_bits(int v) {
  if (v == 0) return 1;
  const unsigned m = (v < 0 ? 0u - (unsigned)v : (unsigned)v) + 1u;
  return 2 * (31 - __clz(m)) + 2;
}
__device__ __forceinline__ unsigned tc_compact_even32(unsigned x) {
  x &= 0x55555555u;
  x = (x | (x >> 1)) & 0x33333333u;
  x = (x | (x >> 2)) & 0x0F0F0F0Fu;
  x = (x | (x >> 4)) & 0x00FF00FFu;
  x = (x | (x >> 8)) & 0x0000FFFFu;
  return x;
}
// Bounded bit reader over 64-bit big-endian words with one word of lookahead; bits past the bound read as 1
// (VLC.cpp:182-185).  A lane reads ITS OWN stream, so the 64 loads of a wavefront instruction go to 64 cache lines, and
// the streams of a CU's wavefronts do not fit its L1: with one 8-byte load per refill every 128-byte line of the payload
// can cross the L2 -> L1 path sixteen times.  So the stream is requested 64 bytes at a time (eight adjacent loads issued
// together: the first brings the line, the others meet it) into a queue of registers that a refill shifts down --
// Reader32's remedy in vc2hip_slices.hip.  (A request goes out when the queue is empty: the take behind it waits for
// the load.)  Loads are whole aligned 8-byte words of the slot, none without a data bit; what a word holds
// outside the component is masked.
struct TcReader {
  const uint2 *pw; // the next word to request
  int left;        // data bits from that word on (<= 0: none)
  unsigned long long acc, nxt;
  int have;
  uint2 b0, b1, b2, b3, b4, b5, b6, b7; // requested words, as they came
  int bn;          // how many of them are unread
  int bleft;       // `left` as it was for b0
  __device__ __forceinline__ void request() {
    bleft = left;
    if (left > 0) b0 = pw[0];
    if (left > 64) b1 = pw[1];
    if (left > 128) b2 = pw[2];
    if (left > 192) b3 = pw[3];
    if (left > 256) b4 = pw[4];
    if (left > 320) b5 = pw[5];
    if (left > 384) b6 = pw[6];
    if (left > 448) b7 = pw[7];
    pw += 8;
    left -= 512;
    bn = 8;
  }
  __device__ __forceinline__ unsigned long long take() {
    unsigned long long v = ~0ull;
    if (bleft > 0) {
      v = ((unsigned long long)__builtin_bswap32(b0.x) << 32) | __builtin_bswap32(b0.y);
      if (bleft < 64) v |= ~0ull >> bleft;
    }
    b0 = b1; b1 = b2; b2 = b3; b3 = b4; b4 = b5; b5 = b6; b6 = b7;
    bleft -= 64;
    if (--bn == 0) request();
    return v;
  }
  __device__ __forceinline__ void init(const uint8_t *data, int nbytes) {
    const size_t a = (size_t)data;
    const int lead = 8 * (int)(a & 7);
    pw = (const uint2 *)(a & ~(size_t)7);
    left = 8 * nbytes + lead;
    if (nbytes <= 0) left = 0; // an empty component reads no word at all
    b0 = b1 = b2 = b3 = b4 = b5 = b6 = b7 = make_uint2(0u, 0u);
    request();
    acc = take() << lead;
    have = 64 - lead;
    nxt = take();
  }
  __device__ __forceinline__ unsigned long long peek() const { return acc | ((nxt >> 1) >> (have - 1)); }
  __device__ __forceinline__ void skip(int n) { // 0 <= n <= 64
    if (n < have) { acc <<= n; have -= n; }
    else {
      const int r = n - have;
      acc = nxt << r;
      have = 64 - r;
      nxt = take();
    }
  }
};

// one component of one input slice, as the decoder's slice reader finds it
struct TcComp {
  const uint8_t *data;
  int len;    // bytes the reader may look at
  int q;      // the slice's index byte
  bool over;  // the component ran past the payload
};
__device__ __forceinline__ TcComp tc_open(const TranscodeParams &p, int pic, int slice, int comp) {
  const uint8_t *pay = p.in + (size_t)pic * p.in_stride;
  const unsigned long long plen = min(p.in_lens[pic], (unsigned long long)p.in_stride); // never past the picture's slot
  unsigned long long pos = (unsigned long long)p.in_offs[(size_t)pic * p.n_slices + slice] + p.prefix;
  auto rd = [&](unsigned long long a) -> unsigned { return a < plen ? pay[a] : 0u; };
  TcComp c;
  c.q = (int)rd(pos);
  pos += 1;
  for (int k = 0; k < comp; ++k) pos += 1 + (unsigned long long)rd(pos) * p.scalar;
  unsigned long long len = (unsigned long long)rd(pos) * p.scalar;
  pos += 1;
  c.over = pos + len > plen;
  if (c.over) len = pos < plen ? plen - pos : 0;
  c.len = (int)min(len, (unsigned long long)0x0FFFFFFF);
  c.data = pay + (pos < plen ? pos : 0);
  return c;
}

// The decoder's look-up table (vc2hip_slices.hip, vc2_unpack_lut_host): what the next 10 stream bits decode to -- bits
// [3:0] consumed, [7:4] coefficients (1..8, zeros included), [11:8] / [15:12] positions of up to two non-zero values,
// [23:16] / [31:24] the values (int8; none: both slots 0 at position 0, one: both slots hold it); 0: the first token is a
// code longer than the index.  Every workgroup copies it into LDS.
__device__ __forceinline__ void tc_lut_init(unsigned *lut) {
  for (int i = threadIdx.x * 4; i < TC_LUT_N; i += blockDim.x * 4) *(uint4 *)(lut + i) = *(const uint4 *)(g_tc_lut + i);
}

// One turn of a lane's decode: the coefficients the next bits of the window hold -- nc of them, all zero but those in the
// slots (position inside the turn, value; position -1: unused; positions ascend) -- and the bits to skip.  Up to TC_LOOKS
// look-ups while each is whole and fits the room; otherwise one token by arithmetic: a run of zeros ('1' bits, at most
// 32) and a code of up to 32 bits.  A code of more than 32 bits (outside the reference's domain) is left to tc_long, after
// the run before it has been skipped.  The turn has ONE skip, at the caller's: the refill code runs once a turn.
constexpr int TC_LOOKS = 3, TC_SLOTS = 2 * TC_LOOKS;
struct TcTurn {
  int nc, consume;
  int pos[TC_SLOTS], val[TC_SLOTS];
  bool longcode;
};
__device__ __forceinline__ void tc_turn(unsigned long long win, int room, const unsigned *lut, TcTurn &t) {
  t.nc = 0; t.consume = 0; t.longcode = false;
#pragma unroll
  for (int s = 0; s < TC_SLOTS; ++s) { t.pos[s] = -1; t.val[s] = 0; }
  unsigned e = lut[win >> (64 - TC_LUT_BITS)];
  if (e != 0u && (int)((e >> 4) & 15u) <= room) {
    bool go = true;
#pragma unroll
    for (int k = 0; k < TC_LOOKS; ++k) {
      if (k > 0) e = lut[(win << t.consume) >> (64 - TC_LUT_BITS)];
      const int nc = (int)((e >> 4) & 15u);
      go = go && e != 0u && nc <= room - t.nc;
      if (go) {
        const int a0 = (int)((e >> 8) & 15u), a1 = (int)((e >> 12) & 15u);
        t.pos[2 * k] = t.nc + a0;
        t.val[2 * k] = __builtin_amdgcn_sbfe((int)e, 16, 8);
        if (a1 != a0) { t.pos[2 * k + 1] = t.nc + a1; t.val[2 * k + 1] = __builtin_amdgcn_sbfe((int)e, 24, 8); }
        t.nc += nc;
        t.consume += (int)(e & 15u);
      }
    }
  } else {
    const int lz = ~win ? __clzll((long long)~win) : 64;
    const int z = min(min(lz, room), 32);
    t.nc = z; t.consume = z;
    if (z < room && z == lz) {
      const unsigned hi = (unsigned)((win << z) >> 32);
      const unsigned follow = hi & 0xAAAAAAAAu;
      if (follow == 0u) t.longcode = true;
      else {
        const int K = __clz((int)follow) >> 1; // 1 .. 15
        const unsigned body = hi >> (32 - 2 * K);
        const unsigned mag = ((1u << K) | tc_compact_even32(body)) - 1u;
        const int neg = (int)((hi >> (30 - 2 * K)) & 1u);
        t.pos[0] = z;
        t.val[0] = neg ? (int)(0u - mag) : (int)mag;
        t.nc = z + 1;
        t.consume = z + 2 * K + 2;
      }
    }
  }
}
// a code of more than 32 bits at the reader's position: bit by bit, wraps as the oracle does (VLC.cpp:283-317)
__device__ __forceinline__ int tc_long(TcReader &br) {
  unsigned value = 1;
  for (;;) {
    const int f = (int)(br.peek() >> 63);
    br.skip(1);
    if (f) break;
    value = (value << 1) | (unsigned)(br.peek() >> 63);
    br.skip(1);
  }
  value -= 1u;
  int v = 0;
  if (value) {
    v = (br.peek() >> 63) ? (int)(0u - value) : (int)value;
    br.skip(1);
  }
  return v;
}

constexpr int TC_SLICES = 64;           // slices of a workgroup; its three wavefronts take Y, U and V
constexpr int TC_THREADS = 3 * TC_SLICES;

// NC - 1: candidate indices measured per decode (16: the first round of the capped search, 8: its second)
template <int NC>
__global__ __launch_bounds__(TC_THREADS) void k_transcode_measure(const TranscodeParams p) {
  __shared__ unsigned long long acc[NC];
  __shared__ __attribute__((aligned(16))) unsigned lut[TC_LUT_N];
  const int lane = threadIdx.x & 63, comp = threadIdx.x >> 6;
  const int pic = blockIdx.y, slice = blockIdx.x * TC_SLICES + lane;
  const bool active = slice < p.n_slices;
  int t0, step, cnt;
  if (p.round == 0) { t0 = p.target; step = 8; cnt = (VC2_CAP_Q_TOP - t0) / 8 + 1; }
  else if (p.round == 1) {
    const unsigned long long *row = p.table + (size_t)pic * VC2_CAP_ROW;
    t0 = (int)row[VC2_CAP_BASE] + 1; step = 1; cnt = (int)row[VC2_CAP_COUNT];
  } else return;
  cnt = min(cnt, NC - 1);
  if (cnt <= 0) return; // (the same for the whole workgroup)
  tc_lut_init(lut);
  if (threadIdx.x < NC) acc[threadIdx.x] = 0;
  __syncthreads();
  const int n = p.comp_n[comp], n0 = p.comp_n0[comp];
  int gross[NC], count[NC], qo[NC];
  unsigned bad32 = 0, bad_scalar = 0;
  if (active) {
    const TcComp c = tc_open(p, pic, slice, comp);
    const int qs = c.q;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      gross[k] = count[k] = 0;
      qo[k] = max(qs, min(t0 + step * min(k, cnt - 1), VC2_CAP_Q_TOP));
    }
    const bool any_requant = qo[NC - 1] != qs; // (the candidates ascend)
    TcReader br;
    br.init(c.data, c.len);
    TcBand bd;
    int j = 0;
    // one value at coefficient `at`, `zeros` zero coefficients behind the value before it
    auto value = [&](int at, int zeros, int val) {
      int d = 0;
      if (any_requant) {
        bd.seek(at, n0, p.qmatrix, qs); // (qs < the candidate <= 115 here)
        d = tc_scale_c(val, bd.qf_in, bd.off_in);
      }
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        int v = val;
        if (qo[k] != qs) v = tc_quant(d, max(qo[k] - bd.m, 0));
        int nb = tc_bits(v);
        if (nb > 32) { bad32 |= 1u << k; v = 0; nb = 1; } // the slice writer refuses it (VLC.h:27); written as 0
        gross[k] += zeros + nb;
        if (v != 0) count[k] = gross[k];
      }
    };
    while (j < n) {
      TcTurn t;
      tc_turn(br.peek(), n - j, lut, t);
      br.skip(t.consume);
      int prev = -1;
#pragma unroll
      for (int s = 0; s < TC_SLOTS; ++s)
        if (t.pos[s] >= 0) { value(j + t.pos[s], t.pos[s] - prev - 1, t.val[s]); prev = t.pos[s]; }
#pragma unroll
      for (int k = 0; k < NC; ++k) gross[k] += t.nc - 1 - prev;
      j += t.nc;
      if (t.longcode) { value(j, 0, tc_long(br)); ++j; }
    }
  }
  unsigned units[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    units[k] = 0;
    if (active) {
      units[k] = (unsigned)((((count[k] + 7) >> 3) + p.scalar - 1) / p.scalar);
      if (units[k] > 255u) { bad_scalar |= 1u << k; units[k] = 255u; }
    }
  }
  if (active) {
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (k < cnt) atomicAdd(&acc[k], (unsigned long long)units[k] * p.scalar + (((bad32 | bad_scalar) >> k & 1u) ? VC2_CAP_NOFIT : 0ull));
  }
  __syncthreads();
  if ((int)threadIdx.x < cnt)
    atomicAdd(&p.table[(size_t)pic * VC2_CAP_ROW + (p.round ? VC2_CAP_R2 : 0) + threadIdx.x], acc[threadIdx.x]);
}

// One thread per picture.  Round 0: the first candidate floor + 8 k that fits brackets the answer (the lengths never
// grow with the index); round 1: the smallest of the up to seven indices in between that fits.
__global__ __launch_bounds__(64) void k_transcode_pick(const TranscodeParams p, int n_pictures) {
  const int pic = blockIdx.x * 64 + threadIdx.x;
  if (pic >= n_pictures) return;
  unsigned long long *row = p.table + (size_t)pic * VC2_CAP_ROW;
  const unsigned long long hdr = (unsigned long long)p.n_slices * ((unsigned long long)p.prefix + 4ull);
  if (p.round == 0) {
    const int floor_q = p.target, nvalid = (VC2_CAP_Q_TOP - floor_q) / 8 + 1; // 1 .. 15
    int fit = -1;
    for (int k = 0; k < nvalid; ++k)
      if (row[k] + hdr <= p.cap) { fit = k; break; }
    int base, count, otherwise;
    if (fit == 0) { base = floor_q; count = 0; otherwise = floor_q; }
    else if (fit > 0) { base = floor_q + 8 * (fit - 1); count = 7; otherwise = floor_q + 8 * fit; }
    else { base = floor_q + 8 * (nvalid - 1); count = min(7, VC2_CAP_Q_TOP - base); otherwise = VC2_CAP_Q_TOP; }
    row[VC2_CAP_BASE] = (unsigned long long)base;
    row[VC2_CAP_COUNT] = (unsigned long long)count;
    row[VC2_CAP_ELSE] = (unsigned long long)otherwise;
    p.qpic[pic] = otherwise;
  } else {
    const int base = (int)row[VC2_CAP_BASE], count = (int)row[VC2_CAP_COUNT];
    int q = (int)row[VC2_CAP_ELSE];
    for (int j = 0; j < count; ++j)
      if (row[VC2_CAP_R2 + j] + hdr <= p.cap) { q = base + 1 + j; break; }
    p.qpic[pic] = q;
  }
}

// The coefficient-parallel step between the decoder's slice reader and the encoder's slice coder.  The reader
// (vc2_launch_unpack) has left every slice's quantised coefficients in the store as slice records and its index in p.qs.
// A slice that ends at a coarser index has its coefficients DEQUANTISED in place, scale(c, q_s) per band: the slice coder,
// which quantises what it finds in the store with the index it is handed, then writes quant(scale(c, q_s), q').  A slice
// that keeps its index must keep its VALUES (no arithmetic: at indices whose factors wrap 32 bits quant(scale(c)) is not
// c), so its coefficients stay as they are and the coder is handed q_s - 256: every coder writes the header's index byte
// as index & 0xFF -- q_s -- and adjusts max(index - matrix, 0) -- 0, whose factor 4 makes quant() the identity.
// G coefficients a piece: 8 (16-bit store: 16 bytes, escapes through the wide array) or 1 (int32 store).  A workgroup takes
// TC_SC_U consecutive slices; a thread takes the same piece of each, so the band arithmetic is done once for the four
// and their loads are in flight together (one piece a thread, the kernel waited for memory three times in a row: the
// slice's index, the piece, the constants -- 4.1 ms per 128 UHD-1 pictures).
constexpr int TC_SC_U = 4;
template <class ST, int G>
__global__ __launch_bounds__(256) void k_transcode_scale(const TranscodeParams p) {
  const int pic = blockIdx.y, gps = p.slice_coefs / G, s0 = blockIdx.x * TC_SC_U;
  const int target = p.capped ? p.qpic[pic] : p.target;
  int qs[TC_SC_U];
  bool work[TC_SC_U];
#pragma unroll
  for (int u = 0; u < TC_SC_U; ++u) {
    const bool valid = s0 + u < p.n_slices;
    qs[u] = valid ? p.qs[(size_t)pic * p.n_slices + s0 + u] : 0;
    work[u] = valid && qs[u] < target; // (a kept slice: no arithmetic)
  }
  if (threadIdx.x < TC_SC_U && s0 + (int)threadIdx.x < p.n_slices) {
    const size_t sidx = (size_t)pic * p.n_slices + s0 + threadIdx.x;
    const int q = p.qs[sidx], qo = max(q, target);
    p.qpack[sidx] = qo == q ? q - 256 : qo;
    if (p.qidx_out) p.qidx_out[sidx] = qo;
    // An index the dequantiser refuses (Quantisation.cpp:61).  vc2hip_sync returns ONE code for everything on the context
    // since the last sync, and the composition's order is reader first: so the flag is not raised once the context's error
    // word holds VC2_DEVERR_STREAM (the index and the reader, which raise it, have finished).  The word is the context's,
    // not the picture's: another picture's broken chain suppresses it as well, which changes nothing sync can return.
    if (q - p.qm_min > 119 && !(__atomic_load_n(p.err, __ATOMIC_RELAXED) & VC2_DEVERR_STREAM)) atomicOr(p.err, VC2_DEVERR_QINDEX);
  }
  for (int g = threadIdx.x; g < gps; g += blockDim.x) {
    const int e0 = g * G;
    const int comp = e0 >= p.comp_off[2] ? 2 : e0 >= p.comp_off[1] ? 1 : 0; // (a piece lies in one component: the 16-bit store's rule)
    const int j0 = e0 - p.comp_off[comp], n0 = p.comp_n0[comp];
    int e[TC_SC_U][G];
    int any[TC_SC_U];
#pragma unroll
    for (int u = 0; u < TC_SC_U; ++u) {
      any[u] = 0;
      if (!work[u]) continue;
      const size_t at = (size_t)pic * p.store_stride + (size_t)(s0 + u) * p.slice_coefs + e0;
      if constexpr (G == 8) St<ST>::load8((const ST *)p.store + at, p.store_wide ? p.store_wide + at : nullptr, e[u]);
      else e[u][0] = (int)((const ST *)p.store)[at];
#pragma unroll
      for (int k = 0; k < G; ++k) any[u] |= e[u][k];
    }
    // (band_of_index without its division where the LL block is a power of two, as it nearly always is)
    const int n0s = n0 > 0 && (n0 & (n0 - 1)) == 0 ? 31 - __clz(n0) : -1;
    auto band_at = [&](int j) -> int {
      const int mm = n0s >= 0 ? j >> n0s : j / n0;
      if (mm == 0) return 0;
      const int L = (31 - __clz(mm)) / 2 + 1;
      return 3 * (L - 1) + (mm >> (2 * (L - 1)));
    };
    const int b_first = band_at(j0), b_last = band_at(j0 + G - 1);
    int mk[G];
#pragma unroll
    for (int k = 0; k < G; ++k) mk[k] = p.qmatrix[b_first == b_last ? b_first : band_at(j0 + k)];
#pragma unroll
    for (int u = 0; u < TC_SC_U; ++u) {
      // most coefficients of a coded picture are zero, and scale(0) is 0: a piece of zeros is left as it is
      if (!work[u] || any[u] == 0) continue;
      int aq = max(qs[u] - mk[0], 0); // (qs < the index the slice ends at <= 115 here)
      int qf = c_qt.qf[aq], off = c_qt.off[aq];
#pragma unroll
      for (int k = 0; k < G; ++k) {
        if (b_first != b_last) { aq = max(qs[u] - mk[k], 0); qf = c_qt.qf[aq]; off = c_qt.off[aq]; }
        e[u][k] = tc_scale_c(e[u][k], qf, off);
      }
      const size_t at = (size_t)pic * p.store_stride + (size_t)(s0 + u) * p.slice_coefs + e0;
      if constexpr (G == 8) St<ST>::store8((ST *)p.store + at, p.store_wide ? p.store_wide + at : nullptr, e[u]);
      else ((ST *)p.store)[at] = (ST)e[u][0];
    }
  }
}

// vc2hip_transcode_cbr_batch_dev: which slices fit their HQ_CBR budget as they are, and the others
// made ready for the search.  One wavefront per slice, TF_WAVES slices a workgroup, a lane takes every 64th piece of G
// coefficients (16 bytes: 8 of the 16-bit store, 4 of the int32 store; 1 where a record is not made of whole pieces).
// A record holds its components' coefficients in coded order, so per component
//   count = bits through the last non-zero value = sum over the non-zero values of (SignedVLC bits - 1) + its position + 1
// (a zero is one bit): a sum and a maximum, reduced over the lanes by shuffles -- no second look at the values, no atomics.
//   need = sum over Y, U, V of ceil(ceil(count / 8) / scalar) * scalar          (component_slice_bytes, Slices.cpp:97-119)
// A slice is KEPT iff every length byte is at most 255 and need <= budget - 4: its values stay as they are and the coder is
// handed q_s - 256 (k_transcode_scale's identity: header byte q_s, adjusted index 0).  Every other slice is dequantised in
// place, scale(c, q_s), from the pieces the lane still holds (TF_HOLD of them: slices of up to 64 * TF_HOLD * G coefficients
// are read once; what lies beyond is read again), and marked for the search (VC2_CBR_MARK).
constexpr int TF_WAVES = 4, TF_HOLD = 2;
__device__ __forceinline__ int tf_wave_sum(int v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ int tf_wave_max(int v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = max(v, __shfl_xor(v, m));
  return v;
}
template <class ST, int G>
__global__ __launch_bounds__(64 * TF_WAVES) void k_transcode_fit(const TranscodeParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pic = blockIdx.y, slice = blockIdx.x * TF_WAVES + wave;
  if (slice >= p.n_slices) return; // (no workgroup barrier below)
  const size_t sidx = (size_t)pic * p.n_slices + slice;
  const int qs = p.qs[sidx], gps = p.slice_coefs / G;
  const size_t rec = (size_t)pic * p.store_stride + (size_t)slice * p.slice_coefs;
  ST *const st = (ST *)p.store + rec;
  int32_t *const wide = p.store_wide ? p.store_wide + rec : nullptr;
  auto load = [&](int g, int (&e)[G]) {
    if constexpr (G == 8) St<ST>::load8(st + g * 8, wide ? wide + g * 8 : nullptr, e);
    else if constexpr (G == 4) St<ST>::load4(st + g * 4, wide ? wide + g * 4 : nullptr, e);
    else e[0] = St<ST>::load1(st + g, wide ? wide + g : nullptr);
  };
  auto comp_of = [&](int e0) -> int { return e0 >= p.comp_off[2] ? 2 : e0 >= p.comp_off[1] ? 1 : 0; }; // (a piece lies in one component)
  int d0 = 0, d1 = 0, d2 = 0, l0 = -1, l1 = -1, l2 = -1; // per component: sum of (bits - 1) over the non-zero values, the last one's position
  auto measure = [&](int g, const int (&e)[G]) {
    const int comp = comp_of(g * G), j0 = g * G - p.comp_off[comp], n = p.comp_n[comp];
    int d = 0, l = -1;
#pragma unroll
    for (int k = 0; k < G; ++k)
      if (e[k] != 0 && j0 + k < n) { d += tc_bits(e[k]) - 1; l = j0 + k; }
    d0 += comp == 0 ? d : 0; d1 += comp == 1 ? d : 0; d2 += comp == 2 ? d : 0;
    l0 = max(l0, comp == 0 ? l : -1); l1 = max(l1, comp == 1 ? l : -1); l2 = max(l2, comp == 2 ? l : -1);
  };
  int held[TF_HOLD][G];
#pragma unroll
  for (int h = 0; h < TF_HOLD; ++h) {
#pragma unroll
    for (int k = 0; k < G; ++k) held[h][k] = 0;
    const int g = lane + 64 * h;
    if (g < gps) { load(g, held[h]); measure(g, held[h]); }
  }
#pragma unroll 1 // (unrolled, the int32 instantiations took 207 registers for a loop that most geometries never enter)
  for (int g = lane + 64 * TF_HOLD; g < gps; g += 64) {
    int e[G];
    load(g, e);
    measure(g, e);
  }
  d0 = tf_wave_sum(d0); d1 = tf_wave_sum(d1); d2 = tf_wave_sum(d2);
  l0 = tf_wave_max(l0); l1 = tf_wave_max(l1); l2 = tf_wave_max(l2);
  const int sc = p.out_scalar;
  auto length_byte = [&](int d, int l) -> int { return (((l >= 0 ? d + l + 1 : 0) + 7) / 8 + sc - 1) / sc; };
  const int b0 = length_byte(d0, l0), b1 = length_byte(d1, l1), b2 = length_byte(d2, l2);
  const bool keep = max(b0, max(b1, b2)) <= 255 && (b0 + b1 + b2) * sc <= p.out_budgets[slice] - 4; // (the same in every lane)
  if (lane == 0) {
    p.qpack[sidx] = keep ? qs - 256 : VC2_CBR_MARK;
    // the dequantiser's refusal (Quantisation.cpp:61), behind the reader's as in k_transcode_scale; a kept slice meets no dequantiser
    if (!keep && qs - p.qm_min > 119 && !(__atomic_load_n(p.err, __ATOMIC_RELAXED) & VC2_DEVERR_STREAM)) atomicOr(p.err, VC2_DEVERR_QINDEX);
  }
  if (keep) return;
  auto dequantise = [&](int g, int (&e)[G]) {
    int any = 0;
#pragma unroll
    for (int k = 0; k < G; ++k) any |= e[k];
    if (any == 0) return; // scale(0) is 0, and most coefficients of a coded picture are zero
    const int comp = comp_of(g * G), j0 = g * G - p.comp_off[comp], n = p.comp_n[comp], n0 = p.comp_n0[comp];
    const int n0s = n0 > 0 && (n0 & (n0 - 1)) == 0 ? 31 - __clz(n0) : -1;
#pragma unroll
    for (int k = 0; k < G; ++k) {
      if (j0 + k >= n) continue; // (what a record holds between its components stays)
      const int mm = n0s >= 0 ? (j0 + k) >> n0s : (j0 + k) / n0;
      int band = 0;
      if (mm) { const int L = (31 - __clz(mm)) / 2 + 1; band = 3 * (L - 1) + (mm >> (2 * (L - 1))); }
      const int aq = min(max(qs - p.qmatrix[band], 0), 119); // (beyond 119: refused above; the tables end there)
      e[k] = tc_scale_c(e[k], c_qt.qf[aq], c_qt.off[aq]);
    }
    if constexpr (G == 8) St<ST>::store8(st + g * 8, wide ? wide + g * 8 : nullptr, e);
    else if constexpr (G == 4) St<ST>::store4(st + g * 4, wide ? wide + g * 4 : nullptr, e[0], e[1], e[2], e[3]);
    else St<ST>::store1(st + g, wide ? wide + g : nullptr, e[0]);
  };
#pragma unroll
  for (int h = 0; h < TF_HOLD; ++h) {
    const int g = lane + 64 * h;
    if (g < gps) dequantise(g, held[h]);
  }
#pragma unroll 1
  for (int g = lane + 64 * TF_HOLD; g < gps; g += 64) {
    int e[G];
    load(g, e);
    dequantise(g, e);
  }
}

// Behind the slice coder of vc2hip_transcode_cbr_batch_dev.  d_qidx: what the coder was handed, a kept slice's index put
// back (q_s - 256 is the only negative entry).  And the order of the refusals: the search and the CBR writer have by now
// worked on whatever a broken chain left in the store and may have refused it; the composition stops at its reader, and
// vc2hip_sync returns ONE code for everything on the context since the last sync -- so once the error word holds
// VC2_DEVERR_STREAM the coders' flags are taken out of it again.
__global__ __launch_bounds__(256) void k_transcode_settle(const TranscodeParams p, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (p.qidx_out && i < total) {
    const int q = p.qpack[i];
    p.qidx_out[i] = q < 0 ? q + 256 : q;
  }
  if (i == 0 && (__atomic_load_n(p.err, __ATOMIC_RELAXED) & VC2_DEVERR_STREAM))
    atomicAnd(p.err, ~(unsigned)(VC2_DEVERR_QINDEX | VC2_DEVERR_SCALAR | VC2_DEVERR_CBR_TOOBIG | VC2_DEVERR_CBR_LEN | VC2_DEVERR_CODE32));
}

} // namespace

void vc2_launch_transcode_fit(Launcher &L, const TranscodeParams &p, int n_pictures, hipStream_t s) {
  vc2_prof_begin(L, "transcode_fit", s);
  const dim3 grid((p.n_slices + TF_WAVES - 1) / TF_WAVES, n_pictures), block(64 * TF_WAVES);
  const bool quads = p.slice_coefs % 4 == 0 && p.store_stride % 4 == 0 && p.comp_off[1] % 4 == 0 && p.comp_off[2] % 4 == 0;
  if (p.store16) VC2_LAUNCH(L, (k_transcode_fit<int16_t, 8>), grid, block, 0, s, p);
  else if (quads) VC2_LAUNCH(L, (k_transcode_fit<int32_t, 4>), grid, block, 0, s, p);
  else VC2_LAUNCH(L, (k_transcode_fit<int32_t, 1>), grid, block, 0, s, p);
  vc2_prof_end(L, s);
}
void vc2_launch_transcode_settle(Launcher &L, const TranscodeParams &p, int n_pictures, hipStream_t s) {
  vc2_prof_begin(L, "transcode_settle", s);
  const int total = n_pictures * p.n_slices;
  VC2_LAUNCH(L, k_transcode_settle, dim3((total + 255) / 256), dim3(256), 0, s, p, total);
  vc2_prof_end(L, s);
}

void vc2_launch_transcode_measure(Launcher &L, const TranscodeParams &p, int n_pictures, hipStream_t s) {
  vc2_prof_begin(L, "transcode_measure", s);
  const dim3 grid((p.n_slices + TC_SLICES - 1) / TC_SLICES, n_pictures);
  if (p.round == 0) VC2_LAUNCH(L, k_transcode_measure<16>, grid, dim3(TC_THREADS), 0, s, p);
  else VC2_LAUNCH(L, k_transcode_measure<8>, grid, dim3(TC_THREADS), 0, s, p);
  vc2_prof_end(L, s);
}
void vc2_launch_transcode_pick(Launcher &L, const TranscodeParams &p, int n_pictures, hipStream_t s) {
  vc2_prof_begin(L, "transcode_pick", s);
  VC2_LAUNCH(L, k_transcode_pick, dim3((n_pictures + 63) / 64), dim3(64), 0, s, p, n_pictures);
  vc2_prof_end(L, s);
}
void vc2_launch_transcode_scale(Launcher &L, const TranscodeParams &p, int n_pictures, hipStream_t s) {
  vc2_prof_begin(L, "transcode_scale", s);
  const int gps = p.slice_coefs / (p.store16 ? 8 : 1);
  const int threads = std::min(256, std::max(64, (gps + 63) / 64 * 64));
  const dim3 grid((p.n_slices + TC_SC_U - 1) / TC_SC_U, n_pictures);
  if (p.store16) VC2_LAUNCH(L, (k_transcode_scale<int16_t, 8>), grid, dim3(threads), 0, s, p);
  else VC2_LAUNCH(L, (k_transcode_scale<int32_t, 1>), grid, dim3(threads), 0, s, p);
  vc2_prof_end(L, s);
}
