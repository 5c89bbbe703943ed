// The decoded picture and its squared error without a payload (vc2hip_encode_recon_batch_dev).
//
// Entropy coding is lossless: what the decoder will show follows from the quantised coefficients alone.  After the
// forward transform (and the index search) the encoder's store still holds the transform coefficients -- the slice coders
// read it as const and quantise on the fly -- so
//   k_requantise     quant (Quantisation.cpp:69-76) of every coefficient with its slice's index and its band's matrix entry,
//                    written where the decoder's inverse level kernels look for quantised values (slice records, band
//                    planes, record heads); without a payload it also makes the slice coder's checks
//   k_ld_check       LD without a payload: the checks of the slice writer on the store vc2_launch_ld_quantise left
//   k_squared_error  sum of (a - b)^2 over the samples of two raw buffers, per picture and component
#include "vc2hip_internal.h"
#include "vc2hip_store.h"

void vc2_prof_begin(Launcher &L, const char *name, hipStream_t s);
void vc2_prof_end(Launcher &L, hipStream_t s);

__constant__ QuantTables c_rq;
void vc2_upload_tables_recon(const QuantTables &t, hipStream_t s) {
  (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(c_rq), &t, sizeof t, 0, hipMemcpyHostToDevice, s);
}

namespace {
// Quantisation.cpp:69-76, as quant_core of vc2hip_slices.hip: exact reciprocal multiply inside the reference's domain, the
// literal int division outside it (factor <= 1: index 0 and the wrapped factors of 116 - 119; |v| << 2 beyond int)
__device__ __forceinline__ int rq_quant(int v, int qf, unsigned mg, int sh) {
  const unsigned mag = v < 0 ? 0u - (unsigned)v : (unsigned)v;
  const int a = (int)(mag << 2);
  const unsigned t = __umulhi(mg, (unsigned)a);
  int q = (int)((t + (((unsigned)a - t) >> 1)) >> sh);
  const bool slow = !(qf > 1 && a >= 0);
  if (__any(slow)) { if (slow) q = a / qf; }
  return v < 0 ? (int)(0u - (unsigned)q) : q;
}
__device__ __forceinline__ int rq_band(int j, int n0, int n0_shift) {
  const int m = n0_shift >= 0 ? (j >> n0_shift) : (j / n0);
  if (m == 0) return 0;
  const int L = (31 - __clz(m)) / 2 + 1;
  return 3 * (L - 1) + (m >> (2 * (L - 1)));
}
// SignedVLC(v).numOfBits(), VLC.cpp:78-85
__device__ __forceinline__ int rq_bits(int v) {
  if (v == 0) return 1;
  const unsigned m = (v < 0 ? 0u - (unsigned)v : (unsigned)v) + 1u;
  return 2 * (31 - __clz(m)) + 2;
}
// element offset, from the picture's store, of coefficient j (a multiple of 8) of component comp of slice (sy, sx) in the
// decoder's band planes; lw: log2 of a block row (band_plane_at of vc2hip_slices.hip)
__device__ __forceinline__ long long rq_plane_at(const BandPlanes &bp, int comp, int n, int j, int sy, int sx, int &lw, int &ow) {
  int l = 0, start = n - (3 << (bp.lbsh[comp][0] + bp.lbsw[comp][0]));
  while (j < start) { ++l; start -= 3 << (bp.lbsh[comp][l] + bp.lbsw[comp][l]); }
  const int lh = bp.lbsh[comp][l], e = j - start;
  lw = bp.lbsw[comp][l]; ow = bp.ow[comp][l];
  const int b = e >> (lh + lw), rem = e & ((1 << (lh + lw)) - 1), r = rem >> lw, c = rem & ((1 << lw) - 1);
  return bp.base[comp][l] + (long long)(b * bp.np[comp][l] + (sy << lh) + r) * ow + (sx << lw) + c;
}

#define VC2_RQ_GROUPS 8 // slice groups a wavefront walks

// Lanes on consecutive pieces (16 bytes: eight 16-bit or four int32 coefficients) of a slice record; 2^grp_log2 lanes share a
// record, a wavefront holds 64 >> grp_log2 neighbouring records (they lie back to back in the encoder's store: the loads
// of a wavefront are one contiguous run).  A piece never straddles a component, a band plane's row pair or a record head
// (use_store16 and the planning of the band planes and heads keep all of them multiples of eight coefficients).
template <class ST, bool CHECK>
__global__ __launch_bounds__(256) void k_requantise(const RequantParams p) {
  constexpr int E = St<ST>::narrow ? 8 : 4;
  // The tables every piece consults -- quantiser constants by index, the matrix, the band planes' geometry -- in LDS: from
  // constant memory and the kernel arguments they are vector loads at lane-dependent addresses, four of them in a chain
  // before the first multiply (measured: 2.8 ms per 64 UHD pictures with fully coalesced loads and stores, latency-bound)
  __shared__ int s_qf[120], s_sh[120], s_qm[VC2_MAX_BANDS];
  __shared__ unsigned s_mg[120];
  __shared__ BandPlanes s_bp;
  __shared__ HeadSplit s_hs;
  for (int i = threadIdx.x; i < 120; i += 256) { s_qf[i] = c_rq.qf[i]; s_sh[i] = c_rq.shift[i]; s_mg[i] = c_rq.magic[i]; }
  if (threadIdx.x < VC2_MAX_BANDS) s_qm[threadIdx.x] = p.qmatrix[threadIdx.x];
  for (int i = threadIdx.x; i < (int)(sizeof(BandPlanes) / 4); i += 256) ((int *)&s_bp)[i] = ((const int *)&p.bp)[i];
  for (int i = threadIdx.x; i < (int)(sizeof(HeadSplit) / 4); i += 256) ((int *)&s_hs)[i] = ((const int *)&p.hs)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, pic = blockIdx.y;
  const int off1 = p.comp_off[1], off2 = p.comp_off[2], n_1 = p.comp_n[1], n_2 = p.comp_n[2];
  const int G = 1 << p.grp_log2, sub = lane & (G - 1), spw = 64 >> p.grp_log2;
  const int pieces = p.slice_coefs / E;
  const ST *__restrict__ src = (const ST *)p.src + (size_t)pic * p.src_stride;
  const int32_t *srcw = St<ST>::narrow ? p.src_wide + (size_t)pic * p.src_stride : nullptr;
  ST *__restrict__ dst = p.dst ? (ST *)p.dst + (size_t)pic * p.dst_stride : nullptr;
  int32_t *dstw = St<ST>::narrow && p.dst ? p.dst_wide + (size_t)pic * p.dst_stride : nullptr;
  for (int it = 0; it < VC2_RQ_GROUPS; ++it) {
    const int slice = ((blockIdx.x * 4 + wave) * VC2_RQ_GROUPS + it) * spw + (lane >> p.grp_log2);
    if (__builtin_amdgcn_readfirstlane(slice) >= p.n_slices) break;
    const bool active = slice < p.n_slices;
    const int q = active ? p.qidx[(size_t)pic * p.n_slices + slice] : 0;
    const int sy = slice / p.xs, sx = slice - sy * p.xs;
    int sum[3] = {0, 0, 0}, last[3] = {0, 0, 0}; // CHECK: code bits of all coefficients; 1 + index of the last non-zero one
    // one piece: quantise, (measure,) store
    auto piece = [&](const int pc, const uint4 raw) __attribute__((always_inline)) {
      const int jr = pc * E;
      const int comp = jr >= off2 && n_2 ? 2 : (jr >= off1 && n_1 ? 1 : 0);
      const int j = jr - (comp == 2 ? off2 : comp == 1 ? off1 : 0), n = comp == 2 ? n_2 : comp == 1 ? n_1 : p.comp_n[0];
      const int n0 = comp == 2 ? p.comp_n0[2] : comp == 1 ? p.comp_n0[1] : p.comp_n0[0];
      const int n0s = (n0 & (n0 - 1)) == 0 ? 31 - __clz(n0) : -1;
      const size_t rec = (size_t)slice * p.slice_coefs + jr;
      int e[E];
      if constexpr (E == 8) St<ST>::unpack8(raw, srcw + rec, e);
      else { e[0] = (int)raw.x; e[1] = (int)raw.y; e[2] = (int)raw.z; e[3] = (int)raw.w; }
      const int b0 = rq_band(j, n0, n0s), b1 = rq_band(j + E - 1, n0, n0s);
      if (b0 == b1) { // (a piece inside one band: every geometry whose LL block has a multiple of E coefficients, and most others)
        const int aq = max(q - s_qm[b0], 0);
        if (aq > 119) {
          atomicOr(p.err, VC2_DEVERR_QINDEX); // (and the coefficients count as zero, as in the slice coders)
#pragma unroll
          for (int k = 0; k < E; ++k) e[k] = 0;
        } else {
          const int qf = s_qf[aq], sh = s_sh[aq];
          const unsigned mg = s_mg[aq];
#pragma unroll
          for (int k = 0; k < E; ++k) e[k] = rq_quant(e[k], qf, mg, sh);
        }
      } else {
#pragma unroll
        for (int k = 0; k < E; ++k) {
          const int aq = max(q - s_qm[rq_band(j + k, n0, n0s)], 0);
          if (aq > 119) { atomicOr(p.err, VC2_DEVERR_QINDEX); e[k] = 0; }
          else e[k] = rq_quant(e[k], s_qf[aq], s_mg[aq], s_sh[aq]);
        }
      }
      if constexpr (CHECK) {
        int s = 0, l = 0;
#pragma unroll
        for (int k = 0; k < E; ++k) {
          const int nb = rq_bits(e[k]);
          if (nb > 32) atomicOr(p.err, VC2_DEVERR_CODE32); // VLC.h:27; measured it has its length (component_bits)
          s += nb;
          if (e[k] != 0) l = j + k + 1;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) if (comp == c) { sum[c] += s; last[c] = max(last[c], l); }
      }
      if (!dst) return;
      if constexpr (St<ST>::narrow) {
        if (j >= s_bp.from[comp]) {
          int lw, ow;
          const long long at = rq_plane_at(s_bp, comp, n, j, sy, sx, lw, ow);
          if (lw >= 3) St<ST>::store8(dst + at, dstw + at, e);
          else { // two block rows of four
            St<ST>::store4(dst + at, dstw + at, e[0], e[1], e[2], e[3]);
            St<ST>::store4(dst + at + ow, dstw + at + ow, e[4], e[5], e[6], e[7]);
          }
        } else {
          const long long at = j < s_hs.n[comp] ? s_hs.base[comp] + (long long)slice * s_hs.n[comp] + j : (long long)rec;
          St<ST>::store8(dst + at, dstw + at, e);
        }
      } else {
        St<ST>::store4(dst + rec, nullptr, e[0], e[1], e[2], e[3]);
      }
    };
    // (two pieces per lane in flight, both loads before the first multiply, changed nothing: 4.16 against 4.04 ms per 128
    // UHD pictures -- the kernel is not waiting for its loads)
    for (int pc0 = 0; pc0 < pieces; pc0 += G) {
      const int pc = pc0 + sub;
      if (active && pc < pieces) piece(pc, *(const uint4 *)(src + (size_t)slice * p.slice_coefs + pc * E));
    }
    if constexpr (CHECK) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        for (int d = 1; d < G; d <<= 1) {
          sum[c] += __shfl_xor(sum[c], d);
          last[c] = max(last[c], __shfl_xor(last[c], d));
        }
      if (active && sub == 0) { // component_slice_bytes' count: the bits up to and including the last non-zero coefficient
        int bytes[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int count = last[c] ? sum[c] - (p.comp_n[c] - last[c]) : 0; // (every zero behind it is one bit)
          int len = (((count + 7) >> 3) + p.scalar - 1) / p.scalar;
          if (len > 255) { atomicOr(p.err, VC2_DEVERR_SCALAR); len = 255; }
          bytes[c] = len * p.scalar;
        }
        if (p.cbr_bytes) { // Slices.cpp:352-368: V absorbs the remainder of the slice
          const int vb = p.cbr_bytes[slice] - 4 - bytes[0] - bytes[1];
          if (vb < bytes[2]) atomicOr(p.err, VC2_DEVERR_CBR_TOOBIG);
          else if (vb / p.scalar > 255) atomicOr(p.err, VC2_DEVERR_CBR_LEN);
        }
      }
    }
  }
}

// One wavefront per slice: the bits of the luma stream and of the interleaved chroma stream up to their last non-zero
// values, and the slice writer's test on them (k_ld_pack: Slices.cpp:195-244)
__device__ __forceinline__ int rq_intlog2(int value) { int l = 0; --value; while (value > 0) { value >>= 1; ++l; } return l; }
__global__ __launch_bounds__(256) void k_ld_check(const LdEncParams p) {
  const int lane = threadIdx.x & 63, slice = blockIdx.x * 4 + (threadIdx.x >> 6), pic = blockIdx.y;
  if (slice >= p.n_slices) return;
  const int32_t *rec = p.store + (size_t)pic * p.store_stride + (size_t)slice * p.slice_coefs;
  int sum[2] = {0, 0}, last[2] = {0, 0};
  auto take = [&](int s, int v, int pos) {
    const int nb = rq_bits(v);
    if (nb > 32) atomicOr(p.err, VC2_DEVERR_CODE32);
    sum[s] += nb;
    if (v != 0) last[s] = max(last[s], pos + 1);
  };
  for (int j = lane; j < p.comp_n[0]; j += 64) take(0, rec[p.comp_off[0] + j], j);
  for (int j = lane; j < p.comp_n[1]; j += 64) { // U and V alternate
    take(1, rec[p.comp_off[1] + j], 2 * j);
    take(1, rec[p.comp_off[2] + j], 2 * j + 1);
  }
#pragma unroll
  for (int s = 0; s < 2; ++s)
    for (int d = 1; d < 64; d <<= 1) {
      sum[s] += __shfl_xor(sum[s], d);
      last[s] = max(last[s], __shfl_xor(last[s], d));
    }
  const int ybits = last[0] ? sum[0] - (p.comp_n[0] - last[0]) : 0;
  const int cbits = last[1] ? sum[1] - (2 * p.comp_n[1] - last[1]) : 0;
  const int size = p.slice_bytes[slice];
  const int uvbits = 8 * size - 7 - rq_intlog2(8 * size - 7) - ybits;
  if (uvbits < cbits && lane == 0) atomicOr(p.err, VC2_DEVERR_LD_TOOBIG);
}

// ------------------------------------------------------------------------------------------
// squared error
// ------------------------------------------------------------------------------------------
typedef unsigned long long u64;
__device__ __forceinline__ u64 sq(unsigned a, unsigned b) {
  const unsigned d = a > b ? a - b : b - a;
  return (u64)d * d;
}
// the samples of one dword of each buffer (words of WB bytes in the layout's byte order, sample = (word >> shift) & mask)
template <int WB> __device__ __forceinline__ u64 sq_dword(unsigned x, unsigned y, int shift, unsigned mask, int le) {
  if constexpr (WB == 4) {
    const unsigned a = le ? x : __builtin_bswap32(x), b = le ? y : __builtin_bswap32(y);
    return sq((a >> shift) & mask, (b >> shift) & mask);
  } else if constexpr (WB == 2) { // (which word of the dword comes first does not matter to a sum)
    const unsigned a = le ? x : __builtin_bswap32(x), b = le ? y : __builtin_bswap32(y);
    return sq(((a >> 16) >> shift) & mask, ((b >> 16) >> shift) & mask) + sq(((a & 0xFFFFu) >> shift) & mask, ((b & 0xFFFFu) >> shift) & mask);
  } else {
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) s += sq((((x >> k) & 0xFFu) >> shift) & mask, (((y >> k) & 0xFFu) >> shift) & mask);
    return s;
  }
}
__device__ __forceinline__ u64 sq_sample(const uint8_t *a, const uint8_t *b, int wb, int shift, unsigned mask, int le) {
  return sq((vc2_load_word(a, wb, le) >> shift) & mask, (vc2_load_word(b, wb, le) >> shift) & mask);
}
// grid (blocks, pictures, 3).  The two buffers start on 16-byte boundaries and a component lies at the same offset in both,
// so its whole 16-byte pieces are the same in both: lanes on consecutive pieces, the words before the first and behind the
// last whole piece one by one.  WB == 0: word by word throughout (three-byte words, which no 16-byte piece holds whole).
// A component is rows[comp] rows of row_bytes[comp] bytes, pitch[comp] apart (SseParams): one row for tight rows, else rows
// that as a rule each start on a 16-byte boundary -- whole pieces first, over all rows, then the words behind each row's last piece.
template <int WB>
__global__ __launch_bounds__(256) void k_squared_error(const SseParams p) {
  __shared__ u64 part[4];
  const int pic = blockIdx.y, comp = blockIdx.z;
  const long long at = (long long)pic * p.pic_bytes + p.comp_at[comp], end = at + p.row_bytes[comp];
  const int rows = p.rows[comp];
  u64 acc = 0;
  if (rows > 1) {
    const long long pitch = p.pitch[comp];
    const int ppr = WB && !((at | pitch) & 15) ? (int)(p.row_bytes[comp] >> 4) : 0;        // whole pieces of a row (a packed picture stride
                                                                                          // may leave a picture's rows off the boundary: words then)
    const int wpr = (int)((p.row_bytes[comp] - 16ll * ppr) / p.word_bytes);              // words behind them
    if constexpr (WB != 0)
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (long long)rows * ppr; i += (long long)gridDim.x * 256) {
      const int r = (int)(i / ppr), j = (int)(i - (long long)r * ppr);
      const long long o = at + r * pitch + 16ll * j;
      const uint4 x = *(const uint4 *)(p.a + o), y = *(const uint4 *)(p.b + o);
      acc += sq_dword<WB>(x.x, y.x, p.shift, p.mask, p.le) + sq_dword<WB>(x.y, y.y, p.shift, p.mask, p.le) +
             sq_dword<WB>(x.z, y.z, p.shift, p.mask, p.le) + sq_dword<WB>(x.w, y.w, p.shift, p.mask, p.le);
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (long long)rows * wpr; i += (long long)gridDim.x * 256) {
      const int r = (int)(i / wpr), j = (int)(i - (long long)r * wpr);
      const long long o = at + r * pitch + 16ll * ppr + (long long)j * p.word_bytes;
      acc += sq_sample(p.a + o, p.b + o, p.word_bytes, p.shift, p.mask, p.le);
    }
  } else if (const long long first = (at + 15) & ~15ll, stop = end & ~15ll; WB != 0 && first <= stop) {
    const long long pieces = (stop - first) >> 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pieces; i += (long long)gridDim.x * 256) {
      const uint4 x = *(const uint4 *)(p.a + first + 16 * i), y = *(const uint4 *)(p.b + first + 16 * i);
      acc += sq_dword<WB>(x.x, y.x, p.shift, p.mask, p.le) + sq_dword<WB>(x.y, y.y, p.shift, p.mask, p.le) +
             sq_dword<WB>(x.z, y.z, p.shift, p.mask, p.le) + sq_dword<WB>(x.w, y.w, p.shift, p.mask, p.le);
    }
    if (blockIdx.x == 0) {
      const int head = (int)(first - at) / (WB ? WB : 1), tail = (int)(end - stop) / (WB ? WB : 1);
      for (int i = threadIdx.x; i < head + tail; i += 256) {
        const long long o = i < head ? at + (long long)i * WB : stop + (long long)(i - head) * WB;
        acc += sq_sample(p.a + o, p.b + o, WB, p.shift, p.mask, p.le);
      }
    }
  } else {
    const long long words = p.row_bytes[comp] / p.word_bytes;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < words; i += (long long)gridDim.x * 256)
      acc += sq_sample(p.a + at + i * p.word_bytes, p.b + at + i * p.word_bytes, p.word_bytes, p.shift, p.mask, p.le);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const u64 s = part[0] + part[1] + part[2] + part[3];
    if (s) atomicAdd(p.sse + 3 * (size_t)pic + comp, s); // (integers: the order of the adds cannot change the sum)
  }
}
} // namespace

void vc2_launch_requantise(Launcher &L, const RequantParams &p0, int n_pictures, hipStream_t s) {
  RequantParams p = p0;
  if (!p.bp.levels) for (int c = 0; c < 3; ++c) p.bp.from[c] = 1 << 30; // everything in the slice records (and heads)
  if (p.xs < 1) p.xs = 1;
  const int pieces = p.slice_coefs / (p.store16 ? 8 : 4);
  p.grp_log2 = 3;
  while (p.grp_log2 < 6 && (1 << p.grp_log2) < pieces) ++p.grp_log2;
  const int per_block = 4 * VC2_RQ_GROUPS * (64 >> p.grp_log2);
  const dim3 grid((unsigned)((p.n_slices + per_block - 1) / per_block), (unsigned)n_pictures);
  vc2_prof_begin(L, "requantise", s);
  if (p.store16) {
    if (p.check) VC2_LAUNCH(L, (k_requantise<int16_t, true>), grid, dim3(256), 0, s, p);
    else VC2_LAUNCH(L, (k_requantise<int16_t, false>), grid, dim3(256), 0, s, p);
  } else {
    if (p.check) VC2_LAUNCH(L, (k_requantise<int32_t, true>), grid, dim3(256), 0, s, p);
    else VC2_LAUNCH(L, (k_requantise<int32_t, false>), grid, dim3(256), 0, s, p);
  }
  vc2_prof_end(L, s);
}

void vc2_launch_ld_check(Launcher &L, const LdEncParams &p, int n_pictures, hipStream_t s) {
  vc2_prof_begin(L, "ld_check", s);
  VC2_LAUNCH(L, k_ld_check, dim3((unsigned)((p.n_slices + 3) / 4), (unsigned)n_pictures), dim3(256), 0, s, p);
  vc2_prof_end(L, s);
}

void vc2_launch_squared_error(Launcher &L, const SseParams &p, int n_pictures, hipStream_t s) {
  // enough workgroups per component to fill the GPU with a few pictures, few enough that a workgroup's one atomic is noise
  long long most = 0;
  for (int c = 0; c < 3; ++c) most = p.rows[c] * p.row_bytes[c] > most ? p.rows[c] * p.row_bytes[c] : most;
  long long bx = most / (16 * 256 * 8);
  bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);
  const dim3 grid((unsigned)bx, (unsigned)n_pictures, 3);
  vc2_prof_begin(L, "squared_error", s);
  switch (p.word_bytes) {
    case 1: VC2_LAUNCH(L, k_squared_error<1>, grid, dim3(256), 0, s, p); break;
    case 2: VC2_LAUNCH(L, k_squared_error<2>, grid, dim3(256), 0, s, p); break;
    case 4: VC2_LAUNCH(L, k_squared_error<4>, grid, dim3(256), 0, s, p); break;
    default: VC2_LAUNCH(L, k_squared_error<0>, grid, dim3(256), 0, s, p); break;
  }
  vc2_prof_end(L, s);
}
