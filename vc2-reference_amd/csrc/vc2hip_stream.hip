// VC-2 streams in device memory (include/vc2hip.h, vc2hip_stream_write_dev / vc2hip_stream_read_dev): the picture data units
// around the fixed-stride payload slots of the batch calls, built and walked on the GPU.
//
//   write: k_stream_layout (one workgroup: unit offsets by a scan of the payload lengths, parse infos, picture headers, end of
//          sequence) -> k_stream_copy (pictures x chunks: every slot to its unit, realigned in registers)
//   read:  k_stream_walk (one wavefront: follows the parse-info chain, checks every picture's parameters, lists each picture's
//          payload segments) -> k_stream_gather (pictures x chunks: the segments into the slots, realigned in registers)
//
// Every stream offset is arbitrary, the slots are 16-byte aligned: the copies load and store whole aligned 16-byte words and
// move the bytes between them with alignbyte.  Nothing is written at or past the stream's cap or a slot's stride.
#include "vc2hip_internal.h"

void vc2_prof_begin(Launcher &L, const char *name, hipStream_t s);
void vc2_prof_end(Launcher &L, hipStream_t s);

#define VC2_SCAN_THREADS 256
#define VC2_COPY_THREADS 256
#define VC2_COPY_WORDS 4 // 16-byte words per thread and chunk
#define VC2_COPY_CHUNK (VC2_COPY_THREADS * VC2_COPY_WORDS)
#define VC2_WALK_WINDOW 128 // bytes of a unit the walk looks at: parse info + the longest header it accepts

// bytes [s, s + 16) of the 32 bytes lo:hi (s = 1 .. 15)
template <int Q> __device__ __forceinline__ uint4 vc2_funnel(const unsigned (&d)[8], unsigned m) {
  return make_uint4(__builtin_amdgcn_alignbyte(d[Q + 1], d[Q], m), __builtin_amdgcn_alignbyte(d[Q + 2], d[Q + 1], m),
                    __builtin_amdgcn_alignbyte(d[Q + 3], d[Q + 2], m), __builtin_amdgcn_alignbyte(d[Q + 4], d[Q + 3], m));
}
__device__ __forceinline__ uint4 vc2_realign(uint4 lo, uint4 hi, unsigned s) {
  const unsigned d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  switch (s >> 2) {
    case 0: return vc2_funnel<0>(d, s & 3);
    case 1: return vc2_funnel<1>(d, s & 3);
    case 2: return vc2_funnel<2>(d, s & 3);
    default: return vc2_funnel<3>(d, s & 3);
  }
}

// ------------------------------------------------------------------------------------------
// write
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long vc2_unit_bytes(const StreamWriteParams &p, int k) {
  const unsigned long long l = p.lens[k];
  return 13ull + (unsigned)p.hdr_len + (l < (unsigned long long)p.payload_stride ? l : (unsigned long long)p.payload_stride);
}
__device__ __forceinline__ void vc2_put(const StreamWriteParams &p, unsigned long long at, unsigned v) {
  if (at < p.cap) p.stream[at] = (uint8_t)v;
}
__device__ void vc2_put_parse_info(const StreamWriteParams &p, unsigned long long at, int code, unsigned long long next,
                                   unsigned long long prev) {
  const unsigned head[5] = {0x42, 0x42, 0x43, 0x44, (unsigned)code};
  for (int i = 0; i < 5; ++i) vc2_put(p, at + i, head[i]);
  for (int i = 0; i < 4; ++i) {
    vc2_put(p, at + 5 + i, (unsigned)(next >> (24 - 8 * i)));
    vc2_put(p, at + 9 + i, (unsigned)(prev >> (24 - 8 * i)));
  }
}

__global__ __launch_bounds__(VC2_SCAN_THREADS) void k_stream_layout(StreamWriteParams p) {
  __shared__ unsigned long long part[VC2_SCAN_THREADS];
  const int t = threadIdx.x;
  const int per = (p.n + VC2_SCAN_THREADS - 1) / VC2_SCAN_THREADS;
  const int k0 = min(p.n, t * per), k1 = min(p.n, k0 + per);
  bool over = false;
  unsigned long long sum = 0;
  for (int k = k0; k < k1; ++k) {
    sum += vc2_unit_bytes(p, k);
    over |= p.lens[k] > (unsigned long long)p.payload_stride;
  }
  part[t] = sum;
  __syncthreads();
  for (int off = 1; off < VC2_SCAN_THREADS; off <<= 1) {
    const unsigned long long v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned long long at = part[t] - sum;
  for (int k = k0; k < k1; ++k) {
    const unsigned long long u = vc2_unit_bytes(p, k);
    over |= u > 0xFFFFFFFFull; // (a next_parse_offset has 32 bits)
    p.unit_off[k] = at;
    vc2_put_parse_info(p, at, p.code, u, k ? vc2_unit_bytes(p, k - 1) : p.prev_parse_offset);
    const uint32_t pn = p.first_picture_number + (uint32_t)k;
    for (int i = 0; i < 4; ++i) vc2_put(p, at + 13 + i, pn >> (24 - 8 * i));
    for (int i = 4; i < p.hdr_len; ++i) vc2_put(p, at + 13 + i, p.hdr[i]);
    at += u;
  }
  if (t == 0) {
    const unsigned long long total = part[VC2_SCAN_THREADS - 1], end = total + (p.eos ? 13 : 0);
    if (p.eos) vc2_put_parse_info(p, total, 0x10, 0, vc2_unit_bytes(p, p.n - 1));
    *p.stream_len = end;
    over |= end > p.cap;
  }
  if (over) atomicOr(p.err, VC2_DEVERR_CAP);
}

// grid: pictures x chunks of VC2_COPY_CHUNK aligned 16-byte words of the stream
__global__ __launch_bounds__(VC2_COPY_THREADS) void k_stream_copy(StreamWriteParams p, int chunks) {
  const int k = blockIdx.x / chunks, chunk = blockIdx.x - k * chunks;
  const unsigned long long l = p.lens[k];
  const unsigned long long plen = l < (unsigned long long)p.payload_stride ? l : (unsigned long long)p.payload_stride;
  const unsigned long long dst0 = p.unit_off[k] + 13 + (unsigned)p.hdr_len;
  const unsigned long long end = dst0 + plen < p.cap ? dst0 + plen : p.cap;
  if (dst0 >= end) return;
  const unsigned long long b0 = dst0 >> 4, b1 = (end + 15) >> 4; // the stream's words [b0, b1)
  const unsigned r = (unsigned)(dst0 & 15);                     // slot byte i goes to stream byte dst0 + i
  const uint8_t *slot8 = p.payload + (long long)k * p.payload_stride;
  const uint4 *slot = (const uint4 *)slot8;
#pragma unroll
  for (int i = 0; i < VC2_COPY_WORDS; ++i) {
    const unsigned long long b = b0 + (unsigned long long)chunk * VC2_COPY_CHUNK + i * VC2_COPY_THREADS + threadIdx.x;
    if (b >= b1) break;
    const unsigned long long x0 = b << 4;
    if (x0 >= dst0 && x0 + 16 <= end) {
      const unsigned long long j = b - b0; // stream word b holds slot bytes [16 j - r, 16 j - r + 16): words j - 1 and j
      *(uint4 *)(p.stream + x0) = r ? vc2_realign(slot[j - 1], slot[j], 16 - r) : slot[j];
    } else { // the partial words at the ends of the payload or at cap
      for (int e = 0; e < 16; ++e) {
        const unsigned long long x = x0 + e;
        if (x >= dst0 && x < end) p.stream[x] = slot8[x - dst0];
      }
    }
  }
}

void vc2_launch_stream_layout(Launcher &L, const StreamWriteParams &p, hipStream_t s) {
  vc2_prof_begin(L, "stream_layout", s);
  VC2_LAUNCH(L, k_stream_layout, dim3(1), dim3(VC2_SCAN_THREADS), 0, s, p);
  vc2_prof_end(L, s);
}
void vc2_launch_stream_copy(Launcher &L, const StreamWriteParams &p, hipStream_t s) {
  // a payload of plen bytes touches at most plen / 16 + 2 words of the stream
  const int chunks = (int)(((unsigned long long)p.payload_stride / 16 + 2 + VC2_COPY_CHUNK - 1) / VC2_COPY_CHUNK);
  vc2_prof_begin(L, "stream_copy", s);
  VC2_LAUNCH(L, k_stream_copy, dim3((unsigned)(chunks * p.n)), dim3(VC2_COPY_THREADS), 0, s, p, chunks);
  vc2_prof_end(L, s);
}

// ------------------------------------------------------------------------------------------
// read
// ------------------------------------------------------------------------------------------
// MSB-first bit reader over the walk's window (DataUnit.cpp's BitReader): past `end` it flags and reads ones, which ends
// every exp-Golomb loop
struct Vc2Bits {
  const unsigned *w;
  int pos, end, bit;
  bool over;
  unsigned cur; // the byte at pos (one LDS load per byte, not per bit: the walk is a chain of dependent loads)
};
__device__ __forceinline__ unsigned vc2_bit(Vc2Bits &r) {
  if (r.bit == 0) {
    if (r.pos >= r.end) { r.over = true; return 1; }
    r.cur = r.w[r.pos];
  }
  const unsigned v = (r.cur >> (7 - r.bit)) & 1;
  if (++r.bit == 8) { r.bit = 0; ++r.pos; }
  return v;
}
// interleaved exp-Golomb (VLC.cpp:304-317)
__device__ uint32_t vc2_uvlc(Vc2Bits &r) {
  unsigned long long v = 1;
  for (int n = 0; !vc2_bit(r); ++n) {
    if (n == 32) { r.over = true; break; }
    v = (v << 1) | vc2_bit(r);
  }
  return (uint32_t)(v - 1);
}
__device__ __forceinline__ uint32_t vc2_be(const unsigned *w, int at, int n) {
  uint32_t v = 0;
  for (int i = 0; i < n; ++i) v = (v << 8) | w[at + i];
  return v;
}
// transform parameters (DataUnit.cpp:1340-1410) against what the caller said the pictures are: 0 or a VC2_SYN_* reason
__device__ int vc2_check_params(const StreamReadParams &p, Vc2Bits &r, int major, bool ld) {
  const uint32_t kernel = vc2_uvlc(r), depth = vc2_uvlc(r);
  bool asym = false;
  if (major >= 3) {
    if (vc2_bit(r)) asym |= vc2_uvlc(r) != kernel; // asym_transform_index_flag: wavelet_index_ho
    if (vc2_bit(r)) asym |= vc2_uvlc(r) != 0;      // asym_transform_flag: dwt_depth_ho
  }
  const uint32_t xs = vc2_uvlc(r), ys = vc2_uvlc(r), a = vc2_uvlc(r), b = vc2_uvlc(r);
  const bool custom_matrix = vc2_bit(r);
  if (r.bit) { r.bit = 0; ++r.pos; }
  if (r.over) return VC2_SYN_PAST_END;
  if (asym) return VC2_SYN_ASYMMETRIC;
  if (custom_matrix) return VC2_SYN_QUANT_MATRIX;
  if (ld != (p.ld != 0) || kernel != (uint32_t)p.kernel || depth != (uint32_t)p.depth || xs != (uint32_t)p.xs || ys != (uint32_t)p.ys)
    return VC2_SYN_PARAMS;
  if (!ld) return a == p.a && b == p.b ? 0 : VC2_SYN_PARAMS;
  return b && (unsigned long long)a * p.b == (unsigned long long)b * p.a ? 0 : VC2_SYN_PARAMS; // the same fraction
}

// one wavefront: every lane loads two bytes of the unit's window, then every lane parses it (the same bytes from LDS, so the
// walk's control flow and state are uniform); lane 0 stores the results.  One byte per LDS word: with a byte array the
// compiler merged the two byte loads of a big-endian field at an odd offset into one 16-bit LDS load at the even offset
// below it (the fragment's slice offset y at bytes 23-24 came from bytes 22-23), and every fragment after a picture's first
// was refused
__global__ __launch_bounds__(64) void k_stream_walk(StreamReadParams p) {
  __shared__ unsigned win[VC2_WALK_WINDOW];
  const bool lead = threadIdx.x == 0;
  const int ns = p.xs * p.ys;
  unsigned long long pos = 0, next = 0;
  int major = p.major_version, pics = 0, why = 0;
  bool open = false; // a fragmented picture is being read
  uint32_t fr_number = 0, dst = 0;
  int fr_slices = 0, nseg = 0;
  while (!why && pics < p.n) {
    __syncthreads(); // (the previous unit's window has been read)
    for (int i = threadIdx.x; i < VC2_WALK_WINDOW; i += 64) win[i] = pos + i < p.len ? p.stream[pos + i] : 0;
    __syncthreads();
    StreamSeg *seg = p.segs + (size_t)pics * p.seg_cap;
    bool done = false;
    next = 0;
    if (pos + 13 > p.len) { why = VC2_SYN_PAST_END; break; }
    if (win[0] != 0x42 || win[1] != 0x42 || win[2] != 0x43 || win[3] != 0x44) { why = VC2_SYN_PREFIX; break; }
    const int code = win[4];
    next = vc2_be(win, 5, 4);
    const int uend = next < VC2_WALK_WINDOW ? (int)next : VC2_WALK_WINDOW;
    const bool picture = code == 0xE8 || code == 0xC8, fragment = code == 0xEC || code == 0xCC;
    if (code != 0x00 && code != 0x10 && code != 0x20 && code != 0x30 && !picture && !fragment) why = VC2_SYN_CODE;
    else if (code == 0x10) why = VC2_SYN_FEWER; // end of sequence before n pictures
    else if (next == 0) why = VC2_SYN_NEXT_ZERO;
    else if (next < 13 || pos + next > p.len) why = VC2_SYN_PAST_END;
    else if (open && !fragment) why = VC2_SYN_FRAGMENT;
    else if ((picture || fragment) && major == 0) why = VC2_SYN_NO_VERSION;
    else if (code == 0x00) { // sequence header: its first field is the major version
      Vc2Bits r = {win, 13, uend, 0, false};
      major = (int)vc2_uvlc(r);
      if (r.over) why = VC2_SYN_PAST_END;
    } else if (picture) {
      Vc2Bits r = {win, 17, uend, 0, false};
      why = vc2_check_params(p, r, major, code == 0xC8);
      if (!why) {
        if (lead) seg[0] = StreamSeg{pos + (unsigned)r.pos, 0u, (uint32_t)(next - (unsigned)r.pos)};
        nseg = 1;
        dst = (uint32_t)(next - (unsigned)r.pos);
        fr_number = vc2_be(win, 13, 4);
        done = true;
      }
    } else if (fragment) {
      const uint32_t number = vc2_be(win, 13, 4), flen = vc2_be(win, 17, 2), count = vc2_be(win, 19, 2);
      if (next < 13 + 8) why = VC2_SYN_PAST_END;
      else if (count == 0) { // the parameters fragment opens the picture
        Vc2Bits r = {win, 21, uend, 0, false};
        why = open ? (int)VC2_SYN_FRAGMENT : vc2_check_params(p, r, major, code == 0xCC);
        open = !why;
        fr_number = number; fr_slices = 0; nseg = 0; dst = 0;
      } else if (!open || number != fr_number) why = VC2_SYN_FRAGMENT;
      else if (next < 13 + 12 || 12 + (unsigned long long)flen > next - 13) why = VC2_SYN_PAST_END;
      else if ((int)(vc2_be(win, 23, 2) * (uint32_t)p.xs + vc2_be(win, 21, 2)) != fr_slices || (int)count > ns - fr_slices)
        why = VC2_SYN_FRAGMENT; // slices continue the running count in raster order
      else {
        if (lead) seg[nseg] = StreamSeg{pos + 25, dst, flen};
        ++nseg;
        dst += flen;
        fr_slices += (int)count;
        done = fr_slices == ns;
        open = !done;
      }
    }
    if (why) break;
    if (done && lead) { // picture `pics` is complete: nseg segments, dst payload bytes
      const unsigned long long stride = (unsigned long long)p.payload_stride;
      p.meta[pics] = make_uint2((unsigned)nseg, dst < stride ? dst : (uint32_t)stride);
      p.lens[pics] = dst;
      if (p.picture_numbers) p.picture_numbers[pics] = fr_number;
      if (dst > stride) atomicOr(p.err, VC2_DEVERR_CAP);
    }
    pics += done;
    pos += next;
  }
  if (!lead) return;
  for (int k = pics; k < p.n; ++k) { p.meta[k] = make_uint2(0, 0); p.lens[k] = 0; }
  if (p.consumed) *p.consumed = pos;
  if (why) {
    *(unsigned long long *)((char *)p.err + VC2_ERRBLK_SYNTAX_AT) = pos;
    *(unsigned *)((char *)p.err + VC2_ERRBLK_SYNTAX_WHY) = (unsigned)why;
    __threadfence();
    atomicOr(p.err, VC2_DEVERR_SYNTAX);
  }
}

// grid: pictures x chunks of VC2_COPY_CHUNK 16-byte words of the slot
__global__ __launch_bounds__(VC2_COPY_THREADS) void k_stream_gather(StreamReadParams p, int chunks) {
  const int k = blockIdx.x / chunks, chunk = blockIdx.x - k * chunks;
  const uint2 m = p.meta[k];
  const int nseg = (int)m.x;
  const uint32_t plen = m.y; // (at most the stride, a multiple of 16)
  if (!nseg) return;
  const StreamSeg *sg = p.segs + (size_t)k * p.seg_cap;
  uint4 *slot = (uint4 *)(p.payload + (long long)k * p.payload_stride);
  const uint32_t words = (plen + 15) >> 4;
#pragma unroll
  for (int i = 0; i < VC2_COPY_WORDS; ++i) {
    const uint32_t j = (uint32_t)chunk * VC2_COPY_CHUNK + i * VC2_COPY_THREADS + threadIdx.x;
    if (j >= words) break;
    const uint32_t x0 = j << 4;
    int lo = 0, hi = nseg - 1; // the last segment that starts at or before x0 (the segments tile [0, plen) in order)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sg[mid].dst <= x0) lo = mid; else hi = mid - 1;
    }
    const StreamSeg g = sg[lo];
    if ((unsigned long long)x0 + 16 <= (unsigned long long)g.dst + g.len) {
      // the whole word from one segment: the two aligned stream words that hold its bytes (each holds at least one byte of
      // the segment, so neither reaches a page the stream does not touch)
      const size_t a = (size_t)(p.stream + g.src + (x0 - g.dst));
      const unsigned r = (unsigned)(a & 15);
      const uint4 *w = (const uint4 *)(a - r);
      slot[j] = r ? vc2_realign(w[0], w[1], r) : w[0];
    } else { // a word across segments, or the payload's last word (zeros behind plen)
      unsigned long long v[2] = {0, 0};
      int si = lo;
      for (int e = 0; e < 16; ++e) {
        const uint32_t x = x0 + e;
        if (x >= plen) break;
        while (si + 1 < nseg && x >= sg[si].dst + sg[si].len) ++si;
        if (x >= sg[si].dst + sg[si].len) break;
        const unsigned long long byte = p.stream[sg[si].src + (x - sg[si].dst)];
        if (e < 8) v[0] |= byte << (8 * e); else v[1] |= byte << (8 * (e - 8));
      }
      slot[j] = make_uint4((unsigned)v[0], (unsigned)(v[0] >> 32), (unsigned)v[1], (unsigned)(v[1] >> 32));
    }
  }
}

void vc2_launch_stream_walk(Launcher &L, const StreamReadParams &p, hipStream_t s) {
  vc2_prof_begin(L, "stream_walk", s);
  VC2_LAUNCH(L, k_stream_walk, dim3(1), dim3(64), 0, s, p);
  vc2_prof_end(L, s);
}
void vc2_launch_stream_gather(Launcher &L, const StreamReadParams &p, hipStream_t s) {
  const int chunks = (int)(((unsigned long long)p.payload_stride / 16 + VC2_COPY_CHUNK - 1) / VC2_COPY_CHUNK);
  vc2_prof_begin(L, "stream_gather", s);
  VC2_LAUNCH(L, k_stream_gather, dim3((unsigned)(chunks * p.n)), dim3(VC2_COPY_THREADS), 0, s, p, chunks);
  vc2_prof_end(L, s);
}
