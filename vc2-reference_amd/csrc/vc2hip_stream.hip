// VC-2 streams in device memory (include/vc2hip.h, vc2hip_stream_write_dev / vc2hip_stream_read_dev): the picture data units
// around the fixed-stride payload slots of the batch calls, built and walked on the GPU.
//
//   write: k_stream_layout (one workgroup: unit offsets by a scan of the payload lengths, parse infos, picture headers, end of
//          sequence) -> k_stream_copy (pictures x chunks: every slot to its unit, realigned in registers)
//   write, fragmented: the decoder's slice index (HQ; LD takes the budget table) -> k_frag_cut (a workgroup per picture: the
//          greedy cut by binary search and pointer jumping) -> k_frag_layout + k_frag_headers (scan over pictures, parse infos
//          and fragment headers) -> k_frag_copy (pictures x chunks of the stream: every fragment's slices, realigned in registers)
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
// Bytes of a unit the walk looks at: parse info + the longest header it accepts.  That is a parameters fragment with a
// matrix: 13 bytes of parse info, 8 of fragment header (picture number, data length, slice count), then in bits: wavelet 5
// (0 .. 6), depth 7 (a matrix comes with depth 1 .. 7), the two asymmetric-transform flags with their values 2 + 5 + 1,
// the slice counts 2 x 63 (the caller's ints), prefix and scalar or an LD fraction in any terms 2 x 65 (32-bit values),
// the matrix flag 1, 22 entries of 17 bits (0 .. 255; 256 .. 510 are as long and are named in the refusal): 651 bits = 82
// bytes, 103 in all.  A longer head runs off the window and is refused as running past the end.
#define VC2_WALK_WINDOW 128

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
template <typename P> __device__ __forceinline__ void vc2_put(const P &p, unsigned long long at, unsigned v) {
  if (at < p.cap) p.stream[at] = (uint8_t)v;
}
template <typename P>
__device__ void vc2_put_parse_info(const P &p, unsigned long long at, int code, unsigned long long next, unsigned long long prev) {
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
// write, fragmented (DataUnit.cpp:156-232, :267-342)
// ------------------------------------------------------------------------------------------
#define VC2_CUT_THREADS 1024
#define VC2_FRAG_STAGE (16 * VC2_COPY_CHUNK / VC2_FRAG_HEADER + 2) // fragments a chunk of k_frag_copy can meet
#define VC2_CUT_LDS_MAX (144u << 10) // dynamic LDS of k_frag_cut (it holds 4 KiB more statically; a workgroup has 160 KiB)

// marks (one bit per slice) and two arrays of ns + 1 jump targets: 16-bit in LDS, 32-bit in the workspace
static size_t frag_words(int ns) { return ((size_t)ns + 31) >> 5; }
size_t vc2_frag_cut_lds(int ns) {
  const size_t b = frag_words(ns) * 4 + ((((size_t)ns + 1) * 2 * 2 + 3) & ~(size_t)3);
  return ns <= 65535 && b <= VC2_CUT_LDS_MAX ? b : 0;
}
size_t vc2_frag_jump_bytes(int ns) { return (frag_words(ns) + ((size_t)ns + 1) * 2) * 4; }

__device__ __forceinline__ unsigned vc2_frag_p0(const FragParams &p) { return 21u + (unsigned)p.tp_len; } // the parameters fragment
__device__ __forceinline__ unsigned long long vc2_frag_pic_bytes(const FragParams &p, uint4 m) {
  return vc2_frag_p0(p) + (unsigned long long)VC2_FRAG_HEADER * m.x + m.y;
}
__device__ __forceinline__ unsigned vc2_frag_last_unit(const FragParams &p, uint4 m) { // bytes of a picture's last data unit
  return m.x ? VC2_FRAG_HEADER + m.z : vc2_frag_p0(p);
}

// One workgroup per picture.  Slice i starts at payload byte O(i), O(ns) = the payload's length.  A fragment that starts at
// slice i ends before nxt(i) = the largest j with O(j) - O(i) <= fragment_length, or i + 1 (a slice beyond the length travels
// alone): a binary search per slice.  The fragments of the picture are the chain 0, nxt(0), nxt(nxt(0)), ...; it is marked
// by pointer jumping -- round r marks the a[i] of every marked i and squares a -- which ends when a round marks nothing new
// (the marked set is then closed under a = nxt^(2^r) and holds the chain's first 2^r elements: all of it).  A slice marked
// early by a thread that saw this round's marks is still one of the chain.  The marked slices, counted in order, are the table.
template <typename J> __global__ __launch_bounds__(VC2_CUT_THREADS) void k_frag_cut(FragParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned cut_lds[];
  __shared__ unsigned part[VC2_CUT_THREADS];
  __shared__ unsigned long long total_s;
  __shared__ int bad_s, changed_s;
  constexpr int T = VC2_CUT_THREADS;
  const int k = blockIdx.x, t = threadIdx.x, ns = p.ns;
  const unsigned words = (unsigned)(ns + 31) >> 5;
  unsigned *marks = p.jump ? p.jump + (size_t)k * (words + 2 * ((size_t)ns + 1)) : cut_lds;
  J *a = (J *)(marks + words), *b = a + (ns + 1);
  const unsigned long long len = p.lens[k], stride = (unsigned long long)p.payload_stride, plen = len < stride ? len : stride;
  const uint32_t *offs = p.offs + (long long)k * p.offs_stride;
  const uint8_t *slot = p.payload + (long long)k * p.payload_stride;
  if (t == 0) {
    unsigned long long total = p.ld_total;
    bool ok = true;
    if (p.hq) { // the end of the last slice, from its three length bytes
      unsigned long long q = offs[ns - 1];
      ok = offs[0] == 0 && q < plen;
      q += (unsigned)p.prefix + 1;
      for (int c = 0; c < 3 && ok; ++c) {
        ok = q < plen;
        if (ok) q += 1 + (unsigned long long)slot[q] * (unsigned)p.scalar;
      }
      total = q;
    }
    total_s = total;
    bad_s = !ok || total != len || len > stride;
    changed_s = 0;
  }
  __syncthreads();
  if (p.hq) { // the index's offsets ascend (an unreached slice holds 0xFFFFFFFF)
    bool bad = false;
    for (int i = t; i + 1 < ns; i += T) bad |= offs[i] >= offs[i + 1];
    if (bad) bad_s = 1;
  }
  __syncthreads();
  const unsigned long long total = total_s;
  if (bad_s) { // (uniform) no slice fragment is written for this picture
    if (t == 0) {
      p.meta[k] = make_uint4(0, 0, 0, 0);
      atomicOr(p.err, len > stride ? VC2_DEVERR_CAP : VC2_DEVERR_STREAM);
    }
    return;
  }
  const unsigned long long F = p.fragment_length;
  for (int i = t; i < ns; i += T) {
    const unsigned long long o = offs[i];
    int lo = i + 1, hi = ns;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((mid < ns ? (unsigned long long)offs[mid] : total) - o <= F) lo = mid; else hi = mid - 1;
    }
    a[i] = (J)lo;
  }
  if (t == 0) a[ns] = (J)ns;
  for (unsigned w = t; w < words; w += T) marks[w] = w == 0 ? 1u : 0u;
  __syncthreads();
  for (;;) {
    bool ch = false;
    for (int i = t; i < ns; i += T) {
      if (!(marks[i >> 5] >> (i & 31) & 1)) continue;
      const int j = (int)a[i];
      if (j < ns && !(marks[j >> 5] >> (j & 31) & 1)) { atomicOr(&marks[j >> 5], 1u << (j & 31)); ch = true; }
    }
    if (ch) changed_s = 1;
    __syncthreads();
    const int c = changed_s;
    __syncthreads();
    if (!c) break;
    if (t == 0) changed_s = 0;
    for (int i = t; i <= ns; i += T) b[i] = a[a[i]];
    __syncthreads();
    J *x = a; a = b; b = x;
  }
  // the marked slices in order: b[f] = the first slice of fragment f
  const unsigned per = (words + T - 1) / T, w0 = min(words, t * per), w1 = min(words, w0 + per);
  unsigned cnt = 0;
  for (unsigned w = w0; w < w1; ++w) cnt += __popc(marks[w]);
  part[t] = cnt;
  __syncthreads();
  for (int off = 1; off < T; off <<= 1) {
    const unsigned v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned f = part[t] - cnt;
  const unsigned nfrag = part[T - 1];
  for (unsigned w = w0; w < w1; ++w)
    for (unsigned m = marks[w]; m; m &= m - 1) b[f++] = (J)(w * 32 + (__ffs(m) - 1));
  __syncthreads();
  for (f = t; f < nfrag; f += T) {
    const int i = (int)b[f], j = f + 1 < nfrag ? (int)b[f + 1] : ns;
    const unsigned long long o = offs[i], l = (j < ns ? (unsigned long long)offs[j] : total) - o;
    p.table[(size_t)k * ns + f] = make_uint4((unsigned)i, (unsigned)o, (unsigned)l, (unsigned)(j - i));
    if (f == nfrag - 1) p.meta[k] = make_uint4(nfrag, (unsigned)total, (unsigned)l, 0);
    if (l > 65535) { // one slice (several share a fragment only within fragment_length): the 16-bit data length cannot hold it
      *(unsigned long long *)((char *)p.err + VC2_ERRBLK_SYNTAX_AT) = (unsigned long long)k;
      *(unsigned *)((char *)p.err + VC2_ERRBLK_SYNTAX_WHY) = (unsigned)VC2_SYN_SLICE_TOO_LONG;
      __threadfence();
      atomicOr(p.err, VC2_DEVERR_SYNTAX);
    }
  }
}

// one workgroup: the pictures' stream offsets and unit indices by a scan, their parameters fragments, the end of sequence
__global__ __launch_bounds__(VC2_SCAN_THREADS) void k_frag_layout(FragParams p) {
  __shared__ unsigned long long part[VC2_SCAN_THREADS], upart[VC2_SCAN_THREADS];
  const int t = threadIdx.x;
  const int per = (p.n + VC2_SCAN_THREADS - 1) / VC2_SCAN_THREADS;
  const int k0 = min(p.n, t * per), k1 = min(p.n, k0 + per);
  const unsigned p0 = vc2_frag_p0(p);
  unsigned long long sum = 0, usum = 0;
  for (int k = k0; k < k1; ++k) {
    const uint4 m = p.meta[k];
    sum += vc2_frag_pic_bytes(p, m);
    usum += 1ull + m.x;
  }
  part[t] = sum;
  upart[t] = usum;
  __syncthreads();
  for (int off = 1; off < VC2_SCAN_THREADS; off <<= 1) {
    const unsigned long long v = t >= off ? part[t - off] : 0, u = t >= off ? upart[t - off] : 0;
    __syncthreads();
    part[t] += v;
    upart[t] += u;
    __syncthreads();
  }
  unsigned long long at = part[t] - sum, unit = upart[t] - usum;
  for (int k = k0; k < k1; ++k) {
    const uint4 m = p.meta[k];
    p.pic_base[k] = at;
    p.unit_base[k] = unit;
    if (p.unit_offsets && unit < p.unit_cap) p.unit_offsets[unit] = at;
    vc2_put_parse_info(p, at, p.code, p0, k ? vc2_frag_last_unit(p, p.meta[k - 1]) : p.prev_parse_offset);
    const uint32_t pn = p.first_picture_number + (uint32_t)k;
    for (int i = 0; i < 4; ++i) vc2_put(p, at + 13 + i, pn >> (24 - 8 * i));
    vc2_put(p, at + 17, (unsigned)p.tp_len >> 8);
    vc2_put(p, at + 18, (unsigned)p.tp_len);
    vc2_put(p, at + 19, 0);
    vc2_put(p, at + 20, 0);
    for (int i = 0; i < p.tp_len; ++i) vc2_put(p, at + 21 + i, p.tp[i]);
    at += vc2_frag_pic_bytes(p, m);
    unit += 1ull + m.x;
  }
  if (t == 0) {
    const unsigned long long total = part[VC2_SCAN_THREADS - 1], units = upart[VC2_SCAN_THREADS - 1];
    if (p.eos) {
      vc2_put_parse_info(p, total, 0x10, 0, vc2_frag_last_unit(p, p.meta[p.n - 1]));
      if (p.unit_offsets && units < p.unit_cap) p.unit_offsets[units] = total;
    }
    const unsigned long long end = total + (p.eos ? 13 : 0), count = units + (p.eos ? 1 : 0);
    *p.stream_len = end;
    if (p.unit_count) *p.unit_count = count;
    if (end > p.cap || (p.unit_offsets && count > p.unit_cap)) atomicOr(p.err, VC2_DEVERR_CAP);
  }
}

// grid: (fragments / 256, pictures): one thread writes one slice fragment's parse info and header
__global__ __launch_bounds__(256) void k_frag_headers(FragParams p) {
  const int k = blockIdx.y;
  const unsigned f = blockIdx.x * 256 + threadIdx.x;
  if (f >= p.meta[k].x) return;
  const uint4 *tab = p.table + (size_t)k * p.ns;
  const uint4 g = tab[f];
  const unsigned p0 = vc2_frag_p0(p);
  const unsigned long long at = p.pic_base[k] + p0 + (unsigned long long)VC2_FRAG_HEADER * f + g.y, unit = p.unit_base[k] + 1 + f;
  if (p.unit_offsets && unit < p.unit_cap) p.unit_offsets[unit] = at;
  vc2_put_parse_info(p, at, p.code, (unsigned long long)VC2_FRAG_HEADER + g.z, f ? VC2_FRAG_HEADER + tab[f - 1].z : p0);
  const uint32_t pn = p.first_picture_number + (uint32_t)k;
  for (int i = 0; i < 4; ++i) vc2_put(p, at + 13 + i, pn >> (24 - 8 * i));
  const unsigned field[4] = {g.z, g.w, g.x % (unsigned)p.xs, g.x / (unsigned)p.xs}; // data length, slices, slice offset x, y
  for (int i = 0; i < 4; ++i) {
    vc2_put(p, at + 17 + 2 * i, field[i] >> 8);
    vc2_put(p, at + 18 + 2 * i, field[i]);
  }
}

// grid: pictures x chunks of VC2_COPY_CHUNK aligned 16-byte words of the stream, from the picture's first slice fragment on.
// The fragments start at ascending stream offsets: the workgroup finds those its chunk meets, every word its own among them.
__global__ __launch_bounds__(VC2_COPY_THREADS) void k_frag_copy(FragParams p, int chunks) {
  const int k = blockIdx.x / chunks, chunk = blockIdx.x - k * chunks;
  const uint4 m = p.meta[k];
  const int nfrag = (int)m.x;
  if (!nfrag) return;
  const uint4 *tab = p.table + (size_t)k * p.ns;
  const unsigned long long plen = m.y; // (the cut has checked it against the slot)
  const unsigned long long unit0 = p.pic_base[k] + vc2_frag_p0(p); // fragment f's unit is at unit0 + 25 f + tab[f].y
  const unsigned long long all = unit0 + (unsigned long long)VC2_FRAG_HEADER * nfrag + plen, end = all < p.cap ? all : p.cap;
  if (unit0 >= end) return;
  const unsigned long long b1 = (end + 15) >> 4, c0 = (unit0 >> 4) + (unsigned long long)chunk * VC2_COPY_CHUNK;
  if (c0 >= b1) return;
  auto find = [&](unsigned long long x, int lo, int hi) { // the last fragment of [lo, hi] whose unit starts at or before x (else lo)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (unit0 + (unsigned long long)VC2_FRAG_HEADER * mid + tab[mid].y <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
  };
  // the fragments this chunk meets, staged in LDS: their units start at least a header apart, so there are at most
  // VC2_FRAG_STAGE of them; every word then finds its own among them
  __shared__ unsigned long long key_s[VC2_FRAG_STAGE];
  __shared__ uint4 ent_s[VC2_FRAG_STAGE];
  const int fa = find(c0 << 4, 0, nfrag - 1), fb = find(((c0 + VC2_COPY_CHUNK) << 4) - 1, fa, nfrag - 1);
  const int cnt = min(fb - fa + 1, VC2_FRAG_STAGE);
  for (int i = threadIdx.x; i < cnt; i += VC2_COPY_THREADS) {
    const uint4 g = tab[fa + i];
    ent_s[i] = g;
    key_s[i] = unit0 + (unsigned long long)VC2_FRAG_HEADER * (fa + i) + g.y;
  }
  __syncthreads();
  const uint8_t *slot8 = p.payload + (long long)k * p.payload_stride;
#pragma unroll
  for (int i = 0; i < VC2_COPY_WORDS; ++i) {
    const unsigned long long b = c0 + i * VC2_COPY_THREADS + threadIdx.x;
    if (b >= b1) break;
    const unsigned long long x0 = b << 4;
    int lo = 0, hi = cnt - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (key_s[mid] <= x0) lo = mid; else hi = mid - 1;
    }
    const int f = fa + lo;
    const uint4 g = ent_s[lo];
    // the body of fragment f: stream bytes [s0, s1) are slot bytes [g.y, g.y + g.z).  No later body begins in this word (a
    // header is longer than a word); the headers are k_frag_headers'
    const unsigned long long s0 = unit0 + (unsigned long long)VC2_FRAG_HEADER * (f + 1) + g.y, s1 = s0 + g.z;
    const unsigned long long src = g.y + (x0 - s0);
    const unsigned r = (unsigned)(src & 15);
    // whole words of the slot (it is 16-byte aligned) that end inside the payload; every other word goes byte by byte
    if (x0 >= s0 && x0 + 16 <= s1 && x0 + 16 <= end && src - r + (r ? 32 : 16) <= plen) {
      const uint4 *w = (const uint4 *)(slot8 + (src - r));
      *(uint4 *)(p.stream + x0) = r ? vc2_realign(w[0], w[1], r) : w[0];
    } else {
      for (int e = 0; e < 16; ++e) {
        const unsigned long long x = x0 + e;
        if (x >= s0 && x < s1 && x < end) p.stream[x] = slot8[g.y + (x - s0)];
      }
    }
  }
}

void vc2_launch_frag_cut(Launcher &L, const FragParams &p, hipStream_t s) {
  const size_t lds = p.jump ? 0 : vc2_frag_cut_lds(p.ns);
  vc2_prof_begin(L, "frag_cut", s);
  if (p.jump) VC2_LAUNCH(L, k_frag_cut<unsigned>, dim3((unsigned)p.n), dim3(VC2_CUT_THREADS), 0, s, p);
  else {
    vc2_allow_lds((const void *)k_frag_cut<unsigned short>, lds);
    VC2_LAUNCH(L, k_frag_cut<unsigned short>, dim3((unsigned)p.n), dim3(VC2_CUT_THREADS), lds, s, p);
  }
  vc2_prof_end(L, s);
}
void vc2_launch_frag_layout(Launcher &L, const FragParams &p, hipStream_t s) {
  vc2_prof_begin(L, "frag_layout", s);
  VC2_LAUNCH(L, k_frag_layout, dim3(1), dim3(VC2_SCAN_THREADS), 0, s, p);
  VC2_LAUNCH(L, k_frag_headers, dim3((unsigned)((p.ns + 255) / 256), (unsigned)p.n), dim3(256), 0, s, p);
  vc2_prof_end(L, s);
}
void vc2_launch_frag_copy(Launcher &L, const FragParams &p, hipStream_t s) {
  // a picture's slice fragments are at most stride + 25 ns bytes of the stream
  const unsigned long long words = ((unsigned long long)p.payload_stride + (unsigned long long)VC2_FRAG_HEADER * p.ns) / 16 + 2;
  const int chunks = (int)((words + VC2_COPY_CHUNK - 1) / VC2_COPY_CHUNK);
  vc2_prof_begin(L, "frag_copy", s);
  VC2_LAUNCH(L, k_frag_copy, dim3((unsigned)(chunks * p.n)), dim3(VC2_COPY_THREADS), 0, s, p, chunks);
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
// interleaved exp-Golomb (VLC.cpp:304-317).  A code of 32 data bits holds 2^32 - 1 ... 2^33 - 2: the value goes back whole, so
// that a field written as its value + 2^32 differs from the caller's instead of equalling it in 32 bits
__device__ unsigned long long vc2_uvlc(Vc2Bits &r) {
  unsigned long long v = 1;
  for (int n = 0; !vc2_bit(r); ++n) {
    if (n == 32) { r.over = true; break; }
    v = (v << 1) | vc2_bit(r);
  }
  return v - 1;
}
__device__ __forceinline__ uint32_t vc2_be(const unsigned *w, int at, int n) {
  uint32_t v = 0;
  for (int i = 0; i < n; ++i) v = (v << 8) | w[at + i];
  return v;
}
// transform parameters (DataUnit.cpp:1340-1410) against what the caller said the pictures are: 0 or a VC2_SYN_* reason
__device__ int vc2_check_params(const StreamReadParams &p, Vc2Bits &r, int major, bool ld) {
  const unsigned long long kernel = vc2_uvlc(r), depth = vc2_uvlc(r);
  bool asym = false;
  if (major >= 3) {
    if (vc2_bit(r)) asym |= vc2_uvlc(r) != kernel; // asym_transform_index_flag: wavelet_index_ho
    if (vc2_bit(r)) asym |= vc2_uvlc(r) != 0;      // asym_transform_flag: dwt_depth_ho
  }
  const unsigned long long xs = vc2_uvlc(r), ys = vc2_uvlc(r), a = vc2_uvlc(r), b = vc2_uvlc(r);
  const bool custom_matrix = vc2_bit(r);
  if (r.over) return VC2_SYN_PAST_END;
  if (asym) return VC2_SYN_ASYMMETRIC;
  if (ld != (p.ld != 0) || kernel != (uint32_t)p.kernel || depth != (uint32_t)p.depth || xs != (uint32_t)p.xs || ys != (uint32_t)p.ys)
    return VC2_SYN_PARAMS;
  // The picture's effective matrix against the context's (p.qmatrix): its own 3 * depth + 1 entries (LL, then HL, LH, HH per
  // level from the coarsest), or the default of its wavelet and depth -- which are the caller's by now, so the host has
  // compared that one (p.flagless_ok).  Every entry is read before the verdict: an entry above 255 is named as such.
  if (custom_matrix) {
    bool differs = p.qm_entries == 0, too_large = false;
    for (int i = 0; i < 3 * (int)depth + 1 && !too_large; ++i) {
      uint32_t v = 1; // an entry's code by hand: one of more than 17 bits is an entry above 255 whatever follows, not a walk off the window
      for (int n = 0; !vc2_bit(r); ++n) {
        if (n == 9) { too_large = true; break; }
        v = (v << 1) | vc2_bit(r);
      }
      const uint32_t m = v - 1;
      too_large |= m > 255u;
      differs |= i >= p.qm_entries || m != (uint32_t)p.qmatrix[i < VC2_MAX_BANDS ? i : 0];
    }
    if (r.over) return VC2_SYN_PAST_END;
    if (too_large) return VC2_SYN_QM_ENTRY;
    if (differs) return VC2_SYN_QUANT_MATRIX;
  } else if (!p.flagless_ok) return VC2_SYN_QUANT_MATRIX;
  if (r.bit) { r.bit = 0; ++r.pos; }
  if (!ld) return a == p.a && b == p.b ? 0 : VC2_SYN_PARAMS;
  return b && a * p.b == b * p.a ? 0 : VC2_SYN_PARAMS; // the same fraction (a, b < 2^33 and p.a, p.b < 2^31: no overflow)
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
      const unsigned long long v = vc2_uvlc(r);
      major = v > 0x7FFFFFFFull ? 0x7FFFFFFF : (int)v;
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
