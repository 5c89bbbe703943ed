// HQ_CAPPED: every picture of a batch gets ONE quantiser index, the smallest of floor .. 115 at which
// its HQ_CONSTQ payload is at most cap bytes.  The payload's length never grows with the index (see k_cbr_search_reg on
// the slice's bytes; a picture's are their sum), so "fits" has a threshold, found in two rounds that read the slice
// records twice instead of once per bisection step:
//   round 1  measure every picture at floor + 8 k (at most 15 candidates), pick its bracket of eight indices
//   round 2  measure the (at most) seven indices inside the picture's own bracket, pick, fill the picture's indices
// A measurement is a trial, as TRIAL is in bits8_tab: a candidate at which the slice coder would raise VC2HIP_ESCALAR or
// VC2HIP_ECODE32 does not fit (its table entry saturates, VC2_CAP_NOFIT) and raises nothing.
// (Included by vc2hip_slices.hip behind the HQ_CBR search, whose measurements these kernels repeat.)
//
// HQ_CAPPED_FILL adds, for the pictures that left the floor and fit at their index q_i:
//   round 3  measure every SLICE at q_i - 1 and q_i: its cost len_s(q_i - 1) - len_s(q_i), or VC2_CAP_NOCOST where the slice
//            coder would raise at q_i - 1, into CapParams::cost (the FILL instantiations of the two measuring kernels)
//   fill     k_cap_fill: along the bit-reversed visit order, the slices whose running cost stays within cap - L(q_i) get q_i - 1
// q_i, the fill flag and the spare bytes travel in words 27 .. 29 of the picture's table row (k_cap_pick).
//
// vc2hip_set_index_offsets: with a map of signed offsets o_s, slice s is measured and coded at
// e_s(b) = min(max(b + o_s, 0), 115) wherever the text above says "index b": the candidates, the bracket and words 27 .. 29
// are the picture's BASE b_i, and only the index handed to the quantiser and written to qidx is per slice.  e_s never
// decreases with b and a slice's bytes never grow with its index up to 115, so a picture's length is still monotone in b and
// the two rounds bracket as before.  The offset forms are instantiations of their own (OFFS = true), as FILL's are: OFFS =
// false folds every trace of the map away, and the kernels that run without a map keep their code and their registers.
#pragma once
#include <type_traits>

__device__ __forceinline__ int cap_eff(int b, int o) { return min(max(b + o, 0), VC2_CAP_Q_TOP); }
// a slice's offset for a whole wavefront: one byte load, any alignment, made wave-uniform so that the index stays scalar
template <bool OFFS> __device__ __forceinline__ int cap_slice_offset(const CapParams &p, int pic, int slice) {
  if constexpr (OFFS) return __builtin_amdgcn_readfirstlane((int)p.offs[(size_t)pic * p.offs_stride + (size_t)slice]);
  else return 0;
}

struct CapCand { int q0, step, nc, off; }; // candidate k < nc is index q0 + step * k; its sum is word off + k of the picture's row
template <bool FILL>
__device__ __forceinline__ CapCand cap_candidates(const CapParams &p, int pic) {
  CapCand c;
  if constexpr (FILL) { // the third round: q_i - 1 and q_i, per slice (off: unused)
    const unsigned long long *row = p.table + (size_t)pic * VC2_CAP_ROW;
    c.q0 = (int)row[VC2_CAP_QI] - 1; c.step = 1; c.nc = row[VC2_CAP_FILL] ? 2 : 0; c.off = 0;
  } else if (p.round == 0) {
    c.q0 = p.floor; c.step = 8; c.nc = (VC2_CAP_Q_TOP - p.floor) / 8 + 1; c.off = 0;
  } else {
    const unsigned long long *row = p.table + (size_t)pic * VC2_CAP_ROW;
    c.q0 = (int)row[VC2_CAP_BASE] + 1; c.step = 1; c.nc = min((int)row[VC2_CAP_COUNT], 7); c.off = VC2_CAP_R2;
  }
  return c;
}
// the third round's result of one slice, from the lanes that hold its bytes at q_i - 1 (lane 0) and at q_i (lane 1)
__device__ __forceinline__ void cap_store_cost(const CapParams &p, int pic, int slice, unsigned long long val, int lane) {
  const unsigned long long v0 = __shfl(val, 0), v1 = __shfl(val, 1);
  if (lane == 0) p.cost[(size_t)pic * p.s.n_slices + slice] = v0 >= VC2_CAP_NOFIT ? VC2_CAP_NOCOST : (unsigned)(v0 - v1);
}

// component_bits<true, false> that also says whether a code passes 32 bits (big), and touches no error flag
template <class Src>
__device__ __forceinline__ int cap_component_bits(Src src, int n, int n0, int q, const int *qm, int lane, bool &big) {
  int base = 0, count = 0;
  const int n0_shift = (n0 & (n0 - 1)) == 0 ? 31 - __clz(n0) : -1;
  for (int r0 = 0; r0 < n; r0 += 512) {
    int sum = 0, last_end = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int j = r0 + lane * 8 + k;
      if (j < n) {
        const int aq = min(max(q - qm[band_of_index_fast(j, n0, n0_shift)], 0), 119);
        const int c = quant_dev(src(j), aq);
        const int nb = svlc_bits(c);
        big |= nb > 32;
        sum += nb;
        if (c != 0) last_end = sum;
      }
    }
    const int incl = wave_incl_scan(sum, lane);
    count = max(count, wave_max(last_end ? base + incl - sum + last_end : 0));
    base += __shfl(incl, 63);
  }
  return count;
}

// The general form: one wavefront per slice, any geometry and either store; the slice staged in LDS, or (GLOBAL) read from
// the store at every candidate.  only_marked: the pass behind k_cap_measure16 over the slices it handed back.
template <class ST, bool GLOBAL, bool FILL, bool OFFS>
__global__ __launch_bounds__(256) void k_cap_measure(const CapParams p) {
  extern __shared__ __attribute__((aligned(16))) int lds_i[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpw = blockDim.x >> 6;
  const int pic = blockIdx.y;
  const CapCand cd = cap_candidates<FILL>(p, pic);
  if (cd.nc <= 0) return; // (no workgroup barrier anywhere in this kernel)
  unsigned long long mine = 0; // lane k: candidate k's bytes over this wavefront's slices
  auto measure = [&](const int slice) {
    int *co = lds_i + (GLOBAL ? 0 : wave * p.s.slice_coefs);
    const size_t rec_at = (size_t)pic * p.s.store_stride + (size_t)slice * p.s.slice_coefs;
    const ST *rec = (const ST *)p.s.store + rec_at;
    const int32_t *recw = St<ST>::narrow ? p.s.store_wide + rec_at : nullptr;
    if constexpr (!GLOBAL) {
      if ((p.s.slice_coefs & 7) == 0 && (rec_at & 7) == 0) {
        for (int i = lane * 8; i < p.s.slice_coefs; i += 512) {
          int e[8];
          St<ST>::load8(rec + i, recw + i, e);
          *(int4 *)(co + i) = make_int4(e[0], e[1], e[2], e[3]);
          *(int4 *)(co + i + 4) = make_int4(e[4], e[5], e[6], e[7]);
        }
      } else {
        for (int i = lane; i < p.s.slice_coefs; i += 64) co[i] = St<ST>::load1(rec + i, recw + i);
      }
      wave_lds_sync(); // no cross-wave sharing of `co`
    }
    unsigned long long val = (unsigned long long)(p.prefix + 4); // a candidate behind the first all-zero one: nothing but the header
    const int o = cap_slice_offset<OFFS>(p, pic, slice);
    for (int k = 0; k < cd.nc; ++k) {
      const int tq = OFFS ? cap_eff(cd.q0 + cd.step * k, o) : cd.q0 + cd.step * k; // (never decreases with k: the early exit below stands)
      bool big = false;
      int need = 0;
      for (int c = 0; c < 3; ++c) {
        const int off = p.s.comp_off[c];
        int count;
        if constexpr (GLOBAL) count = cap_component_bits([&](int j) { return St<ST>::load1(rec + off + j, recw + off + j); }, p.s.comp_n[c],
                                                         p.s.comp_n0[c], tq, p.s.qmatrix, lane, big);
        else count = cap_component_bits([&](int j) { return co[off + j]; }, p.s.comp_n[c], p.s.comp_n0[c], tq, p.s.qmatrix, lane, big);
        const int len = ((count + 7) / 8 + p.s.scalar - 1) / p.s.scalar;
        big |= len > 255;
        need += len * p.s.scalar;
      }
      big = __any(big);
      if (lane == k) val = big ? VC2_CAP_NOFIT : (unsigned long long)(p.prefix + 4 + need);
      if (!big && need == 0) break; // no coefficient left, at this index and at every larger one
    }
    if constexpr (FILL) cap_store_cost(p, pic, slice, val, lane);
    else mine += val;
    if constexpr (!GLOBAL) wave_lds_sync();
  };
  const int first = blockIdx.x * wpw + wave;
  if (!p.s.only_marked) {
    if (first < p.s.n_slices) measure(first);
  } else { // 64 marks per look: the wavefronts of the small grid stride over the picture's slices
    for (int base = first * 64; base < p.s.n_slices; base += (int)gridDim.x * wpw * 64) {
      const bool marked = base + lane < p.s.n_slices && p.s.qidx[(size_t)pic * p.s.n_slices + base + lane] == VC2_CBR_MARK;
      for (unsigned long long m = __ballot(marked); m; m &= m - 1) measure(base + __ffsll((long long)m) - 1);
    }
  }
  if constexpr (!FILL)
    if (lane < cd.nc && mine) atomicAdd(&p.table[(size_t)pic * VC2_CAP_ROW + cd.off + lane], mine);
}

// The fast form: the lane layout and the float measurement of k_cbr_search16 (vc2hip_cbr16.h: cbr16_plan, need_bytes) for
// the common geometry on the 16-bit store, CBR_SPW consecutive slices per wavefront and ONE atomic per wavefront.  A slice
// with an escape of the 16-bit store is marked and left to k_cap_measure.
// The quantiser table stops at index 79 as k_cbr_search16's does, and larger adjusted indices read entry 79; here that is
// exact, so no index is handed back: a magnitude of the 16-bit store is at most 32767, 4 * 32767 < factor(79) = 3 526 975
// <= factor(a) for 79 <= a <= 115, so both the true quotient and fl(|c| * r79) < 1 are zero.
// With index offsets the argument is the same one: every e_s(b) <= 115 by its clamp, a band's index max(e_s(b) - m, 0) no
// larger, and entry() keeps the table offset inside 0 .. 79 * 16 whatever the offset's value.
template <bool FILL, bool OFFS>
__global__ __launch_bounds__(256, VC2_CBR16_WPE) void k_cap_measure16(const CapParams p) {
  __shared__ uint4 s_tab[80]; // by quantiser index: (rounded-up 4 / factor as a float, -, -, -)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slice0 = (blockIdx.x * 4 + wave) * CBR_SPW, pic = blockIdx.y;
  if (threadIdx.x < 80) s_tab[threadIdx.x] = make_uint4(__float_as_uint(c_qs.inv4[threadIdx.x]), 0u, 0u, 0u);
  const unsigned lq = p.s.lane8[lane];
  const int headY = (int)p.s.lane8[64], headC = (int)p.s.lane8[65], runsY = (int)p.s.lane8[66], runsC = (int)p.s.lane8[67];
  const CapCand cd = cap_candidates<FILL>(p, pic);
  __syncthreads();
  if (cd.nc <= 0) return;
  const bool has_y = lane < runsY, has_c = lane < 2 * runsC;
  const int ccb = lane < runsC ? 1 : 2, crun = lane < runsC ? lane : lane - runsC; // the chroma run's component, its number
  const int hc = lane < 32 ? 0 : (lane < 48 ? 1 : 2), hj = lane - (lane < 32 ? 0 : (lane < 48 ? 32 : 48)); // the head coefficient's
  const bool has_h = hj < (hc == 0 ? headY : headC);
  const int m_y = 16 * (int)(lq & 0xFFu), m_c = 16 * (int)((lq >> 8) & 0xFFu), m_h = 16 * (int)((lq >> 16) & 0xFFu);
  const char *tab = (const char *)s_tab;
  unsigned long long mine = 0;
  for (int slice = slice0; slice < min(slice0 + CBR_SPW, p.s.n_slices); ++slice) { // no workgroup barriers below
    const size_t rec_at = (size_t)pic * p.s.store_stride + (size_t)slice * p.s.slice_coefs;
    const int16_t *rec = (const int16_t *)p.s.store + rec_at;
    float fy[8], fc[8], fh = 0.f; // |coefficient|
    bool out = false;
    {
      uint4 wy = make_uint4(0u, 0u, 0u, 0u), wc = wy;
      int hv = 0;
      if (has_y) wy = *(const uint4 *)(rec + p.s.comp_off[0] + headY + 8 * lane);
      if (has_c) wc = *(const uint4 *)(rec + p.s.comp_off[ccb] + headC + 8 * crun);
      if (has_h) hv = rec[p.s.comp_off[hc] + hj];
      const unsigned dy[4] = {wy.x, wy.y, wy.z, wy.w}, dc[4] = {wc.x, wc.y, wc.z, wc.w};
      float mx = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        fy[2 * k] = __builtin_fabsf((float)(int)(short)(dy[k] & 0xFFFFu)); fy[2 * k + 1] = __builtin_fabsf((float)((int)dy[k] >> 16));
        fc[2 * k] = __builtin_fabsf((float)(int)(short)(dc[k] & 0xFFFFu)); fc[2 * k + 1] = __builtin_fabsf((float)((int)dc[k] >> 16));
        mx = fmaxf(mx, fmaxf(fmaxf(fy[2 * k], fy[2 * k + 1]), fmaxf(fc[2 * k], fc[2 * k + 1])));
      }
      fh = __builtin_fabsf((float)hv);
      out = fmaxf(mx, fh) > 32767.f; // an escape of the 16-bit store (the sentinel is -32768): the general kernel
    }
    out = __any(out);
    if (lane == 0) p.s.qidx[(size_t)pic * p.s.n_slices + slice] = out ? VC2_CBR_MARK : 0;
    if (out) continue;
    auto entry = [&](int tq16, int m) -> int { return min(max(tq16 - m, 0), 16 * 79); };
    auto bits8u = [&](const float (&f)[8], float r, bool has, int &sum, int &last_end) { // see k_cbr_search16
      sum = 0; last_end = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int eb = (int)__builtin_amdgcn_ubfe(__float_as_uint(__builtin_fmaf(f[k], r, 1.0f)), 23, 8); // 127 + E
        sum += 2 * eb + min(eb, 128) - 380;                                                               // 2E + min(E, 1) + 1
        last_end = eb >= 128 ? sum : last_end;
      }
      if (!has) { sum = 0; last_end = 0; }
    };
    auto comp_bytes = [&](int count, bool &bad) -> int {
      const int len = (int)((float)(((count + 7) >> 3) + p.s.scalar - 1) * p.s.inv_scalar);
      bad |= len > 255;
      return __mul24(len, p.s.scalar);
    };
    auto last_of = [&](unsigned long long body, unsigned long long head, int v_body, int v_head) -> int {
      if (body) return __builtin_amdgcn_readlane(v_body, 63 - __builtin_clzll(body));
      if (head) return __builtin_amdgcn_readlane(v_head, 63 - __builtin_clzll(head));
      return 0;
    };
    auto need_bytes = [&](int tq, bool &bad) -> int { // k_cbr_search16's, without its limit on the index (see above)
      const float ry = *(const float *)(tab + entry(16 * tq, m_y)), rc = *(const float *)(tab + entry(16 * tq, m_c)),
                  rh = *(const float *)(tab + entry(16 * tq, m_h));
      int sy, ly, sc, lc;
      bits8u(fy, ry, has_y, sy, ly);
      bits8u(fc, rc, has_c, sc, lc);
      const int ebh = (int)__builtin_amdgcn_ubfe(__float_as_uint(__builtin_fmaf(fh, rh, 1.0f)), 23, 8);
      const int hb = has_h ? 2 * ebh + min(ebh, 128) - 380 : 0;
      const bool hnz = has_h && ebh >= 128;
      const int pk1 = ((hc == 0 ? hb : 0) << 16) | sy, pk2 = ((hc != 0 ? hb : 0) << 16) | sc;
      const int s1 = wave_incl_scan(pk1, lane), s2 = wave_incl_scan(pk2, lane);
      const int e1 = s1 - pk1, e2 = s2 - pk2;
      const int tot_hy = __builtin_amdgcn_readlane(s1, 63) >> 16;
      const int tot_hu = __builtin_amdgcn_readlane(s2, 47) >> 16, tot_hv = (__builtin_amdgcn_readlane(s2, 63) >> 16) - tot_hu;
      const int tot_bu = __builtin_amdgcn_readlane(s2, runsC - 1) & 0xFFFF;
      const int end_yb = tot_hy + (e1 & 0xFFFF) + ly, end_yh = (e1 >> 16) + hb;
      const int end_cb = (ccb == 1 ? tot_hu + (e2 & 0xFFFF) : tot_hv + (e2 & 0xFFFF) - tot_bu) + lc;
      const int end_ch = (e2 >> 16) - (hc == 2 ? tot_hu : 0) + hb;
      const unsigned long long b_y = __ballot(ly != 0), h_y = __ballot(hnz && hc == 0);
      const unsigned long long b_c = __ballot(lc != 0), h_c = __ballot(hnz && hc != 0);
      const unsigned long long u_lanes = runsC >= 64 ? ~0ull : ((1ull << runsC) - 1);
      int need = comp_bytes(last_of(b_y, h_y, end_yb, end_yh), bad);
      need += comp_bytes(last_of(b_c & u_lanes, h_c & 0x0000FFFF00000000ull, end_cb, end_ch), bad);
      need += comp_bytes(last_of(b_c & ~u_lanes, h_c & 0xFFFF000000000000ull, end_cb, end_ch), bad);
      return need;
    };
    unsigned long long val = (unsigned long long)(p.prefix + 4);
    const int o = cap_slice_offset<OFFS>(p, pic, slice);
    for (int k = 0; k < cd.nc; ++k) {
      bool bad = false; // (a length byte beyond 255; a code beyond 32 bits needs a quotient above 65534: not from 16-bit magnitudes)
      const int need = need_bytes(OFFS ? cap_eff(cd.q0 + cd.step * k, o) : cd.q0 + cd.step * k, bad);
      if (lane == k) val = bad ? VC2_CAP_NOFIT : (unsigned long long)(p.prefix + 4 + need);
      if (!bad && need == 0) break;
    }
    if constexpr (FILL) cap_store_cost(p, pic, slice, val, lane);
    else mine += val;
  }
  if constexpr (!FILL)
    if (lane < cd.nc && mine) atomicAdd(&p.table[(size_t)pic * VC2_CAP_ROW + cd.off + lane], mine);
}

// The pick, per picture.  Round 1 (one thread): the first fitting candidate closes a bracket of eight indices whose lower
// end does not fit -- base, the count of indices to measure inside it, and the index if none of those fits.  Round 2: the
// smallest fitting index of the bracket, written to the picture's n_slices entries of qidx -- and, for HQ_CAPPED_FILL, q_i,
// whether the picture is to be filled (it left the floor and fits at q_i) and its spare bytes cap - L(q_i), L(q_i) from
// the table: the round-2 entry that fitted, or the round-1 entry of an index floor + 8 k.
// OFFS: q is the picture's base b_i, slice i's entry of qidx is e_i(b_i), and words 27 .. 29 carry b_i.
template <bool OFFS>
__global__ __launch_bounds__(256) void k_cap_pick(const CapParams p) {
  const int pic = blockIdx.y;
  unsigned long long *row = p.table + (size_t)pic * VC2_CAP_ROW;
  auto fits = [&](unsigned long long v) { return v < VC2_CAP_NOFIT && v <= p.cap; };
  if (p.round == 0) {
    if (threadIdx.x) return;
    const int n1 = (VC2_CAP_Q_TOP - p.floor) / 8 + 1;
    int k = 0;
    while (k < n1 && !fits(row[k])) ++k;
    int base, count, other;
    if (k == 0) { base = p.floor; count = 0; other = p.floor; }                       // the floor itself fits
    else if (k < n1) { base = p.floor + 8 * (k - 1); count = 7; other = base + 8; }
    else { base = p.floor + 8 * (n1 - 1); count = min(7, VC2_CAP_Q_TOP - base); other = VC2_CAP_Q_TOP; } // nothing fit so far
    row[VC2_CAP_BASE] = (unsigned long long)base; row[VC2_CAP_COUNT] = (unsigned long long)count; row[VC2_CAP_ELSE] = (unsigned long long)other;
    return;
  }
  const int base = (int)row[VC2_CAP_BASE], count = min((int)row[VC2_CAP_COUNT], 7);
  int q = (int)row[VC2_CAP_ELSE];
  int hit = -1;
  for (int j = count - 1; j >= 0; --j) if (fits(row[VC2_CAP_R2 + j])) { q = base + 1 + j; hit = j; }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < p.s.n_slices) p.s.qidx[(size_t)pic * p.s.n_slices + i] = OFFS ? cap_eff(q, (int)p.offs[(size_t)pic * p.offs_stride + (size_t)i]) : q;
  if (i == 0) { // (words no thread of this launch reads)
    const unsigned long long len = hit >= 0 ? row[VC2_CAP_R2 + hit] : ((q - p.floor) % 8 == 0 ? row[(q - p.floor) / 8] : VC2_CAP_NOFIT);
    const bool fill = q > p.floor && fits(len);
    row[VC2_CAP_QI] = (unsigned long long)q; row[VC2_CAP_FILL] = fill ? 1ull : 0ull; row[VC2_CAP_SPARE] = fill ? p.cap - len : 0ull;
  }
}

// HQ_CAPPED_FILL's index map, one workgroup per picture.  B = the bits of n_slices - 1; position k = 0 .. 2^B - 1 visits
// slice rev_B(k) (positions past the picture are skipped), and the slice there gets q_i - 1 iff it has a cost and the running
// sum of the costs through k, in 64 bits, is at most the spare bytes.  256 positions per turn: an inclusive scan in each
// wavefront, the four totals through LDS, the carry in a register.  Pictures with nothing to fill keep k_cap_pick's indices.
// OFFS: qi is the base b_i; a promoted slice gets e_s(b_i - 1), every other e_s(b_i) (equal where the clamp acts: its cost was 0).
template <bool OFFS>
__global__ __launch_bounds__(256) void k_cap_fill(const CapParams p) {
  __shared__ unsigned long long s_tot[4];
  const int pic = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long *row = p.table + (size_t)pic * VC2_CAP_ROW;
  if (!row[VC2_CAP_FILL]) return; // (the whole workgroup)
  const int ns = p.s.n_slices, qi = (int)row[VC2_CAP_QI];
  const unsigned long long spare = row[VC2_CAP_SPARE];
  const int bits = ns > 1 ? 32 - __clz(ns - 1) : 0;
  const unsigned *cost = p.cost + (size_t)pic * ns;
  int32_t *q = p.s.qidx + (size_t)pic * ns;
  unsigned long long carry = 0;
  for (int k0 = 0; k0 < (1 << bits); k0 += 256) {
    const int k = k0 + (int)threadIdx.x;
    const int slice = bits ? (int)(__brev((unsigned)k) >> (32 - bits)) : 0;
    const bool valid = k < (1 << bits) && slice < ns;
    const unsigned c = valid ? cost[slice] : VC2_CAP_NOCOST;
    const bool eligible = c != VC2_CAP_NOCOST;
    unsigned long long v = eligible ? (unsigned long long)c : 0ull;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long t = __shfl_up(v, d);
      if (lane >= d) v += t;
    }
    if (lane == 63) s_tot[wave] = v;
    __syncthreads();
    unsigned long long before = carry, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const unsigned long long t = s_tot[w];
      if (w < wave) before += t;
      total += t;
    }
    if (valid) {
      const int b = eligible && before + v <= spare ? qi - 1 : qi;
      q[slice] = OFFS ? cap_eff(b, (int)p.offs[(size_t)pic * p.offs_stride + (size_t)slice]) : b;
    }
    carry += total;
    __syncthreads(); // s_tot is written again
  }
}

void vc2_launch_cap(Launcher &L, const CapParams &p0, int n_pictures, hipStream_t s) {
  CapParams p = p0;
  p.s.qm_min = 0;
  p.s.inv_scalar = 1.0f / (float)p.s.scalar; // the smallest float >= 1 / scalar
  if ((double)p.s.inv_scalar < 1.0 / (double)p.s.scalar) p.s.inv_scalar = nextafterf(p.s.inv_scalar, INFINITY);
  const CbrParams &g = p.s;
  // (general_only = VC2HIP_FLAG_CAP_GENERAL: A/B and test switch).  The conditions of k_cbr_search16 in vc2_launch_cbr
  CapParams p16 = p;
  const bool fast = !g.general_only && g.comp_n[0] <= 512 && g.comp_n[1] <= 256 && g.comp_n[1] == g.comp_n[2] && g.n_bands <= 32 &&
                    g.comp_n[0] % 8 == 0 && g.comp_n[1] % 8 == 0 && (g.store_stride % 8) == 0 && (g.slice_coefs % 8) == 0 &&
                    g.comp_off[1] % 8 == 0 && g.comp_off[2] % 8 == 0 && cbr16_plan(p16.s, p16.s.lane8);
  const size_t per_wave = (size_t)g.slice_coefs * 4;
  const bool global = per_wave > 160 * 1024; // the slice does not fit in LDS: every candidate reads it from the store
  const int wpw = global ? 4 : std::max(1, std::min(4, (int)((160 * 1024) / per_wave)));
  static const char *const names[3] = {"cap_measure1", "cap_measure2", "cap_measure3"};
  const bool offs = p.offs != nullptr; // the offset forms: the same rounds under the same names
  for (int round = 0; round < (p.cost ? 3 : 2); ++round) {
    const bool fill = round == 2;
    vc2_prof_begin(L, names[round], s);
    p.round = p16.round = round;
    p.s.only_marked = 0;
    if (fast) {
      const int per_wg = 4 * CBR_SPW;
      const dim3 grid16((g.n_slices + per_wg - 1) / per_wg, n_pictures);
      void (*const fast16)(const CapParams) = fill ? (offs ? k_cap_measure16<true, true> : k_cap_measure16<true, false>)
                                                   : (offs ? k_cap_measure16<false, true> : k_cap_measure16<false, false>);
      VC2_LAUNCH(L, fast16, grid16, dim3(256), 0, s, p16);
      p.s.only_marked = 1;
    }
    const int gx = p.s.only_marked ? std::min((g.n_slices + wpw - 1) / wpw, 64) : (g.n_slices + wpw - 1) / wpw;
    const dim3 grid(gx, n_pictures), block(64 * wpw);
    auto general = [&](auto st, auto gl, auto fl) { // one launch of k_cap_measure<ST, GLOBAL, FILL>
      using ST = decltype(st);
      constexpr bool GL = decltype(gl)::value, FL = decltype(fl)::value;
      void (*const kernel)(const CapParams) = offs ? k_cap_measure<ST, GL, FL, true> : k_cap_measure<ST, GL, FL, false>;
      if (!GL) vc2_allow_lds((const void *)kernel, 160 * 1024);
      VC2_LAUNCH(L, kernel, grid, block, GL ? 0 : wpw * per_wave, s, p);
    };
    auto by_store = [&](auto gl, auto fl) {
      if (g.store16) general(int16_t(), gl, fl);
      else general(int32_t(), gl, fl);
    };
    if (global) { if (fill) by_store(std::true_type(), std::true_type()); else by_store(std::true_type(), std::false_type()); }
    else { if (fill) by_store(std::false_type(), std::true_type()); else by_store(std::false_type(), std::false_type()); }
    vc2_prof_end(L, s);
    vc2_prof_begin(L, fill ? "cap_fill" : "cap_pick", s);
    if (fill) VC2_LAUNCH(L, offs ? k_cap_fill<true> : k_cap_fill<false>, dim3(1, n_pictures), dim3(256), 0, s, p);
    else VC2_LAUNCH(L, offs ? k_cap_pick<true> : k_cap_pick<false>, dim3(round ? (g.n_slices + 255) / 256 : 1, n_pictures), dim3(256), 0, s, p);
    vc2_prof_end(L, s);
  }
}
