// Packed and semi-planar pictures on the device batch path (vc2hip_set_packed_format).
//
// The transform's edge kernels read and write planes.  A picture that reaches the GPU as v210 (six 4:2:2 10-bit pixels in
// four little-endian dwords) or with its chroma as one plane of U, V word pairs (NV12 / NV16 / NV24, P010 / P210 / P016) is
// converted to and from a context-owned planar staging buffer by the bandwidth-bound kernels of this file, on the call's
// stream, in front of the first and behind the last transform launch:
//   k_v210_unpack     v210 rows -> Y, U, V staging planes (16-bit little-endian LSB-justified words)
//   k_v210_pack       the inverse; every group of a row is written whole, unused bits and fields zero
//   k_uv_deinterleave the UV plane -> U and V staging planes; the words' bytes are carried through unchanged
//   k_uv_interleave   the inverse
// Grids follow n, the rows and the width only.  No LDS, no scratch.
#include "vc2hip_internal.h"

void vc2_prof_begin(Launcher &L, const char *name, hipStream_t s);
void vc2_prof_end(Launcher &L, hipStream_t s);

namespace {
typedef int nt4_t __attribute__((ext_vector_type(4)));
// the caller's buffer is read once and written once per call: streaming loads and stores, as the edge kernels' raw rows
__device__ __forceinline__ uint4 ld_nt(const void *p) {
  const nt4_t x = __builtin_nontemporal_load((const __attribute__((address_space(1))) nt4_t *)(size_t)p);
  return make_uint4((unsigned)x.x, (unsigned)x.y, (unsigned)x.z, (unsigned)x.w);
}
__device__ __forceinline__ void st_nt(void *p, uint4 v) {
  const nt4_t x = {(int)v.x, (int)v.y, (int)v.z, (int)v.w};
  __builtin_nontemporal_store(x, (__attribute__((address_space(1))) nt4_t *)(size_t)p);
}

// The six luma and 3 + 3 chroma samples of one v210 group (bits 30 - 31 of every word ignored):
//   w0 = Cb0 | Y0 << 10 | Cr0 << 20    w1 = Y1 | Cb1 << 10 | Y2 << 20    w2 = Cr1 | Y3 << 10 | Cb2 << 20    w3 = Y4 | Cr2 << 10 | Y5 << 20
__device__ __forceinline__ void v210_split(const uint4 w, unsigned y[6], unsigned u[3], unsigned v[3]) {
  u[0] = w.x & 1023u; y[0] = (w.x >> 10) & 1023u; v[0] = (w.x >> 20) & 1023u;
  y[1] = w.y & 1023u; u[1] = (w.y >> 10) & 1023u; y[2] = (w.y >> 20) & 1023u;
  v[1] = w.z & 1023u; y[3] = (w.z >> 10) & 1023u; u[2] = (w.z >> 20) & 1023u;
  y[4] = w.w & 1023u; v[2] = (w.w >> 10) & 1023u; y[5] = (w.w >> 20) & 1023u;
}
__device__ __forceinline__ uint4 v210_join(const unsigned y[6], const unsigned u[3], const unsigned v[3]) {
  uint4 w;
  w.x = (u[0] & 1023u) | (y[0] & 1023u) << 10 | (v[0] & 1023u) << 20;
  w.y = (y[1] & 1023u) | (u[1] & 1023u) << 10 | (y[2] & 1023u) << 20;
  w.z = (v[1] & 1023u) | (y[3] & 1023u) << 10 | (u[2] & 1023u) << 20;
  w.w = (y[4] & 1023u) | (v[2] & 1023u) << 10 | (y[5] & 1023u) << 20;
  return w;
}

// One work-item: one group = 16 bytes of v210, so a wavefront's load or store covers 1024 consecutive bytes of the caller's
// row.  On the staging side a group is 12 bytes of Y (three dwords) and 6 + 6 bytes of chroma; two neighbouring lanes (groups
// 2m and 2m + 1, always of one row: a row's work-items are rounded up to an even count) share the three dwords that hold
// their six U samples, and likewise V: the even lane moves dwords 0 and 1, the odd lane dword 2, and the one sample that
// sits in the other lane's dword crosses by a lane shuffle.  Every sample is tested against the row's width, which is where
// the partial last group and its zero fields come from; a dword whose first sample is inside the row lies inside the
// staging row's pitch (rows are pitched to 16 bytes; an odd chroma width leaves two bytes of slack).
// grid (blocks over rows * work-items per row, pictures)
template <bool PACK>
__global__ __launch_bounds__(256) void k_v210(const PackedParams p) {
  const int groups = (p.width + 5) / 6, cw = p.width >> 1;
  const unsigned gpr = (unsigned)(groups + 1) & ~1u;
  const unsigned i = blockIdx.x * 256u + threadIdx.x; // (rows * work-items per row < 2^28: a plane stays below 2^31 bytes)
  const unsigned r0 = i / gpr;
  const int g = (int)(i - r0 * gpr), m = g >> 1;
  const bool live = r0 < (unsigned)p.rows && g < groups, even = !(g & 1);
  const int r = live ? (int)r0 : 0;
  const int pic = blockIdx.y;
  uint8_t *row = p.packed + (long long)pic * p.packed_stride + (long long)r * p.packed_pitch;
  unsigned *qy = (unsigned *)(p.plane[0] + (long long)pic * p.plane_stride + (long long)r * p.plane_pitch[0]) + 3 * g;
  unsigned *qu = (unsigned *)(p.plane[1] + (long long)pic * p.plane_stride + (long long)r * p.plane_pitch[1]) + 3 * m;
  unsigned *qv = (unsigned *)(p.plane[2] + (long long)pic * p.plane_stride + (long long)r * p.plane_pitch[2]) + 3 * m;
  // the pair's chroma dwords: samples 6m, 6m + 1 | 6m + 2, 6m + 3 | 6m + 4, 6m + 5 -- inside the row by their first sample
  const bool c0 = live && even && 6 * m < cw, c1 = live && even && 6 * m + 2 < cw, c2 = live && !even && 6 * m + 4 < cw;
  unsigned y[6], u[3], v[3];
  if constexpr (!PACK) {
    uint4 w = make_uint4(0, 0, 0, 0);
    if (live) w = ld_nt(row + 16ll * g);
    v210_split(w, y, u, v);
    const unsigned nu = __shfl_down(u[0], 1), nv = __shfl_down(v[0], 1); // the odd lane's first chroma samples (6m + 3)
    if (live) {
#pragma unroll
      for (int k = 0; k < 3; ++k) if (6 * g + 2 * k < p.width) qy[k] = y[2 * k] | y[2 * k + 1] << 16;
    }
    if (c0) { qu[0] = u[0] | u[1] << 16; qv[0] = v[0] | v[1] << 16; }
    if (c1) { qu[1] = u[2] | nu << 16; qv[1] = v[2] | nv << 16; }
    if (c2) { qu[2] = u[1] | u[2] << 16; qv[2] = v[1] | v[2] << 16; }
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const unsigned t = live && 6 * g + 2 * k < p.width ? qy[k] : 0u;
      y[2 * k] = t & 0xFFFFu; y[2 * k + 1] = t >> 16;
    }
    const unsigned u0 = c0 ? qu[0] : 0u, v0 = c0 ? qv[0] : 0u, u1 = c1 ? qu[1] : 0u, v1 = c1 ? qv[1] : 0u;
    const unsigned u2 = c2 ? qu[2] : 0u, v2 = c2 ? qv[2] : 0u;
    const unsigned pu = __shfl_up(u1 >> 16, 1), pv = __shfl_up(v1 >> 16, 1); // sample 6m + 3, from the even lane's second dword
    if (even) { u[0] = u0 & 0xFFFFu; u[1] = u0 >> 16; u[2] = u1 & 0xFFFFu; v[0] = v0 & 0xFFFFu; v[1] = v0 >> 16; v[2] = v1 & 0xFFFFu; }
    else { u[0] = pu; u[1] = u2 & 0xFFFFu; u[2] = u2 >> 16; v[0] = pv; v[1] = v2 & 0xFFFFu; v[2] = v2 >> 16; }
#pragma unroll
    for (int k = 0; k < 3; ++k) if (3 * g + k >= cw) u[k] = v[k] = 0u; // (the fields beyond the row's width are written as zero)
    if (live) st_nt(row + 16ll * g, v210_join(y, u, v));
  }
}

// The UV plane of a semi-planar picture: rows of p.width pairs of WB-byte words, U then V.  One work-item: 32 bytes of pairs
// = 16 bytes of U and 16 of V, split or merged by v_perm (bytes move, none is interpreted: byte order and justification are
// the caller's on both sides).  p.vec == 0 (a row of the caller's plane may start off a 16-byte boundary: tight rows, packed
// pictures) and behind a row's last whole piece: pair by pair.
template <int WB, bool PACK>
__global__ __launch_bounds__(256) void k_uv(const PackedParams p) {
  constexpr int PER = 16 / WB; // pairs of one piece
  const int pieces = p.vec ? p.width / PER : 0;
  const unsigned ipr = (unsigned)(pieces + (p.width - pieces * PER));
  const unsigned i = blockIdx.x * 256u + threadIdx.x; // (rows * items per row < 2^30: a plane stays below 2^31 bytes, an item is 2 bytes or more)
  if (i >= (unsigned)p.rows * ipr) return;
  const int r = (int)(i / ipr), j = (int)(i - (unsigned)r * ipr);
  const int pic = blockIdx.y;
  uint8_t *row = p.packed + (long long)pic * p.packed_stride + (long long)r * p.packed_pitch;
  uint8_t *pu = p.plane[1] + (long long)pic * p.plane_stride + (long long)r * p.plane_pitch[1];
  uint8_t *pv = p.plane[2] + (long long)pic * p.plane_stride + (long long)r * p.plane_pitch[2];
  constexpr unsigned SEL_U = WB == 2 ? 0x05040100u : 0x06040200u, SEL_V = WB == 2 ? 0x07060302u : 0x07050301u; // pairs -> planes
  constexpr unsigned SEL_LO = WB == 2 ? 0x05040100u : 0x05010400u, SEL_HI = WB == 2 ? 0x07060302u : 0x07030602u; // planes -> pairs
  if (j < pieces) {
    if constexpr (!PACK) {
      const uint4 a = ld_nt(row + 32ll * j), b = ld_nt(row + 32ll * j + 16);
      *(uint4 *)(pu + 16ll * j) = make_uint4(__builtin_amdgcn_perm(a.y, a.x, SEL_U), __builtin_amdgcn_perm(a.w, a.z, SEL_U),
                                             __builtin_amdgcn_perm(b.y, b.x, SEL_U), __builtin_amdgcn_perm(b.w, b.z, SEL_U));
      *(uint4 *)(pv + 16ll * j) = make_uint4(__builtin_amdgcn_perm(a.y, a.x, SEL_V), __builtin_amdgcn_perm(a.w, a.z, SEL_V),
                                             __builtin_amdgcn_perm(b.y, b.x, SEL_V), __builtin_amdgcn_perm(b.w, b.z, SEL_V));
    } else {
      const uint4 u = *(const uint4 *)(pu + 16ll * j), v = *(const uint4 *)(pv + 16ll * j);
      st_nt(row + 32ll * j, make_uint4(__builtin_amdgcn_perm(v.x, u.x, SEL_LO), __builtin_amdgcn_perm(v.x, u.x, SEL_HI),
                                       __builtin_amdgcn_perm(v.y, u.y, SEL_LO), __builtin_amdgcn_perm(v.y, u.y, SEL_HI)));
      st_nt(row + 32ll * j + 16, make_uint4(__builtin_amdgcn_perm(v.z, u.z, SEL_LO), __builtin_amdgcn_perm(v.z, u.z, SEL_HI),
                                            __builtin_amdgcn_perm(v.w, u.w, SEL_LO), __builtin_amdgcn_perm(v.w, u.w, SEL_HI)));
    }
    return;
  }
  const int x = pieces * PER + (j - pieces);
  if constexpr (WB == 2) {
    uint16_t *q = (uint16_t *)row + 2 * x, *su = (uint16_t *)pu + x, *sv = (uint16_t *)pv + x;
    if constexpr (!PACK) { *su = q[0]; *sv = q[1]; } else { q[0] = *su; q[1] = *sv; }
  } else {
    uint8_t *q = row + 2 * x;
    if constexpr (!PACK) { pu[x] = q[0]; pv[x] = q[1]; } else { q[0] = pu[x]; q[1] = pv[x]; }
  }
}
} // namespace

void vc2_launch_packed(Launcher &L, const PackedParams &p, bool pack, int n_pictures, hipStream_t s) {
  if (p.rows < 1 || p.width < 1 || n_pictures < 1) return;
  long long ipr;
  if (p.v210) {
    ipr = (((p.width + 5) / 6) + 1) & ~1; // one work-item per group, an even count per row
  } else {
    const int per = 16 / p.word_bytes, pieces = p.vec ? p.width / per : 0;
    ipr = pieces + (p.width - pieces * per);
  }
  const dim3 grid((unsigned)((p.rows * ipr + 255) / 256), (unsigned)n_pictures);
  if (p.v210) {
    vc2_prof_begin(L, pack ? "v210_pack" : "v210_unpack", s);
    if (pack) VC2_LAUNCH(L, k_v210<true>, grid, dim3(256), 0, s, p);
    else VC2_LAUNCH(L, k_v210<false>, grid, dim3(256), 0, s, p);
  } else {
    vc2_prof_begin(L, pack ? "uv_interleave" : "uv_deinterleave", s);
    if (p.word_bytes == 2) {
      if (pack) VC2_LAUNCH(L, (k_uv<2, true>), grid, dim3(256), 0, s, p);
      else VC2_LAUNCH(L, (k_uv<2, false>), grid, dim3(256), 0, s, p);
    } else {
      if (pack) VC2_LAUNCH(L, (k_uv<1, true>), grid, dim3(256), 0, s, p);
      else VC2_LAUNCH(L, (k_uv<1, false>), grid, dim3(256), 0, s, p);
    }
  }
  vc2_prof_end(L, s);
}
