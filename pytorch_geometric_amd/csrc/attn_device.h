// attn_device.h — what the one-pass attention kernels share (gatv2.hip, transformer.hip): the
// lanes-per-head layout, the work items of a launch with the hub plan's chunks, the in-order merges
// of the chunks of a long row and, on the host, the choice of the lane shape and the checks and
// typed view of the entry points' handle (pygamd_csr).  gine.hip uses the items and the host part.
//
// Lane layout (wave64, one wave per row or per chunk of a long row): `lph` lanes per head, a power
// of two with H * lph <= 64; lane l serves head l / lph and the channels sub + lph * r (scalar) or
// the float4 units sub + lph * q (VEC) of that head, EPL registers per row.  A head's dot product
// is an xor-butterfly over its lph lanes, so heads that are narrower or wider than a lane's share,
// odd C and H*C < 64 all take the same code.
#pragma once
#include <math.h>

#include "common.h"

namespace pygamd {
namespace attn {

constexpr int kAttnMaxWidth = 512;
constexpr int kAttnMaxHeads = 64;

struct Lay {
  int H, C, lph, h, sub;
  bool head_ok;
};

__device__ __forceinline__ Lay make_lay(int H, int C, int lph) {
  Lay L;
  L.H = H;
  L.C = C;
  L.lph = lph;
  L.h = lane_id() / lph;
  L.sub = lane_id() % lph;
  L.head_ok = L.h < H;
  return L;
}

template <int EPL, bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ row, const Lay& L,
                                         float (&v)[EPL]) {
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < EPL / 4; ++q) {
      const int c = (L.sub + L.lph * q) * 4;
      if (L.head_ok && c < L.C) {
        const Vec<4> t = load_vec<4>(row + L.h * L.C + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[4 * q + i] = t.v[i];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[4 * q + i] = 0.f;
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < EPL; ++r) {
      const int c = L.sub + L.lph * r;
      v[r] = (L.head_ok && c < L.C) ? row[L.h * L.C + c] : 0.f;
    }
  }
}

template <int EPL, bool VEC>
__device__ __forceinline__ void store_row(float* __restrict__ row, const Lay& L,
                                          const float (&v)[EPL]) {
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < EPL / 4; ++q) {
      const int c = (L.sub + L.lph * q) * 4;
      if (L.head_ok && c < L.C) {
        Vec<4> t;
#pragma unroll
        for (int i = 0; i < 4; ++i) t.v[i] = v[4 * q + i];
        store_vec<4>(row + L.h * L.C + c, t);
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < EPL; ++r) {
      const int c = L.sub + L.lph * r;
      if (L.head_ok && c < L.C) row[L.h * L.C + c] = v[r];
    }
  }
}

// sum over the lph lanes of a head; every lane of the group gets the total
__device__ __forceinline__ float group_sum(float v, int lph) {
  for (int o = lph >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// ---- the online softmax -------------------------------------------------------------------------
// A running (maximum m, sum l, weighted sum acc) takes in a score p, or a chunk's (m_c, l_c, acc_c),
// as   mn = fmaxf(m, p);  l = l * exp(m - mn) + exp(p - mn)   (acc like l).
// Both factors are exp(-inf - -inf) = NaN while nothing finite has been seen: a masked score
// (p = -inf) ahead of the first finite one, or a fully masked first chunk, would poison the row.
// A side that is -inf has weight exactly 0 — which is also what expf gives whenever the other side
// is finite, so for finite scores nothing changes, bit for bit.  NaN and +inf scores still reach l
// through the other factor and poison their own (row, head), as the reference's softmax does.
__device__ __forceinline__ float softmax_weight(float x, float mn) {
  return x == -INFINITY ? 0.f : expf(x - mn);
}

// 1 / (l + 1e-16) of a finished row; NaN for a row with slots whose every score is -inf (m is still
// -inf: l and acc are 0), the reference's exp(-inf - -inf).  A row without slots keeps out = 0.
__device__ __forceinline__ float softmax_inv(float m, float l, bool has_slots) {
  return (has_slots && m == -INFINITY) ? NAN : 1.f / (l + 1e-16f);
}

// ---- edge features (transformer.hip's edge variant) -----------------------------------------------
// The lane that serves head h, sub-lane `sub` additionally owns the edge features d = sub + lph * r,
// r < kEdgeRegs, of that head: a fixed register capacity with predication, so De <= kEdgeRegs * lph.
constexpr int kEdgeRegs = 4;

// `row` holds De floats: a slot's raw features (every head reads the same line) or one head's block
// of a per-destination [H, De] row
__device__ __forceinline__ void load_edge(const float* __restrict__ row, const Lay& L, int De,
                                          float (&v)[kEdgeRegs]) {
#pragma unroll
  for (int r = 0; r < kEdgeRegs; ++r) {
    const int d = L.sub + L.lph * r;
    v[r] = (L.head_ok && d < De) ? row[d] : 0.f;
  }
}

__device__ __forceinline__ void store_edge(float* __restrict__ row, const Lay& L, int De,
                                           const float (&v)[kEdgeRegs]) {
#pragma unroll
  for (int r = 0; r < kEdgeRegs; ++r) {
    const int d = L.sub + L.lph * r;
    if (L.head_ok && d < De) row[d] = v[r];
  }
}

// sum over the heads, i.e. across the lane groups of a wave: lanes with equal `sub` are combined by
// an xor-butterfly over the lane offsets lph, 2 * lph, ...; every lane gets the total
__device__ __forceinline__ float head_sum(float v, int lph) {
  for (int o = lph; o < kWave; o <<= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// Work items of a launch: the chunks of the hub rows first (they are the long ones), then every
// row; a hub row's own item does nothing.
template <typename IdxT>
struct Items {
  const IdxT* rowptr;
  const IdxT* hub_rows;
  const IdxT* hub_cptr;
  int64_t n_rows, n_hub, n_chunks, threshold, chunk;
};

struct Span {
  int64_t row, k0, k1, row_start, row_end, chunk_id;  // chunk_id < 0: a whole row
  int64_t hub;                                        // a chunk's row as an index into hub_rows
};

template <typename IdxT>
__device__ __forceinline__ bool decode(const Items<IdxT>& it, int64_t item, Span& s) {
  if (item < it.n_chunks) {
    int64_t lo = 0, hi = it.n_hub - 1;  // last hub row whose first chunk is <= item
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (static_cast<int64_t>(it.hub_cptr[mid]) <= item) lo = mid; else hi = mid - 1;
    }
    s.row = static_cast<int64_t>(it.hub_rows[lo]);
    s.row_start = static_cast<int64_t>(it.rowptr[s.row]);
    s.row_end = static_cast<int64_t>(it.rowptr[s.row + 1]);
    s.k0 = s.row_start + (item - static_cast<int64_t>(it.hub_cptr[lo])) * it.chunk;
    s.k1 = s.k0 + it.chunk < s.row_end ? s.k0 + it.chunk : s.row_end;
    s.chunk_id = item;
    s.hub = lo;
    return s.k0 < s.row_end;
  }
  s.row = item - it.n_chunks;
  if (s.row >= it.n_rows) return false;
  s.row_start = s.k0 = static_cast<int64_t>(it.rowptr[s.row]);
  s.row_end = s.k1 = static_cast<int64_t>(it.rowptr[s.row + 1]);
  s.chunk_id = s.hub = -1;
  return !(it.n_hub > 0 && s.row_end - s.row_start > it.threshold);
}

// The forward merge of hub row `hr`, for one 64-lane workgroup: the chunks' partials
// (acc [W], m [H], l [H]) at stride W + 2H combined IN CHUNK ORDER into the final (m, l) per head,
// the columns [col0, col1) of the output row (out may be NULL) and the row's alpha (raw scores in,
// coefficients out; left alone unless rescale_alpha).  stats != NULL: (m [H], 1 / (l + 1e-16) [H])
// go to stats + hr * 2H, for a launch that rescales the alpha of all chunks in parallel.
template <typename IdxT>
__device__ __forceinline__ void merge_softmax_row(const IdxT* __restrict__ rowptr,
                                                  const IdxT* __restrict__ hub_rows,
                                                  const IdxT* __restrict__ hub_cptr, int64_t hr,
                                                  int H, int C, const float* __restrict__ part,
                                                  float* __restrict__ alpha,
                                                  float* __restrict__ out, float* sm,
                                                  float* sinv, int64_t col0, int64_t col1,
                                                  bool rescale_alpha,
                                                  float* __restrict__ stats) {
  const int64_t row = static_cast<int64_t>(hub_rows[hr]);
  const int64_t c0 = static_cast<int64_t>(hub_cptr[hr]), c1 = static_cast<int64_t>(hub_cptr[hr + 1]);
  const int64_t W = static_cast<int64_t>(H) * C, S = W + 2 * H;
  const int lane = threadIdx.x;
  if (lane < H) {
    float m = -INFINITY, l = 0.f;
    for (int64_t c = c0; c < c1; ++c) {
      const float mc = part[c * S + W + lane], lc = part[c * S + W + H + lane];
      const float mn = fmaxf(m, mc);
      l = l * softmax_weight(m, mn) + lc * softmax_weight(mc, mn);
      m = mn;
    }
    sm[lane] = m;
    sinv[lane] = softmax_inv(m, l, true);  // (a hub row has slots)
  }
  __syncthreads();
  if (out) {
    for (int64_t t = col0 + lane; t < col1; t += kWave) {
      const int h = static_cast<int>(t / C);
      float acc = 0.f;
      for (int64_t c = c0; c < c1; ++c)
        acc = fmaf(part[c * S + t], expf(part[c * S + W + h] - sm[h]), acc);
      out[row * W + t] = acc * sinv[h];
    }
  }
  if (stats && lane < H) {
    stats[hr * 2 * H + lane] = sm[lane];
    stats[hr * 2 * H + H + lane] = sinv[lane];
  }
  if (!rescale_alpha) return;
  const int64_t k0 = static_cast<int64_t>(rowptr[row]) * H;
  const int64_t k1 = static_cast<int64_t>(rowptr[row + 1]) * H;
  for (int64_t t = k0 + lane; t < k1; t += kWave) {
    const int h = static_cast<int>(t % H);
    alpha[t] = expf(alpha[t] - sm[h]) * sinv[h];
  }
}

// partial rows of hub row `hr` (W floats at stride ld_part per chunk) summed in chunk order into
// row `row` of dst (stride ld_dst)
template <typename IdxT>
__device__ __forceinline__ void merge_sum_row(const IdxT* __restrict__ hub_rows,
                                              const IdxT* __restrict__ hub_cptr, int64_t hr,
                                              int64_t W, const float* __restrict__ part,
                                              int64_t ld_part, float* __restrict__ dst,
                                              int64_t ld_dst) {
  const int64_t row = static_cast<int64_t>(hub_rows[hr]);
  const int64_t c0 = static_cast<int64_t>(hub_cptr[hr]), c1 = static_cast<int64_t>(hub_cptr[hr + 1]);
  for (int64_t t = threadIdx.x; t < W; t += kWave) {
    float acc = 0.f;
    for (int64_t c = c0; c < c1; ++c) acc += part[c * ld_part + t];
    dst[row * ld_dst + t] = acc;
  }
}

// ---- host side -------------------------------------------------------------------------------
struct Shape {
  int lph, epl;
  bool vec;
};

inline bool choose_shape(int64_t H, int64_t C, bool aligned, Shape* s) {
  if (H < 1 || C < 1 || H * C > kAttnMaxWidth || H > kAttnMaxHeads) return false;
  int cap = 1;
  while (cap * 2 * H <= kWave) cap *= 2;
  if (aligned && C % 4 == 0) {
    const int units = static_cast<int>(C / 4);
    int lph = cap;
    while (lph > 1 && lph / 2 >= units) lph /= 2;
    const int n = (units + lph - 1) / lph;
    if (n <= 2) {
      *s = Shape{lph, 4 * n, true};
      return true;
    }
  }
  int lph = cap;
  while (lph > 1 && lph / 2 >= C) lph /= 2;
  const int n = static_cast<int>((C + lph - 1) / lph);
  int epl = 1;
  while (epl < n) epl *= 2;
  if (epl > 16) return false;
  *s = Shape{lph, epl, false};
  return true;
}

// The lane shape of the edge variant: the shape of (H, C) with lph widened (idle lanes for the row)
// until kEdgeRegs * lph >= De.  Whether one exists does not depend on `aligned`.
inline bool choose_shape_edge(int64_t H, int64_t C, int64_t De, bool aligned, Shape* s) {
  if (De < 1 || !choose_shape(H, C, aligned, s)) return false;
  int lph = s->lph;
  while (kEdgeRegs * lph < De && lph * 2 * H <= kWave) lph *= 2;
  if (kEdgeRegs * lph < De) return false;
  if (lph != s->lph) {
    const int n = static_cast<int>(((s->vec ? C / 4 : C) + lph - 1) / lph);
    int epl = 1;
    while (epl < n) epl *= 2;
    *s = Shape{lph, s->vec ? 4 * n : epl, s->vec};
  }
  return true;
}

#define ATTN_DISPATCH_SHAPE(shape, ...)                                 \
  do {                                                                  \
    if ((shape).vec) {                                                  \
      if ((shape).epl == 4) { constexpr int EPL = 4; constexpr bool VEC = true; __VA_ARGS__ }   \
      else { constexpr int EPL = 8; constexpr bool VEC = true; __VA_ARGS__ }                    \
    } else {                                                            \
      switch ((shape).epl) {                                            \
        case 1: { constexpr int EPL = 1; constexpr bool VEC = false; __VA_ARGS__ } break;       \
        case 2: { constexpr int EPL = 2; constexpr bool VEC = false; __VA_ARGS__ } break;       \
        case 4: { constexpr int EPL = 4; constexpr bool VEC = false; __VA_ARGS__ } break;       \
        case 8: { constexpr int EPL = 8; constexpr bool VEC = false; __VA_ARGS__ } break;       \
        default: { constexpr int EPL = 16; constexpr bool VEC = false; __VA_ARGS__ } break;     \
      }                                                                 \
    }                                                                   \
  } while (0)

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the checks every entry point shares on its handle `g`, the row count of the other side and the
// head layout; 0 = go on
inline int check_args(const pygamd_csr* g, int64_t n_other, int64_t H, int64_t C) {
  if (!g) return PYGAMD_ERR_INVALID_ARG;
  if (g->idx_dtype != PYGAMD_IDX_I64 && g->idx_dtype != PYGAMD_IDX_I32)
    return PYGAMD_ERR_INVALID_ARG;
  if (g->n_rows < 0 || n_other < 0 || H < 1 || C < 1 || g->n_hub < 0 || g->n_chunks < 0)
    return PYGAMD_ERR_INVALID_ARG;
  if (g->n_hub > 0 && (!g->hub_rows || !g->hub_chunk_ptr || g->n_chunks < g->n_hub ||
                       g->hub_threshold < 1 || g->hub_chunk < 1))
    return PYGAMD_ERR_INVALID_ARG;
  if (g->n_hub == 0 && g->n_chunks != 0) return PYGAMD_ERR_INVALID_ARG;
  if (H * C > kAttnMaxWidth || H > kAttnMaxHeads) return PYGAMD_ERR_UNSUPPORTED;
  return PYGAMD_OK;
}

// the work items of a launch over the handle, and its column array, at the handle's index type
template <typename IdxT>
inline Items<IdxT> make_items(const pygamd_csr& g) {
  return Items<IdxT>{static_cast<const IdxT*>(g.rowptr), static_cast<const IdxT*>(g.hub_rows),
                     static_cast<const IdxT*>(g.hub_chunk_ptr), g.n_rows, g.n_hub, g.n_chunks,
                     g.hub_threshold, g.hub_chunk};
}

template <typename IdxT>
inline const IdxT* typed_col(const pygamd_csr& g) {
  return static_cast<const IdxT*>(g.col);
}

}  // namespace attn
}  // namespace pygamd
