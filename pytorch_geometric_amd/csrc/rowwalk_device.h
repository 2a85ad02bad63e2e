// rowwalk_device.h — the base layer of every kernel that walks the rows of a sorted handle
// (pygamd_csr); nothing here knows what a kernel computes.  Device side: the lanes-per-head layout
// of a row in registers, the work items of a launch with the hub plan's chunks and a wave's walk
// over them, the in-order sum merge of a long row's chunks, and the two helper kernels that need
// nothing else (that merge; the reduce of per-workgroup parameter partials).  Host side: the lane
// shape and its dispatch, the checks and typed views of the entry points' handle, the launches of
// the two kernels.  Included by attn_device.h and gine_device.h, through which every kernel file
// that includes one of them has it, and alone by graph_norm.hip.
//
// Lane layout (wave64, one wave per row or per chunk of a long row): `lph` lanes per head, a power
// of two with H * lph <= 64; lane l serves head l / lph and the channels sub + lph * r (scalar) or
// the float4 units sub + lph * q (VEC) of that head, EPL registers per row.  A head's dot product
// is an xor-butterfly over its lph lanes, so heads that are narrower or wider than a lane's share,
// odd C and H*C < 64 all take the same code.  Kernels without heads use H = 1, C = the row width.
#pragma once
#include "common.h"

namespace pygamd {
namespace rowwalk {

constexpr int kMaxWidth = 512;  // floats of a row (H * C) that the lane shapes cover

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

// the column of register e of this lane
template <bool VEC>
__device__ __forceinline__ int lane_col(const Lay& L, int e) {
  if constexpr (VEC) return (L.sub + L.lph * (e >> 2)) * 4 + (e & 3);
  return L.sub + L.lph * e;
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

// the items of a wave: for (item = wk.first; item < wk.n; item += wk.stride)
struct Walk {
  int64_t n, stride, first;
};

template <typename IdxT>
__device__ __forceinline__ Walk item_walk(const Items<IdxT>& it) {
  return Walk{it.n_chunks + it.n_rows, static_cast<int64_t>(gridDim.x) * kWavesPerBlock,
              xcd_logical_block() * kWavesPerBlock + wave_in_block()};
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

// (the two kernels are static: every file that launches them carries its own copy)
// hub rows: the chunks' partial rows summed in chunk order
template <typename IdxT>
static __global__ void __launch_bounds__(kWave)
    sum_merge_kernel(const IdxT* __restrict__ hub_rows, const IdxT* __restrict__ hub_cptr,
                     int64_t F, const float* __restrict__ part, float* __restrict__ grad_x) {
  merge_sum_row(hub_rows, hub_cptr, static_cast<int64_t>(blockIdx.x), F, part, F, grad_x, F);
}

// the workgroups' partials (grad_W [FD], then grad_b [F]; F = 0: no bias block) summed in
// workgroup order
static __global__ void __launch_bounds__(kBlock)
    param_reduce_kernel(const float* __restrict__ wpart, int n_blocks, int FD, int F,
                        float* __restrict__ grad_weight, float* __restrict__ grad_bias) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const int S = FD + F;
  if (t >= S) return;
  float acc = 0.f;
  for (int g = 0; g < n_blocks; ++g) acc += wpart[static_cast<int64_t>(g) * S + t];
  if (t < FD) {
    grad_weight[t] = acc;
  } else if (grad_bias) {
    grad_bias[t - FD] = acc;
  }
}

// ---- host side -------------------------------------------------------------------------------
struct Shape {
  int lph, epl;
  bool vec;
};

inline bool choose_shape(int64_t H, int64_t C, bool aligned, Shape* s) {
  if (H < 1 || C < 1 || H * C > kMaxWidth || H > kWave) return false;  // (a head has a lane)
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

#define ROWWALK_DISPATCH_SHAPE(shape, ...)                              \
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

// the checks every entry point shares on its handle `g` and the row count of the other side;
// 0 = go on
inline int check_handle(const pygamd_csr* g, int64_t n_other) {
  if (!g) return PYGAMD_ERR_INVALID_ARG;
  if (g->idx_dtype != PYGAMD_IDX_I64 && g->idx_dtype != PYGAMD_IDX_I32)
    return PYGAMD_ERR_INVALID_ARG;
  if (g->n_rows < 0 || n_other < 0 || g->n_hub < 0 || g->n_chunks < 0)
    return PYGAMD_ERR_INVALID_ARG;
  if (g->n_hub > 0 && (!g->hub_rows || !g->hub_chunk_ptr || g->n_chunks < g->n_hub ||
                       g->hub_threshold < 1 || g->hub_chunk < 1))
    return PYGAMD_ERR_INVALID_ARG;
  if (g->n_hub == 0 && g->n_chunks != 0) return PYGAMD_ERR_INVALID_ARG;
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

// after a main launch: the hub rows' chunks (partial rows of W floats in `part`) into rows of dst
template <typename IdxT>
inline int launch_sum_merge(const Items<IdxT>& it, int64_t W, const float* part, float* dst,
                            hipStream_t st) {
  if (it.n_hub > 0) {
    hipLaunchKernelGGL((sum_merge_kernel<IdxT>), dim3(static_cast<unsigned>(it.n_hub)),
                       dim3(kWave), 0, st, it.hub_rows, it.hub_cptr, W, part, dst);
    PYGAMD_LAUNCH_CHECK();
  }
  return PYGAMD_OK;
}

// after a main launch of n_blocks workgroups: their partials into the gradients (F = 0: no bias)
inline int launch_param_reduce(const float* wpart, unsigned n_blocks, int FD, int F,
                               float* grad_weight, float* grad_bias, hipStream_t st) {
  hipLaunchKernelGGL(param_reduce_kernel, dim3(static_cast<unsigned>(ceil_div(FD + F, kBlock))),
                     dim3(kBlock), 0, st, wpart, static_cast<int>(n_blocks), FD, F, grad_weight,
                     grad_bias);
  PYGAMD_LAUNCH_CHECK();
  return PYGAMD_OK;
}

}  // namespace rowwalk
}  // namespace pygamd
