// mixture.hip — the aggregate-first half of the layers whose message is a per-edge mixture of K
// linear maps: GMMConv (nn/conv/gmm_conv.py:154-165 of the reference, m_e = sum_k w_k(e) (x_j G_k))
// and NNConv (nn/conv/nn_conv.py:119-122, m_e = x_j reshape(nn(e))).  With per-edge coefficients
// c[e, k] both are
//     Z[i, k, :] = sum_{slots s of i} c[edge_id[s], k] * x[col[s], :]         ("expand", this file)
//     out[i, :]  = Z[i].reshape(K F) @ W                                      (one dense product)
// so a slot gathers ONE narrow row of F floats and everything wide (K F) is per node.  The same
// expand over the transposed handle with x := grad_out gives grad_x's wide plane, and
//     grad_c[edge_id[s], k] = <wide[i, k F : (k + 1) F], x[col[s], :]>         ("coef_grad")
// with wide = grad_out @ W^T, the destination's own row in registers.
//
// One 64-lane wave per row (or per chunk of a row over the hub threshold), lane l owns the columns
// l + 64 e, e < EPL.  k runs in compile-time tiles of KT (KT * EPL <= 32 registers) so that the
// accumulators are named registers; a row's slots are walked once per tile and the repeated x rows
// are L2 hits.  The coefficients of a slot and tile are loaded by the first KT lanes once and
// broadcast from there.  Work items, hub chunks and the in-order merge: rowwalk_device.h; a slot's
// edge id: gine_device.h.  No float atomics and every grid depends on the problem's sizes only:
// every result is bitwise reproducible.
#include "common.h"
#include "gine_device.h"

namespace pygamd {
namespace {

using namespace rowwalk;
using gine::slot_edge;

constexpr int kMixMaxWidth = 512;  // F
constexpr int kMixMaxK = 256;      // K
constexpr int kMixRegs = 32;       // KT * EPL: a tile's accumulators (expand) or wide values (coef_grad)

template <int EPL>
struct MixSlots {  // slots in flight per wave
  static constexpr int expand = EPL >= 4 ? 2 : 4;
  static constexpr int coef = 2;
};

// ---- expand ----------------------------------------------------------------------------------
template <typename IdxT, int EPL, int KT>
__global__ void __launch_bounds__(kBlock)
    mixture_expand_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                          const IdxT* __restrict__ edge_id, const float* __restrict__ x,
                          int64_t ld_x, const float* __restrict__ coef, int F, int K,
                          float* __restrict__ z, float* __restrict__ part) {
  constexpr int U = MixSlots<EPL>::expand;
  const Lay L = make_lay(1, F, kWave);
  const int lane = lane_id();
  const int64_t W = static_cast<int64_t>(K) * F;
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float* dst = s.chunk_id >= 0 ? part + s.chunk_id * W : z + s.row * W;
    for (int k0 = 0; k0 < K; k0 += KT) {
      float acc[KT][EPL];
#pragma unroll
      for (int t = 0; t < KT; ++t) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[t][e] = 0.f;
      }
      const bool mine = lane < KT && k0 + lane < K;  // this lane fetches coefficient k0 + lane
      for (int64_t k = s.k0; k < s.k1; k += U) {
        float xv[U][EPL], cv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (k + u < s.k1) {
            load_row<EPL, false>(x + static_cast<int64_t>(col[k + u]) * ld_x, L, xv[u]);
            cv[u] = mine ? coef[slot_edge(edge_id, k + u) * K + k0 + lane] : 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (k + u < s.k1) {
#pragma unroll
            for (int t = 0; t < KT; ++t) {
              const float c = bcast_uniform(cv[u], t);
#pragma unroll
              for (int e = 0; e < EPL; ++e) acc[t][e] = fmaf(c, xv[u][e], acc[t][e]);
            }
          }
        }
      }
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        if (k0 + t < K) store_row<EPL, false>(dst + static_cast<int64_t>(k0 + t) * F, L, acc[t]);
      }
    }
  }
}

// ---- coef_grad -------------------------------------------------------------------------------
// The KT per-lane partial dot products of a slot are reduced across the wave TOGETHER: log2(KT)
// halving steps (a lane keeps one half of its values and hands the other to its partner across
// lane bit 32, 16, ...: KT - 1 exchanges), then a butterfly of the one value left over the
// remaining lane bits.  Afterwards every lane holds the total of tile entry mix_lane_k(lane).
// (H and BIT are template constants: every index into p is then a compile-time one; with H a loop
// variable the compiler selected among all of p's registers per access)
template <int H, int BIT, int KT>
__device__ __forceinline__ void tile_halve(float (&p)[KT], int lane) {
  if constexpr (H >= 1) {
    const bool upper = (lane & BIT) != 0;
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const float send = upper ? p[i] : p[i + H];
      const float keep = upper ? p[i + H] : p[i];
      p[i] = keep + __shfl_xor(send, BIT, kWave);
    }
    tile_halve<H / 2, BIT / 2, KT>(p, lane);
  }
}

template <int KT>
__device__ __forceinline__ float tile_reduce(float (&p)[KT], int lane) {
  tile_halve<KT / 2, kWave / 2, KT>(p, lane);
  float v = p[0];
#pragma unroll
  for (int o = kWave / 2 / KT; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// the tile entry whose total tile_reduce leaves in this lane
template <int KT>
__device__ __forceinline__ int mix_lane_k(int lane) {
  int k = 0, bit = kWave / 2;
#pragma unroll
  for (int h = KT / 2; h >= 1; h >>= 1, bit >>= 1) k += (lane & bit) ? h : 0;
  return k;
}

template <typename IdxT, int EPL, int KT>
__global__ void __launch_bounds__(kBlock)
    mixture_coef_grad_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                             const IdxT* __restrict__ edge_id, const float* __restrict__ wide,
                             const float* __restrict__ x, int64_t ld_x, int F, int K,
                             float* __restrict__ grad_coef) {
  constexpr int U = MixSlots<EPL>::coef;
  const Lay L = make_lay(1, F, kWave);
  const int lane = lane_id();
  const int64_t W = static_cast<int64_t>(K) * F;
  const int my_k = mix_lane_k<KT>(lane);
  const bool writer = (lane & (kWave / KT - 1)) == 0;  // one lane per tile entry
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s) || s.k0 >= s.k1) continue;  // (a row without slots loads nothing)
    const float* wrow = wide + s.row * W;
    for (int k0 = 0; k0 < K; k0 += KT) {
      float w[KT][EPL];
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        if (k0 + t < K) {
          load_row<EPL, false>(wrow + static_cast<int64_t>(k0 + t) * F, L, w[t]);
        } else {
#pragma unroll
          for (int e = 0; e < EPL; ++e) w[t][e] = 0.f;
        }
      }
      const bool mine = writer && k0 + my_k < K;
      for (int64_t k = s.k0; k < s.k1; k += U) {
        float xv[U][EPL];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (k + u < s.k1)
            load_row<EPL, false>(x + static_cast<int64_t>(col[k + u]) * ld_x, L, xv[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (k + u < s.k1) {
            float p[KT];
#pragma unroll
            for (int t = 0; t < KT; ++t) {
              p[t] = 0.f;
#pragma unroll
              for (int e = 0; e < EPL; ++e) p[t] = fmaf(w[t][e], xv[u][e], p[t]);
            }
            const float total = tile_reduce<KT>(p, lane);
            if (mine) grad_coef[slot_edge(edge_id, k + u) * K + k0 + my_k] = total;
          }
        }
      }
    }
  }
}

// ---- host side -------------------------------------------------------------------------------
bool mix_envelope(int64_t F, int64_t K) {
  return F >= 1 && F <= kMixMaxWidth && K >= 1 && K <= kMixMaxK;
}

struct MixShape {
  int epl, kt;
};

MixShape mix_shape(int64_t F, int64_t K) {
  const int n = static_cast<int>((F + kWave - 1) / kWave);
  int epl = 1;
  while (epl < n) epl *= 2;
  int kt = 1;
  while (kt < K && kt * 2 * epl <= kMixRegs) kt *= 2;
  return MixShape{epl, kt};
}

// `...` sees the constants EPL and KT of the shape
#define MIX_CASE(epl_, kt_, ...)                          \
  if (sh.epl == epl_ && sh.kt == kt_) {                   \
    constexpr int EPL = epl_; constexpr int KT = kt_;     \
    __VA_ARGS__                                           \
  } else

#define MIX_DISPATCH(...)                                                                 \
  do {                                                                                    \
    MIX_CASE(1, 1, __VA_ARGS__) MIX_CASE(1, 2, __VA_ARGS__) MIX_CASE(1, 4, __VA_ARGS__)   \
    MIX_CASE(1, 8, __VA_ARGS__) MIX_CASE(1, 16, __VA_ARGS__) MIX_CASE(1, 32, __VA_ARGS__) \
    MIX_CASE(2, 1, __VA_ARGS__) MIX_CASE(2, 2, __VA_ARGS__) MIX_CASE(2, 4, __VA_ARGS__)   \
    MIX_CASE(2, 8, __VA_ARGS__) MIX_CASE(2, 16, __VA_ARGS__)                              \
    MIX_CASE(4, 1, __VA_ARGS__) MIX_CASE(4, 2, __VA_ARGS__) MIX_CASE(4, 4, __VA_ARGS__)   \
    MIX_CASE(4, 8, __VA_ARGS__)                                                           \
    MIX_CASE(8, 1, __VA_ARGS__) MIX_CASE(8, 2, __VA_ARGS__) MIX_CASE(8, 4, __VA_ARGS__)   \
    { return PYGAMD_ERR_UNSUPPORTED; }                                                    \
  } while (0)

// the checks both entry points share; 0 = go on
int mix_check(const pygamd_csr* g, int64_t n_cols, int64_t F, int64_t K, int64_t ld_x) {
  if (F < 1 || K < 1) return PYGAMD_ERR_INVALID_ARG;
  const int rc = check_handle(g, n_cols);
  if (rc != PYGAMD_OK) return rc;
  if (!mix_envelope(F, K)) return PYGAMD_ERR_UNSUPPORTED;
  return ld_x < F ? PYGAMD_ERR_INVALID_ARG : PYGAMD_OK;
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_mixture_supported(int64_t F, int64_t K) { return mix_envelope(F, K) ? 1 : 0; }

int pygamd_mixture_workspace_bytes(int64_t n_chunks, int64_t F, int64_t K, size_t* bytes) {
  if (!bytes || n_chunks < 0 || F < 1 || K < 1) return PYGAMD_ERR_INVALID_ARG;
  if (!mix_envelope(F, K)) return PYGAMD_ERR_UNSUPPORTED;
  *bytes = sizeof(float) * static_cast<size_t>(n_chunks * K * F);  // a chunk's partial wide row
  return PYGAMD_OK;
}

int pygamd_mixture_expand(const pygamd_csr* g, const void* edge_id, const float* x, int64_t ld_x,
                          const float* coef, int64_t n_cols, int64_t F, int64_t K, float* z,
                          void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = mix_check(g, n_cols, F, K, ld_x);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !x || !coef || !z) return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < sizeof(float) * n_chunks * K * F))
    return PYGAMD_ERR_WORKSPACE;
  const MixShape sh = mix_shape(F, K);
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    MIX_DISPATCH({
      hipLaunchKernelGGL((mixture_expand_kernel<IdxT, EPL, KT>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), x, ld_x, coef,
                         static_cast<int>(F), static_cast<int>(K), z, part);
    });
    PYGAMD_LAUNCH_CHECK();
    // (hub rows: the chunks' partial wide rows in chunk order)
    return launch_sum_merge(it, K * F, part, z, st);
  });
}

int pygamd_mixture_coef_grad(const pygamd_csr* g, const void* edge_id, const float* wide,
                             const float* x, int64_t ld_x, int64_t n_cols, int64_t F, int64_t K,
                             float* grad_coef, void* stream) {
  const int rc = mix_check(g, n_cols, F, K, ld_x);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;  // (chunks write their own edges)
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !wide || !x || !grad_coef) return PYGAMD_ERR_INVALID_ARG;
  const MixShape sh = mix_shape(F, K);
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    MIX_DISPATCH({
      hipLaunchKernelGGL((mixture_coef_grad_kernel<IdxT, EPL, KT>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), wide, x, ld_x,
                         static_cast<int>(F), static_cast<int>(K), grad_coef);
    });
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

}  // extern "C"
