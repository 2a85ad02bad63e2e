// spline.hip — SplineConv (nn/conv/spline_conv.py:150-153 of the reference: spline_basis followed by
// spline_weighting) without the [E, S] pair tensors and without an [E, K] coefficient plane.  An
// edge with pseudo-coordinates u in [0, 1]^dim touches S = (degree + 1)^dim of the K = prod
// kernel_size weight matrices, entry s with the product of one B-spline polynomial per dimension:
//     m_e = sum_{s < S} basis[e, s] * x_j W[wi[e, s]]
// The pairs (basis, wi) are a few flops on `dim` floats, so every kernel here REBUILDS them per
// slot (lane s computes entry s, the values are broadcast from there) and the kernels are
//   collect      out[i]  = scale_i * sum_{slots} sum_s basis_s * H[j, wi_s, :] (+ root[i]) (+ bias)
//                over the by-destination handle, H = x_src @ W as ONE dense product [n_src, K * M]
//                ("transform first": a slot gathers S rows of M floats);
//   expand       GH[j, k, :] = sum_{slots of source j} sum_{s: wi_s = k} basis_s * scale_i * g[i]
//                over the by-source handle, a row's K * M bins accumulated in LDS (lane l owns the
//                columns l + 64 e of EVERY bin: adds never collide and their order is the slots');
//                grad_W and grad_x are dense products with GH;
//   pseudo_grad  grad_pseudo[e, d] = sum_s <H[j, wi_s], scale_i g[i]> * d basis_s / d u_d
//                over the by-destination handle, g[i] in registers, S dot products reduced four at
//                a time across the wave;
//   basis        the stand-alone [E, S] pair tensors for the public spline_basis().
// Work items, hub chunks and the in-order merge: rowwalk_device.h; a slot's edge id:
// gine_device.h; lane l owns the columns l + 64 e of a row (spmm_device.h's layout).  No float
// atomics and every grid depends on the problem's sizes only: results are bitwise reproducible.
//
// Index safety: whatever pseudo holds (negative, > 1, infinite, NaN), every per-dimension index is
// wrapped into [0, kernel_size[d]) non-negatively and the flat index is clamped below K, so no
// input makes a kernel read or write out of range.  NaN: bin of digit k alone, NaN basis.
#include "common.h"
#include "gine_device.h"

namespace pygamd {
namespace {

using namespace rowwalk;
using gine::slot_edge;

constexpr int kSplineMaxWidth = 512;  // F_in, F_out
constexpr int kSplineMaxS = kWave;    // one lane per entry
constexpr int kSplineMaxDim = 6;      // (degree + 1)^dim <= 64 with degree >= 1
// expand keeps a row's K * F_out bins in LDS: ONE wave per workgroup, and the workgroup's whole
// 64 KiB (what a launch gets without opting in to more) as that wave's slice
constexpr int64_t kSplineLdsBytes = 64 * 1024;
constexpr int64_t kSplineMaxBins = kSplineLdsBytes / sizeof(float);  // 16,384 = K * F_out
constexpr unsigned kSplineMaxGrid = 1u << 20;

// how an edge's pseudo-coordinates select and weight its bins
struct Bins {
  const float* pseudo;         // [E, dim]
  const int64_t* kernel_size;  // [dim]
  const uint8_t* open;         // [dim]
  int dim, degree, S;
  int64_t K;
};

// B_degree(f, k) and its derivative in f
template <bool GRAD>
__device__ __forceinline__ float bspline(int degree, int k, float f, float& df) {
  float b;
  if (degree == 1) {
    b = k == 0 ? 1.f - f : f;
    if constexpr (GRAD) df = k == 0 ? -1.f : 1.f;
  } else if (degree == 2) {
    if (k == 0) {
      b = 0.5f * f * f - f + 0.5f;
      if constexpr (GRAD) df = f - 1.f;
    } else if (k == 1) {
      b = -f * f + f + 0.5f;
      if constexpr (GRAD) df = -2.f * f + 1.f;
    } else {
      b = 0.5f * f * f;
      if constexpr (GRAD) df = f;
    }
  } else {
    const float sixth = 1.f / 6.f;
    if (k == 0) {
      const float r = 1.f - f;
      b = r * r * r * sixth;
      if constexpr (GRAD) df = -0.5f * r * r;
    } else if (k == 1) {
      b = (3.f * f * f * f - 6.f * f * f + 4.f) * sixth;
      if constexpr (GRAD) df = 1.5f * f * f - 2.f * f;
    } else if (k == 2) {
      b = (-3.f * f * f * f + 3.f * f * f + 3.f * f + 1.f) * sixth;
      if constexpr (GRAD) df = -1.5f * f * f + f + 0.5f;
    } else {
      b = f * f * f * sixth;
      if constexpr (GRAD) df = 0.5f * f * f;
    }
  }
  return b;
}

// Entry s of edge `e`: its basis value, its flat weight index in [0, K) and (GRAD) the derivative
// of the basis value by pseudo[e, d] in dv[d].  s >= S: basis 0, index 0, derivatives 0.
template <bool GRAD>
__device__ __forceinline__ void spline_entry(const Bins& B, int64_t e, int s, float& basis,
                                             int64_t& wi, float (&dv)[kSplineMaxDim]) {
  float b = 1.f, fac[kSplineMaxDim], dfac[kSplineMaxDim];
  int64_t w = 0, off = 1;
  int digits = s;
  const int base = B.degree + 1;
#pragma unroll
  for (int d = 0; d < kSplineMaxDim; ++d) {
    fac[d] = 1.f;
    dfac[d] = 0.f;
    if (d < B.dim) {
      int64_t ks = B.kernel_size[d];
      ks = ks < 1 ? 1 : ks;
      const float span = static_cast<float>(ks - (B.open[d] ? B.degree : 0));
      const float v = B.pseudo[e * B.dim + d] * span;
      const int k = digits % base;
      digits /= base;
      // (the cast is defined only inside the range; NaN fails the comparison too)
      const int64_t t = fabsf(v) < 9.0e18f ? static_cast<int64_t>(v) : 0;
      const int64_t idx = ((t + k) % ks + ks) % ks;
      float df = 0.f;
      fac[d] = bspline<GRAD>(B.degree, k, v - floorf(v), df);
      dfac[d] = df * span;
      b *= fac[d];
      w += idx * off;
      off *= ks;
    }
  }
  const bool live = s < B.S;
  basis = live ? b : 0.f;
  wi = live ? (w < B.K ? w : B.K - 1) : 0;
  if constexpr (GRAD) {
#pragma unroll
    for (int d = 0; d < kSplineMaxDim; ++d) {
      float p = dfac[d];
#pragma unroll
      for (int o = 0; o < kSplineMaxDim; ++o) p *= o == d ? 1.f : fac[o];
      dv[d] = live && d < B.dim ? p : 0.f;
    }
  }
}

// ---- basis (stand-alone) ---------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
    spline_basis_kernel(Bins B, int64_t E, float* __restrict__ basis,
                        int64_t* __restrict__ weight_index) {
  const int64_t n = E * B.S;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; t < n; t += stride) {
    float b, dv[kSplineMaxDim];
    int64_t w;
    spline_entry<false>(B, t / B.S, static_cast<int>(t % B.S), b, w, dv);
    basis[t] = b;
    weight_index[t] = w;
  }
}

// ---- collect (forward) -----------------------------------------------------------------------
constexpr int kCollectSlots = 2;  // slots in flight per wave: 2 * EPL rows of H per step

template <typename IdxT, int EPL>
__global__ void __launch_bounds__(kBlock)
    spline_collect_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                          const IdxT* __restrict__ edge_id, Bins B, const float* __restrict__ h,
                          int64_t ld_h, int F, const float* __restrict__ row_scale,
                          const float* __restrict__ root, int64_t ld_root,
                          const float* __restrict__ bias, float* __restrict__ out,
                          float* __restrict__ part) {
  constexpr int U = kCollectSlots;
  const Lay L = make_lay(1, F, kWave);
  const int lane = lane_id();
  float bv[EPL];
  if (bias) {
    load_row<EPL, false>(bias, L, bv);
  } else {
#pragma unroll
    for (int e = 0; e < EPL; ++e) bv[e] = 0.f;
  }
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    const bool whole = s.chunk_id < 0;
    float acc[EPL], rv[EPL];
    // the epilogue's root row is requested before the gathers
    if (whole && root) {
      load_row<EPL, false>(root + s.row * ld_root, L, rv);
    } else {
#pragma unroll
      for (int e = 0; e < EPL; ++e) rv[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float bs[U], dv[kSplineMaxDim];
      int wi[U];
      const float* src[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        bs[u] = 0.f;
        wi[u] = 0;
        src[u] = h;
        if (k + u < s.k1) {
          int64_t w;
          spline_entry<false>(B, slot_edge(edge_id, k + u), lane, bs[u], w, dv);
          wi[u] = static_cast<int>(w);
          src[u] = h + static_cast<int64_t>(col[k + u]) * ld_h;
        }
      }
      for (int s0 = 0; s0 < B.S; ++s0) {
        float hv[U][EPL];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (k + u < s.k1)
            load_row<EPL, false>(src[u] + static_cast<int64_t>(bcast_uniform(wi[u], s0)) * F, L,
                                 hv[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (k + u < s.k1) {
            const float b = bcast_uniform(bs[u], s0);
#pragma unroll
            for (int e = 0; e < EPL; ++e) acc[e] = fmaf(b, hv[u][e], acc[e]);
          }
        }
      }
    }
    if (whole) {
      const float sc = row_scale ? row_scale[s.row] : 1.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[e] = fmaf(acc[e], sc, rv[e] + bv[e]);
      store_row<EPL, false>(out + s.row * F, L, acc);
    } else {
      store_row<EPL, false>(part + s.chunk_id * F, L, acc);
    }
  }
}

// a split row: its chunks' partial rows in chunk order, then the epilogue once
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    spline_collect_merge_kernel(const IdxT* __restrict__ hub_rows,
                                const IdxT* __restrict__ hub_cptr, int F,
                                const float* __restrict__ part,
                                const float* __restrict__ row_scale,
                                const float* __restrict__ root, int64_t ld_root,
                                const float* __restrict__ bias, float* __restrict__ out) {
  const int64_t hr = blockIdx.x;
  const int64_t row = static_cast<int64_t>(hub_rows[hr]);
  const int64_t c0 = static_cast<int64_t>(hub_cptr[hr]), c1 = static_cast<int64_t>(hub_cptr[hr + 1]);
  const float sc = row_scale ? row_scale[row] : 1.f;
  for (int t = threadIdx.x; t < F; t += kWave) {
    float acc = 0.f;
    for (int64_t c = c0; c < c1; ++c) acc += part[c * F + t];
    const float add = (root ? root[row * ld_root + t] : 0.f) + (bias ? bias[t] : 0.f);
    out[row * F + t] = fmaf(acc, sc, add);
  }
}

// ---- expand (backward, by source) ------------------------------------------------------------
constexpr int kExpandSlots = 2;

template <typename IdxT, int EPL>
__global__ void __launch_bounds__(kWave)
    spline_expand_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                         const IdxT* __restrict__ edge_id, Bins B, const float* __restrict__ g,
                         int64_t ld_g, int F, const float* __restrict__ col_scale,
                         float* __restrict__ gh, float* __restrict__ part) {
  constexpr int U = kExpandSlots;
  extern __shared__ float bins[];  // [K, F]: this wave's (the workgroup is one wave)
  const Lay L = make_lay(1, F, kWave);
  const int lane = lane_id();
  const int W = static_cast<int>(B.K) * F;
  const int64_t n_items = it.n_chunks + it.n_rows;
  for (int64_t item = xcd_logical_block(); item < n_items; item += gridDim.x) {
    Span s;
    if (!decode(it, item, s)) continue;  // (wave-uniform: the barriers below are reached by all)
    float* dst = s.chunk_id >= 0 ? part + s.chunk_id * W : gh + s.row * W;
    if (s.k0 >= s.k1) {  // a source without slots: exact zeros, no LDS
      for (int t = lane; t < W; t += kWave) dst[t] = 0.f;
      continue;
    }
    for (int t = lane; t < W; t += kWave) bins[t] = 0.f;
    __syncthreads();
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float bs[U], gv[U][EPL], dv[kSplineMaxDim];
      int wi[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        bs[u] = 0.f;
        wi[u] = 0;
        if (k + u < s.k1) {
          const int64_t i = static_cast<int64_t>(col[k + u]);
          int64_t w;
          spline_entry<false>(B, slot_edge(edge_id, k + u), lane, bs[u], w, dv);
          wi[u] = static_cast<int>(w);
          load_row<EPL, false>(g + i * ld_g, L, gv[u]);
          const float sc = col_scale ? col_scale[i] : 1.f;
#pragma unroll
          for (int e = 0; e < EPL; ++e) gv[u][e] *= sc;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          for (int s0 = 0; s0 < B.S; ++s0) {
            float* bin = bins + bcast_uniform(wi[u], s0) * F;
            const float b = bcast_uniform(bs[u], s0);
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
              const int c = lane + kWave * e;  // this lane's column of every bin, no other's
              if (c < F) bin[c] = fmaf(b, gv[u][e], bin[c]);
            }
          }
        }
      }
    }
    __syncthreads();
    for (int t = lane; t < W; t += kWave) dst[t] = bins[t];  // the row, coalesced
    __syncthreads();
  }
}

// ---- pseudo_grad -----------------------------------------------------------------------------
// Four per-lane partial dot products reduced across the wave together, as mixture.hip's
// tile_reduce does for a tile of 4: two halving exchanges (lane bits 32 and 16), then a butterfly
// over the 16 lanes left.  Afterwards lane l holds the total of entry quad_entry(l).
__device__ __forceinline__ float quad_reduce(const float (&p)[4], int lane) {
  const bool up32 = (lane & 32) != 0, up16 = (lane & 16) != 0;
  const float q0 = (up32 ? p[2] : p[0]) + __shfl_xor(up32 ? p[0] : p[2], 32, kWave);
  const float q1 = (up32 ? p[3] : p[1]) + __shfl_xor(up32 ? p[1] : p[3], 32, kWave);
  float v = (up16 ? q1 : q0) + __shfl_xor(up16 ? q0 : q1, 16, kWave);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// a lane that holds entry t (0..3) after quad_reduce
__device__ __forceinline__ int quad_holder(int t) { return ((t & 2) ? 32 : 0) | ((t & 1) ? 16 : 0); }

template <typename IdxT, int EPL>
__global__ void __launch_bounds__(kBlock)
    spline_pseudo_grad_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                              const IdxT* __restrict__ edge_id, Bins B,
                              const float* __restrict__ h, int64_t ld_h, int F,
                              const float* __restrict__ g, int64_t ld_g,
                              const float* __restrict__ row_scale,
                              float* __restrict__ grad_pseudo) {
  const Lay L = make_lay(1, F, kWave);
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s) || s.k0 >= s.k1) continue;  // (chunks write their own edges)
    float gv[EPL];
    load_row<EPL, false>(g + s.row * ld_g, L, gv);
    const float sc = row_scale ? row_scale[s.row] : 1.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) gv[e] *= sc;
    for (int64_t k = s.k0; k < s.k1; ++k) {
      const int64_t id = slot_edge(edge_id, k);
      const float* src = h + static_cast<int64_t>(col[k]) * ld_h;
      float bs, dv[kSplineMaxDim];
      int64_t w;
      spline_entry<true>(B, id, lane, bs, w, dv);
      const int wi = static_cast<int>(w);
      float dot = 0.f;  // lane s: <H[j, wi_s], scale_i g_i>
      for (int s0 = 0; s0 < B.S; s0 += 4) {
        float hv[4][EPL], p[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (s0 + t < B.S)
            load_row<EPL, false>(src + static_cast<int64_t>(bcast_uniform(wi, s0 + t)) * F, L,
                                 hv[t]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          p[t] = 0.f;
          if (s0 + t < B.S) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) p[t] = fmaf(hv[t][e], gv[e], p[t]);
          }
        }
        const float total = quad_reduce(p, lane);
        const float mine = bcast_lane(total, quad_holder((lane - s0) & 3));
        if (lane >= s0 && lane < s0 + 4) dot = mine;
      }
      float keep = 0.f;
#pragma unroll
      for (int d = 0; d < kSplineMaxDim; ++d) {
        if (d < B.dim) {
          const float c = group_sum(dot * dv[d], kWave);  // (dv is 0 in the lanes beyond S)
          if (lane == d) keep = c;
        }
      }
      if (lane < B.dim) grad_pseudo[id * B.dim + lane] = keep;
    }
  }
}

// ---- host side -------------------------------------------------------------------------------
bool spline_envelope(int64_t F_in, int64_t F_out, int64_t K, int64_t S) {
  return F_in >= 1 && F_in <= kSplineMaxWidth && F_out >= 1 && F_out <= kSplineMaxWidth &&
         S >= 1 && S <= kSplineMaxS && K >= 1 && K * F_out <= kSplineMaxBins;
}

int spline_epl(int64_t F) {
  const int n = static_cast<int>((F + kWave - 1) / kWave);
  int epl = 1;
  while (epl < n) epl *= 2;
  return epl;
}

// `...` sees the constant EPL
#define SPLINE_DISPATCH(epl, ...)                                        \
  switch (epl) {                                                         \
    case 1: { constexpr int EPL = 1; __VA_ARGS__ } break;                \
    case 2: { constexpr int EPL = 2; __VA_ARGS__ } break;                \
    case 4: { constexpr int EPL = 4; __VA_ARGS__ } break;                \
    default: { constexpr int EPL = 8; __VA_ARGS__ } break;               \
  }

// S = (degree + 1)^dim, or 0 when (dim, degree) is outside what a wave's lanes hold
int64_t spline_entries(int64_t dim, int64_t degree) {
  if (dim < 1 || dim > kSplineMaxDim || degree < 1 || degree > 3) return 0;
  int64_t S = 1;
  for (int64_t d = 0; d < dim; ++d) S *= degree + 1;
  return S <= kSplineMaxS ? S : 0;
}

// the checks the three handle-walking entry points share; fills `B`; 0 = go on
int spline_check(const pygamd_csr* g, int64_t n_cols, const float* pseudo,
                 const int64_t* kernel_size, const void* is_open_spline, int64_t dim,
                 int64_t degree, int64_t K, int64_t F, int64_t ld, Bins* B) {
  if (F < 1 || K < 1 || dim < 1 || degree < 1) return PYGAMD_ERR_INVALID_ARG;
  const int rc = check_handle(g, n_cols);
  if (rc != PYGAMD_OK) return rc;
  const int64_t S = spline_entries(dim, degree);
  if (S == 0 || !spline_envelope(1, F, K, S)) return PYGAMD_ERR_UNSUPPORTED;
  if (ld < F) return PYGAMD_ERR_INVALID_ARG;
  *B = Bins{pseudo, kernel_size, static_cast<const uint8_t*>(is_open_spline),
            static_cast<int>(dim), static_cast<int>(degree), static_cast<int>(S), K};
  return PYGAMD_OK;
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_spline_supported(int64_t F_in, int64_t F_out, int64_t K, int64_t S) {
  return spline_envelope(F_in, F_out, K, S) ? 1 : 0;
}

int pygamd_spline_workspace_size(int64_t n_chunks, int64_t F_out, int64_t K, size_t* bytes) {
  if (!bytes || n_chunks < 0 || F_out < 1 || K < 1) return PYGAMD_ERR_INVALID_ARG;
  if (!spline_envelope(1, F_out, K, 1)) return PYGAMD_ERR_UNSUPPORTED;
  *bytes = sizeof(float) * static_cast<size_t>(n_chunks * K * F_out);  // a chunk's partial row
  return PYGAMD_OK;
}

int pygamd_spline_basis(const float* pseudo, const int64_t* kernel_size,
                        const void* is_open_spline, int64_t E, int64_t dim, int64_t degree,
                        int64_t K, float* basis, int64_t* weight_index, void* stream) {
  if (E < 0 || K < 1 || dim < 1 || degree < 1) return PYGAMD_ERR_INVALID_ARG;
  const int64_t S = spline_entries(dim, degree);
  if (S == 0) return PYGAMD_ERR_UNSUPPORTED;
  if (E == 0) return PYGAMD_OK;
  if (!pseudo || !kernel_size || !is_open_spline || !basis || !weight_index)
    return PYGAMD_ERR_INVALID_ARG;
  const Bins B{pseudo, kernel_size, static_cast<const uint8_t*>(is_open_spline),
               static_cast<int>(dim), static_cast<int>(degree), static_cast<int>(S), K};
  const int64_t blocks = ceil_div(E * S, kBlock);
  const dim3 grid(static_cast<unsigned>(blocks < kSplineMaxGrid ? blocks : kSplineMaxGrid));
  hipLaunchKernelGGL(spline_basis_kernel, grid, dim3(kBlock), 0, as_stream(stream), B, E, basis,
                     weight_index);
  PYGAMD_LAUNCH_CHECK();
  return PYGAMD_OK;
}

int pygamd_spline_collect(const pygamd_csr* g, const void* edge_id, const float* pseudo,
                          const int64_t* kernel_size, const void* is_open_spline, int64_t dim,
                          int64_t degree, int64_t K, const float* h, int64_t ld_h, int64_t n_cols,
                          int64_t F_out, const float* row_scale, const float* root,
                          int64_t ld_root, const float* bias, float* out, void* workspace,
                          size_t workspace_bytes, void* stream) {
  Bins B;
  const int rc = spline_check(g, n_cols, pseudo, kernel_size, is_open_spline, dim, degree, K,
                              F_out, F_out, &B);
  if (rc != PYGAMD_OK) return rc;
  if (ld_h < K * F_out || (root && ld_root < F_out)) return PYGAMD_ERR_INVALID_ARG;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !h || !pseudo || !kernel_size || !is_open_spline || !out)
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < sizeof(float) * n_chunks * F_out))
    return PYGAMD_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const int F = static_cast<int>(F_out);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    SPLINE_DISPATCH(spline_epl(F_out), {
      hipLaunchKernelGGL((spline_collect_kernel<IdxT, EPL>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), B, h, ld_h, F,
                         row_scale, root, ld_root, bias, out, part);
    });
    PYGAMD_LAUNCH_CHECK();
    if (it.n_hub > 0) {
      hipLaunchKernelGGL((spline_collect_merge_kernel<IdxT>),
                         dim3(static_cast<unsigned>(it.n_hub)), dim3(kWave), 0, st, it.hub_rows,
                         it.hub_cptr, F, part, row_scale, root, ld_root, bias, out);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

int pygamd_spline_expand(const pygamd_csr* g, const void* edge_id, const float* pseudo,
                         const int64_t* kernel_size, const void* is_open_spline, int64_t dim,
                         int64_t degree, int64_t K, const float* grad_out, int64_t ld_g,
                         int64_t n_cols, int64_t F_out, const float* col_scale, float* gh,
                         void* workspace, size_t workspace_bytes, void* stream) {
  Bins B;
  const int rc = spline_check(g, n_cols, pseudo, kernel_size, is_open_spline, dim, degree, K,
                              F_out, ld_g, &B);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !grad_out || !pseudo || !kernel_size || !is_open_spline || !gh)
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < sizeof(float) * n_chunks * K * F_out))
    return PYGAMD_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const int F = static_cast<int>(F_out);
  const size_t lds = sizeof(float) * static_cast<size_t>(K * F_out);  // <= kSplineLdsBytes
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const int64_t blocks = round_up(n_rows + n_chunks, 8);  // one wave, one item at a time
    const dim3 grid(static_cast<unsigned>(blocks < kSplineMaxGrid ? blocks : kSplineMaxGrid));
    SPLINE_DISPATCH(spline_epl(F_out), {
      hipLaunchKernelGGL((spline_expand_kernel<IdxT, EPL>), grid, dim3(kWave), lds, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), B, grad_out,
                         ld_g, F, col_scale, gh, part);
    });
    PYGAMD_LAUNCH_CHECK();
    // (hub rows: the chunks' partial rows in chunk order)
    return launch_sum_merge(it, K * F_out, part, gh, st);
  });
}

int pygamd_spline_pseudo_grad(const pygamd_csr* g, const void* edge_id, const float* pseudo,
                              const int64_t* kernel_size, const void* is_open_spline,
                              int64_t dim, int64_t degree, int64_t K, const float* h,
                              int64_t ld_h, int64_t n_cols, int64_t F_out, const float* grad_out,
                              int64_t ld_g, const float* row_scale, float* grad_pseudo,
                              void* stream) {
  Bins B;
  const int rc = spline_check(g, n_cols, pseudo, kernel_size, is_open_spline, dim, degree, K,
                              F_out, ld_g, &B);
  if (rc != PYGAMD_OK) return rc;
  if (ld_h < K * F_out) return PYGAMD_ERR_INVALID_ARG;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !h || !grad_out || !pseudo || !kernel_size || !is_open_spline ||
      !grad_pseudo)
    return PYGAMD_ERR_INVALID_ARG;
  hipStream_t st = as_stream(stream);
  const int F = static_cast<int>(F_out);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    SPLINE_DISPATCH(spline_epl(F_out), {
      hipLaunchKernelGGL((spline_pseudo_grad_kernel<IdxT, EPL>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), B, h, ld_h, F,
                         grad_out, ld_g, row_scale, grad_pseudo);
    });
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

}  // extern "C"
