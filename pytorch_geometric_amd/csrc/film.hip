// film.hip — the R propagate steps of FiLMConv (nn/conv/film_conv.py:128-161 of the reference: one
// masked propagate per relation, its message at 157-161) as row-gather kernels on sorted handles,
// ONE launch forward and two backward whatever R is.  For destination i, slot k with source
// j = col[k], edge e = edge_id[k] and relation r = rel[e]:
//     pre_k    = fmaf(gamma_{r,i}, H[j, rF:(r+1)F], beta_{r,i})
//     out[i,:] = residual[i,:] + sum_k scale[e] * act(pre_k)
// H [N_src, R F] and G [N_dst, R 2F] (block r = [beta_r | gamma_r]) are node-level projections (the
// algebra: include/pyg_amd.h).  A slot gathers ONE F-wide row of H; the lane's [beta | gamma] stay
// in registers and are loaded again only when a slot's relation differs from the slot before it:
// any in-row order is correct, a row grouped by relation reloads once per relation present.
// act_mode 0 is the identity, 1 is ReLU (pre > 0 ? pre : 0, derivative pre > 0).  Nothing is
// saved: the backward recomputes the activation's mask from the inputs.
//
// Backward, with g = grad_out[i,:] and gm = g * act'(pre):
//   by destination (the (relation, destination) pair rows: row p is the slots of relation
//     pair_rel[p] into destination pair_node[p], col = their sources): [beta | gamma]_{r,i} and
//     g_i in registers, ONE gathered row of H per slot,
//     grad_G[i, r 2F:(r+1) 2F] = [sum gm | sum gm * h], divided by the pair row's length for mean;
//   by source (the (relation, source) pair rows of the flipped graph, col = the destinations):
//     H[j, block r] in registers, the contiguous 2F row [beta | gamma]_{r,i} and g_i gathered per
//     slot, grad_H[j, rF:(r+1)F] = sum scale[e] * g_i * act'(pre) * gamma_{r,i}.
// Pairs that do not occur are not written: the caller zero-fills both planes once.
//
// Lane layout, work items, their walk, hub chunks and in-order merges: rowwalk_device.h.  Lane
// shape, capped grid, dispatch and a slot's edge id: gine_device.h (resgated.hip's shapes without
// an edge term).  No float atomics anywhere and every grid depends on the problem's sizes only:
// every result is bitwise reproducible.
#include <math.h>

#include "common.h"
#include "gine_device.h"

namespace pygamd {
namespace {

using namespace rowwalk;
using namespace gine;

template <int EPL>
struct FilmSlots {  // slots in flight per wave (by source: three rows per slot)
  static constexpr int fwd = EPL >= 8 ? 2 : 4;
  static constexpr int dst = fwd;
  static constexpr int src = EPL >= 8 ? 1 : 2;
};

// act'(pre) as a mask: ReLU's is pre > 0 (0 at exactly 0, as torch), the identity's is 1
__device__ __forceinline__ bool act_on(int relu, float pre) { return !relu || pre > 0.f; }

// ---- forward ---------------------------------------------------------------------------------
template <typename IdxT, int EPL, bool VEC>
__global__ void __launch_bounds__(kBlock)
    film_fwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col, const IdxT* __restrict__ edge_id,
                    const int* __restrict__ rel, const float* __restrict__ H, int64_t ld_h,
                    const float* __restrict__ G, int64_t ld_gb, const float* __restrict__ scale,
                    const float* __restrict__ residual, int64_t ld_r, int relu, int F, int lph,
                    float* __restrict__ out, float* __restrict__ part) {
  constexpr int U = FilmSlots<EPL>::fwd;
  const Lay L = make_lay(1, F, lph);
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float beta[EPL], gamma[EPL], acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = beta[e] = gamma[e] = 0.f;
    int cur = -1;  // the relation whose [beta | gamma] the registers hold
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float hh[U][EPL], sc[U];
      int r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          const int64_t id = slot_edge(edge_id, k + u);
          r[u] = rel[id];
          sc[u] = scale ? scale[id] : 1.f;
          load_row<EPL, VEC>(H + static_cast<int64_t>(col[k + u]) * ld_h +
                                 static_cast<int64_t>(r[u]) * F, L, hh[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          if (r[u] != cur) {
            cur = r[u];
            const float* bg = G + s.row * ld_gb + static_cast<int64_t>(cur) * 2 * F;
            load_row<EPL, VEC>(bg, L, beta);
            load_row<EPL, VEC>(bg + F, L, gamma);
          }
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const float pre = fmaf(gamma[e], hh[u][e], beta[e]);
            acc[e] = fmaf(sc[u], act_on(relu, pre) ? pre : 0.f, acc[e]);
          }
        }
      }
    }
    if (s.chunk_id >= 0) {  // partial sum of one chunk of a long row: the merge adds the residual
      store_row<EPL, VEC>(part + s.chunk_id * F, L, acc);
    } else {
      if (residual) {
        float res[EPL];
        load_row<EPL, VEC>(residual + s.row * ld_r, L, res);
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] += res[e];
      }
      store_row<EPL, VEC>(out + s.row * F, L, acc);
    }
  }
}

// ---- backward, by destination ----------------------------------------------------------------
// A wave owns pair row p = (r, i) (or a chunk of its slots) with [beta | gamma]_{r,i} and g_i in
// registers.  part and the block r of grad_g hold rows of 2F: [sum gm | sum gm * h].
template <typename IdxT, int EPL, bool VEC>
__global__ void __launch_bounds__(kBlock)
    film_bwd_dst_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                        const IdxT* __restrict__ pair_rel, const IdxT* __restrict__ pair_node,
                        const float* __restrict__ H, int64_t ld_h, const float* __restrict__ G,
                        int64_t ld_gb, const float* __restrict__ grad_out, int64_t ld_g, int relu,
                        int mean, int F, int lph, float* __restrict__ grad_g, int64_t ld_gg,
                        float* __restrict__ part) {
  constexpr int U = FilmSlots<EPL>::dst;
  const Lay L = make_lay(1, F, lph);
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    const int64_t r = static_cast<int64_t>(pair_rel[s.row]);
    const int64_t i = static_cast<int64_t>(pair_node[s.row]);
    float beta[EPL], gamma[EPL], g[EPL], gb[EPL], gg[EPL];
    const float* bg = G + i * ld_gb + r * 2 * F;
    load_row<EPL, VEC>(bg, L, beta);
    load_row<EPL, VEC>(bg + F, L, gamma);
    load_row<EPL, VEC>(grad_out + i * ld_g, L, g);
#pragma unroll
    for (int e = 0; e < EPL; ++e) gb[e] = gg[e] = 0.f;
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float hh[U][EPL];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1)
          load_row<EPL, VEC>(H + static_cast<int64_t>(col[k + u]) * ld_h + r * F, L, hh[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const float pre = fmaf(gamma[e], hh[u][e], beta[e]);
            const float gm = act_on(relu, pre) ? g[e] : 0.f;
            gb[e] += gm;
            gg[e] = fmaf(gm, hh[u][e], gg[e]);
          }
        }
      }
    }
    float* row;
    if (s.chunk_id >= 0) {  // (the merge divides a split row, once)
      row = part + s.chunk_id * 2 * F;
    } else {
      row = grad_g + i * ld_gg + r * 2 * F;
      if (mean) {  // (a decoded span has slots)
        const float d = static_cast<float>(s.row_end - s.row_start);
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          gb[e] /= d;
          gg[e] /= d;
        }
      }
    }
    store_row<EPL, VEC>(row, L, gb);
    store_row<EPL, VEC>(row + F, L, gg);
  }
}

// ---- backward, by source ---------------------------------------------------------------------
// A wave owns pair row p = (r, j) of the flipped graph (or a chunk of its out-slots) with
// H[j, block r] in registers; slot t has destination i = col_t[t] and edge edge_id_t[t].
template <typename IdxT, int EPL, bool VEC>
__global__ void __launch_bounds__(kBlock)
    film_bwd_src_kernel(Items<IdxT> it, const IdxT* __restrict__ col_t,
                        const IdxT* __restrict__ edge_id_t, const IdxT* __restrict__ pair_rel,
                        const IdxT* __restrict__ pair_node, const float* __restrict__ H,
                        int64_t ld_h, const float* __restrict__ G, int64_t ld_gb,
                        const float* __restrict__ scale, const float* __restrict__ grad_out,
                        int64_t ld_g, int relu, int F, int lph, float* __restrict__ grad_h,
                        int64_t ld_gh, float* __restrict__ part) {
  constexpr int U = FilmSlots<EPL>::src;
  const Lay L = make_lay(1, F, lph);
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    const int64_t r = static_cast<int64_t>(pair_rel[s.row]);
    const int64_t j = static_cast<int64_t>(pair_node[s.row]);
    float h[EPL], gh[EPL];
    load_row<EPL, VEC>(H + j * ld_h + r * F, L, h);
#pragma unroll
    for (int e = 0; e < EPL; ++e) gh[e] = 0.f;
    for (int64_t t = s.k0; t < s.k1; t += U) {
      float beta[U][EPL], gamma[U][EPL], gg[U][EPL], sc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u < s.k1) {
          const int64_t i = static_cast<int64_t>(col_t[t + u]);
          const float* bg = G + i * ld_gb + r * 2 * F;
          load_row<EPL, VEC>(bg, L, beta[u]);
          load_row<EPL, VEC>(bg + F, L, gamma[u]);
          load_row<EPL, VEC>(grad_out + i * ld_g, L, gg[u]);
          sc[u] = scale ? scale[slot_edge(edge_id_t, t + u)] : 1.f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u < s.k1) {
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const float pre = fmaf(gamma[u][e], h[e], beta[u][e]);
            const float gm = act_on(relu, pre) ? sc[u] * gg[u][e] : 0.f;
            gh[e] = fmaf(gm, gamma[u][e], gh[e]);
          }
        }
      }
    }
    float* row = s.chunk_id >= 0 ? part + s.chunk_id * F : grad_h + j * ld_gh + r * F;
    store_row<EPL, VEC>(row, L, gh);
  }
}

// hub rows: the chunks' partial rows (W floats each) summed in chunk order, then the epilogue
// (mean: / the row's slot count; residual != NULL: + residual[node]) into block pair_rel[row] of
// row pair_node[row] of dst (pair tables NULL: the row itself, block 0)
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    film_merge_kernel(const IdxT* __restrict__ rowptr, const IdxT* __restrict__ hub_rows,
                      const IdxT* __restrict__ hub_cptr, const IdxT* __restrict__ pair_rel,
                      const IdxT* __restrict__ pair_node, int64_t W,
                      const float* __restrict__ part, int mean,
                      const float* __restrict__ residual, int64_t ld_r, float* __restrict__ dst,
                      int64_t ld_dst) {
  const int64_t hr = blockIdx.x;
  const int64_t row = static_cast<int64_t>(hub_rows[hr]);
  const int64_t c0 = static_cast<int64_t>(hub_cptr[hr]), c1 = static_cast<int64_t>(hub_cptr[hr + 1]);
  const int64_t node = pair_node ? static_cast<int64_t>(pair_node[row]) : row;
  const int64_t off = pair_rel ? static_cast<int64_t>(pair_rel[row]) * W : 0;
  const float d = static_cast<float>(rowptr[row + 1] - rowptr[row]);  // (a hub row has slots)
  for (int64_t t = threadIdx.x; t < W; t += kWave) {
    float acc = 0.f;
    for (int64_t c = c0; c < c1; ++c) acc += part[c * W + t];
    if (mean) acc /= d;
    if (residual) acc += residual[node * ld_r + t];
    dst[node * ld_dst + off + t] = acc;
  }
}

// ---- host side -------------------------------------------------------------------------------
// Every launch walks its items at the stride of a capped grid, as cg.hip does: consecutive rows go
// to different workgroups, so the long rows of a skewed graph do not share a few compute units.
constexpr unsigned kFilmBlocks = 2048;

unsigned film_grid(int64_t n_items) { return gine_grid(n_items, true, kFilmBlocks); }

bool film_envelope(int64_t F, int64_t) { return F >= 1 && F <= kMaxWidth; }

// pygamd_resgated_workspace_bytes(n_chunks, F, 0): a chunk's partial row of up to 2F
size_t film_ws_bytes(int64_t n_chunks, int64_t F) {
  size_t bytes = 0;
  pygamd_resgated_workspace_bytes(n_chunks, F, 0, &bytes);  // (inside resgated's envelope)
  return bytes;
}

template <typename IdxT>
int launch_merge(const Items<IdxT>& it, const IdxT* pair_rel, const IdxT* pair_node, int64_t W,
                 const float* part, int mean, const float* residual, int64_t ld_r, float* dst,
                 int64_t ld_dst, hipStream_t st) {
  if (it.n_hub > 0) {
    hipLaunchKernelGGL((film_merge_kernel<IdxT>), dim3(static_cast<unsigned>(it.n_hub)),
                       dim3(kWave), 0, st, it.rowptr, it.hub_rows, it.hub_cptr, pair_rel,
                       pair_node, W, part, mean, residual, ld_r, dst, ld_dst);
    PYGAMD_LAUNCH_CHECK();
  }
  return PYGAMD_OK;
}

// gine_device.h's shape table without an edge term: `...` sees EPL and VEC
#define FILM_DISPATCH(...)                  \
  GINE_DISPATCH({                           \
    if constexpr (DE == 0) {                \
      __VA_ARGS__                           \
    } else {                                \
      return PYGAMD_ERR_UNSUPPORTED;        \
    }                                       \
  })

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_film_supported(int64_t F) { return film_envelope(F, 0) ? 1 : 0; }

int pygamd_film_forward(const pygamd_csr* g, const void* edge_id, const int32_t* rel,
                        const float* h, int64_t ld_h, const float* gb, int64_t ld_gb,
                        const float* scale, const float* residual, int64_t ld_r, int act_mode,
                        int64_t n_src, int64_t F, int64_t R, float* out, void* workspace,
                        size_t workspace_bytes, void* stream) {
  const int rc = gine_check(g, n_src, F, 0, film_envelope);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;
  if (R < 1 || ld_h < R * F || ld_gb < 2 * R * F || (residual && ld_r < F) ||
      (act_mode != 0 && act_mode != 1))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !rel || !h || !gb || !out) return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < film_ws_bytes(n_chunks, F)))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(h) && ld_h % 4 == 0 && aligned16(gb) && ld_gb % 4 == 0 &&
                  aligned16(out) && (!residual || (aligned16(residual) && ld_r % 4 == 0)) &&
                  (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, 0, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(film_grid(n_rows + n_chunks)), block(kBlock);
    FILM_DISPATCH({
      hipLaunchKernelGGL((film_fwd_kernel<IdxT, EPL, VEC>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), rel, h, ld_h, gb,
                         ld_gb, scale, residual, ld_r, act_mode, static_cast<int>(F), sh.lph, out,
                         part);
    });
    PYGAMD_LAUNCH_CHECK();
    // (hub rows: the chunks' partial sums in chunk order, then the residual, once)
    return launch_merge<IdxT>(it, nullptr, nullptr, F, part, 0, residual, ld_r, out, F, st);
  });
}

int pygamd_film_backward_dst(const pygamd_csr* g, const void* pair_rel, const void* pair_dst,
                             const float* h, int64_t ld_h, const float* gb, int64_t ld_gb,
                             const float* grad_out, int64_t ld_g, int act_mode, int mean,
                             int64_t n_src, int64_t F, int64_t R, float* grad_gb, int64_t ld_ggb,
                             void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = gine_check(g, n_src, F, 0, film_envelope);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;
  if (R < 1 || ld_h < R * F || ld_gb < 2 * R * F || ld_g < F || ld_ggb < 2 * R * F ||
      (act_mode != 0 && act_mode != 1) || (mean != 0 && mean != 1))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !pair_rel || !pair_dst || !h || !gb || !grad_out || !grad_gb)
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < film_ws_bytes(n_chunks, F)))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(h) && ld_h % 4 == 0 && aligned16(gb) && ld_gb % 4 == 0 &&
                  aligned16(grad_out) && ld_g % 4 == 0 && aligned16(grad_gb) && ld_ggb % 4 == 0 &&
                  (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, 0, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const IdxT* prel = static_cast<const IdxT*>(pair_rel);
    const IdxT* pnode = static_cast<const IdxT*>(pair_dst);
    const dim3 grid(film_grid(n_rows + n_chunks)), block(kBlock);
    FILM_DISPATCH({
      hipLaunchKernelGGL((film_bwd_dst_kernel<IdxT, EPL, VEC>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), prel, pnode, h, ld_h, gb, ld_gb, grad_out, ld_g,
                         act_mode, mean, static_cast<int>(F), sh.lph, grad_gb, ld_ggb, part);
    });
    PYGAMD_LAUNCH_CHECK();
    // (long pair rows: the chunks' packed partial rows of 2F in chunk order, then the division)
    return launch_merge<IdxT>(it, prel, pnode, 2 * F, part, mean, nullptr, 0, grad_gb, ld_ggb, st);
  });
}

int pygamd_film_backward_src(const pygamd_csr* g, const void* edge_id_t, const void* pair_rel,
                             const void* pair_src, const float* h, int64_t ld_h, const float* gb,
                             int64_t ld_gb, const float* scale, const float* grad_out,
                             int64_t ld_g, int act_mode, int64_t n_dst, int64_t F, int64_t R,
                             float* grad_h, int64_t ld_gh, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const int rc = gine_check(g, n_dst, F, 0, film_envelope);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;
  if (R < 1 || ld_h < R * F || ld_gb < 2 * R * F || ld_g < F || ld_gh < R * F ||
      (act_mode != 0 && act_mode != 1))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !pair_rel || !pair_src || !h || !gb || !grad_out || !grad_h)
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < film_ws_bytes(n_chunks, F)))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(h) && ld_h % 4 == 0 && aligned16(gb) && ld_gb % 4 == 0 &&
                  aligned16(grad_out) && ld_g % 4 == 0 && aligned16(grad_h) && ld_gh % 4 == 0 &&
                  (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, 0, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const IdxT* prel = static_cast<const IdxT*>(pair_rel);
    const IdxT* pnode = static_cast<const IdxT*>(pair_src);
    const dim3 grid(film_grid(n_rows + n_chunks)), block(kBlock);
    FILM_DISPATCH({
      hipLaunchKernelGGL((film_bwd_src_kernel<IdxT, EPL, VEC>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id_t), prel, pnode, h,
                         ld_h, gb, ld_gb, scale, grad_out, ld_g, act_mode, static_cast<int>(F),
                         sh.lph, grad_h, ld_gh, part);
    });
    PYGAMD_LAUNCH_CHECK();
    // (long pair rows: the chunks' partial rows in chunk order)
    return launch_merge<IdxT>(it, prel, pnode, F, part, 0, nullptr, 0, grad_h, ld_gh, st);
  });
}

}  // extern "C"
