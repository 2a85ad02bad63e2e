// gine_device.h — what the kernels with a per-slot linear edge term W a_k (+ b) share, on top of
// the row walk of rowwalk_device.h.  Forward side: the envelope, the edge arguments, a slot's edge
// id and raw features, a lane's rows of the edge weight in registers, the edge term, the lane
// shape with its register capacity for De, the capped grid and the dispatch over the
// instantiations.  Backward side: the update of the parameter gradients in registers by a slot
// (gine.hip, pna.hip, resgated.hip; gen.hip keeps it written out, the call cost its backward 1 %)
// and the launches that follow a backward's main one.  Each kernel keeps its own loop, loads and
// arithmetic in its own file — and the fold of a workgroup's waves into its partial through LDS,
// which as a function changed the register allocation of the backward (CHANGELOG).
// Included by gine.hip, pna.hip, gen.hip, resgated.hip and cg.hip; by film.hip for the shape, the
// capped grid and gine_check without an edge term; by mixture.hip for slot_edge.
#pragma once
#include "common.h"
#include "rowwalk_device.h"

namespace pygamd {
namespace gine {

using namespace rowwalk;

constexpr int kGineMaxDe = 32;
constexpr int kGineMaxWeight = 4096;  // F * De: 64 registers per lane at 64 busy lanes
// Linear mode: a wave loads its 64 * EPL * De weights once and then walks items at the stride of
// the grid, so the grid is capped; the caps depend on nothing but these constants, and the number
// of workgroups of a launch on the problem's sizes only (grad_W is reduced in workgroup order).
constexpr unsigned kGineFwdBlocks = 1024;
constexpr unsigned kGineBwdBlocks = 512;

// rows of W [F, De] (torch.nn.Linear's layout) and entries of b [F] (or NULL) of the lane's columns
template <int EPL, bool VEC, int DE>
__device__ __forceinline__ void load_weight(const float* __restrict__ weight,
                                            const float* __restrict__ bias, const Lay& L, int De,
                                            float (&w)[EPL][DE], float (&b)[EPL]) {
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int c = lane_col<VEC>(L, e);
    const bool ok = L.head_ok && c < L.C;
#pragma unroll
    for (int d = 0; d < DE; ++d)
      w[e][d] = (ok && d < De) ? weight[static_cast<int64_t>(c) * De + d] : 0.f;
    b[e] = (ok && bias) ? bias[c] : 0.f;
  }
}

// e = b + W a for this lane's columns; lane d of the wave holds a[d] in `av` (0 beyond De)
template <int EPL, int DE>
__device__ __forceinline__ void edge_term(const float (&w)[EPL][DE], const float (&b)[EPL],
                                          float av, float (&ev)[EPL]) {
#pragma unroll
  for (int e = 0; e < EPL; ++e) ev[e] = b[e];
#pragma unroll
  for (int d = 0; d < DE; ++d) {
    const float a = bcast_uniform(av, d);
#pragma unroll
    for (int e = 0; e < EPL; ++e) ev[e] = fmaf(w[e][d], a, ev[e]);
  }
}

// ---- the edge arguments and a slot's fetch ---------------------------------------------------
struct EdgeArgs {
  const float* edge_attr;  // [E, F] (wide), [E, De] (linear) or NULL (no edge term)
  const float* weight;     // [F, De] or NULL
  const float* bias;       // [F] or NULL
  int De;
};

// the edge of slot k in the original edge order
template <typename IdxT>
__device__ __forceinline__ int64_t slot_edge(const IdxT* __restrict__ edge_id, int64_t k) {
  return edge_id ? static_cast<int64_t>(edge_id[k]) : k;
}

// this lane's entry of a_k, the raw features of edge `id` (0 beyond De)
__device__ __forceinline__ float edge_lane(const EdgeArgs& ed, int64_t id, int lane) {
  return lane < ed.De ? ed.edge_attr[id * ed.De + lane] : 0.f;
}

// ---- backward of the linear edge term ---------------------------------------------------------
// grad_W[f, d] = sum_k g_k[f] a_k[d] and grad_b[f] = sum_k g_k[f] accumulate in the lane's registers
// gw and gb (the kernel zeroes them) over all items of the wave.  BIAS = false: no grad_b, gb is
// not touched and may be any array of the lane.
//
// One slot with the gradient g of its edge term (already masked) and its raw features `av` (lane
// d holds a[d]): gw and gb take it in, and grad_edge_attr[id, d] = sum_f g[f] W[f, d], a wave sum
// per d, goes to row `id` of grad_edge (NULL, wave-uniform: not wanted).
template <bool BIAS, int EPL, int DE>
__device__ __forceinline__ void edge_grad_take(const float (&g)[EPL], float av,
                                               const float (&w)[EPL][DE], int De, int lane,
                                               float* grad_edge, int64_t id,
                                               float (&gw)[EPL][DE], float (&gb)[EPL]) {
#pragma unroll
  for (int d = 0; d < DE; ++d) {
    const float a = bcast_uniform(av, d);
#pragma unroll
    for (int e = 0; e < EPL; ++e) gw[e][d] = fmaf(g[e], a, gw[e][d]);
  }
  if constexpr (BIAS) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) gb[e] += g[e];
  }
  if (grad_edge) {
    float mine = 0.f;
#pragma unroll
    for (int d = 0; d < DE; ++d) {
      if (d < De) {
        float p = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) p = fmaf(g[e], w[e][d], p);
        p = group_sum(p, kWave);
        if (lane == d) mine = p;
      }
    }
    if (lane < De) grad_edge[id * De + lane] = mine;
  }
}

// ---- host side -------------------------------------------------------------------------------
struct GineShape {
  int lph, epl, de;  // de: the register capacity for De (0: wide mode)
  bool vec;
};

inline bool gine_envelope(int64_t F, int64_t De) {
  if (F < 1 || F > kMaxWidth || De < 0) return false;
  return De == 0 || (De <= kGineMaxDe && F * De <= kGineMaxWeight);
}

inline bool gine_shape(int64_t F, int64_t De, bool aligned, GineShape* g) {
  if (!gine_envelope(F, De)) return false;
  if (De == 0) {
    Shape s;
    if (!choose_shape(1, F, aligned, &s)) return false;
    *g = GineShape{s.lph, s.epl, 0, s.vec};
    return true;
  }
  // linear mode: all 64 lanes share the columns, so that a lane's rows of W stay few
  const int de = De <= 4 ? 4 : De <= 8 ? 8 : De <= 16 ? 16 : 32;
  if (aligned && F % 4 == 0 && F > 128) {
    *g = GineShape{kWave, F <= 256 ? 4 : 8, de, true};
  } else {
    const int n = static_cast<int>((F + kWave - 1) / kWave);
    int epl = 1;
    while (epl < n) epl *= 2;
    *g = GineShape{kWave, epl, de, false};
  }
  return g->epl * g->de <= 128;  // (holds inside the envelope)
}

inline unsigned gine_grid(int64_t n_items, bool linear, unsigned cap) {
  const unsigned full = wave_grid(n_items);
  return linear && full > cap ? cap : full;
}

// `...` sees IdxT-independent constants EPL, VEC, DE of the shape
#define GINE_CASE(epl_, vec_, de_, ...)                                              \
  if (sh.epl == epl_ && sh.vec == vec_ && sh.de == de_) {                            \
    constexpr int EPL = epl_; constexpr bool VEC = vec_; constexpr int DE = de_;     \
    __VA_ARGS__                                                                      \
  } else

#define GINE_CASES_DE(de_, ...)                                                      \
  GINE_CASE(1, false, de_, __VA_ARGS__) GINE_CASE(2, false, de_, __VA_ARGS__)        \
  GINE_CASE(4, false, de_, __VA_ARGS__) GINE_CASE(4, true, de_, __VA_ARGS__)

#define GINE_DISPATCH(...)                                                           \
  do {                                                                               \
    GINE_CASES_DE(0, __VA_ARGS__) GINE_CASES_DE(4, __VA_ARGS__)                      \
    GINE_CASES_DE(8, __VA_ARGS__) GINE_CASES_DE(16, __VA_ARGS__)                     \
    GINE_CASES_DE(32, __VA_ARGS__)                                                   \
    GINE_CASE(8, false, 0, __VA_ARGS__) GINE_CASE(8, true, 0, __VA_ARGS__)           \
    GINE_CASE(8, false, 4, __VA_ARGS__) GINE_CASE(8, true, 4, __VA_ARGS__)           \
    GINE_CASE(8, false, 8, __VA_ARGS__) GINE_CASE(8, true, 8, __VA_ARGS__)           \
    GINE_CASE(8, false, 16, __VA_ARGS__) GINE_CASE(8, true, 16, __VA_ARGS__)         \
    { return PYGAMD_ERR_UNSUPPORTED; }                                               \
  } while (0)

// the edge arguments against the mode (PYGAMD_GEN_EDGE_*: none, wide, linear); 0 = go on
inline int check_edge(int edge_mode, const EdgeArgs& ed) {
  switch (edge_mode) {
    case PYGAMD_GEN_EDGE_NONE:
      return (ed.De == 0 && !ed.edge_attr && !ed.weight && !ed.bias) ? PYGAMD_OK
                                                                      : PYGAMD_ERR_INVALID_ARG;
    case PYGAMD_GEN_EDGE_WIDE:
      return (ed.De == 0 && ed.edge_attr && !ed.weight && !ed.bias) ? PYGAMD_OK
                                                                     : PYGAMD_ERR_INVALID_ARG;
    case PYGAMD_GEN_EDGE_LINEAR:
      return (ed.De > 0 && ed.edge_attr && ed.weight) ? PYGAMD_OK : PYGAMD_ERR_INVALID_ARG;
    default:
      return PYGAMD_ERR_INVALID_ARG;
  }
}

// floats of the backward's per-workgroup partials of (grad_W[, grad_b]) in the workspace
inline int64_t wpart_floats(int64_t F, int64_t De, bool bias_block) {
  return De > 0 ? static_cast<int64_t>(kGineBwdBlocks) * (F * De + (bias_block ? F : 0)) : 0;
}

// what follows a backward's main launch of n_blocks workgroups: the hub rows' chunks into grad_x,
// then (linear mode) the workgroups' partials into grad_weight and grad_bias (may be NULL)
template <typename IdxT>
inline int launch_backward_tail(const Items<IdxT>& it, int64_t F, int64_t De, bool bias_block,
                                unsigned n_blocks, const float* part, float* grad_x,
                                const float* wpart, float* grad_weight, float* grad_bias,
                                hipStream_t st) {
  const int rc = launch_sum_merge(it, F, part, grad_x, st);
  if (rc != PYGAMD_OK || De <= 0) return rc;
  return launch_param_reduce(wpart, n_blocks, static_cast<int>(F * De),
                             bias_block ? static_cast<int>(F) : 0, grad_weight, grad_bias, st);
}

// (`envelope`: a kernel file with a narrower one than gine_envelope passes its own)
inline int gine_check(const pygamd_csr* g, int64_t n_other, int64_t F, int64_t De,
                      bool (*envelope)(int64_t, int64_t) = gine_envelope) {
  if (De < 0 || F < 1) return PYGAMD_ERR_INVALID_ARG;
  const int rc = check_handle(g, n_other);
  if (rc != PYGAMD_OK) return rc;
  return envelope(F, De) ? PYGAMD_OK : PYGAMD_ERR_UNSUPPORTED;
}

}  // namespace gine
}  // namespace pygamd
