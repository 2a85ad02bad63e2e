// gine_device.h — what the kernels with a per-slot linear edge term share (gine.hip, pna.hip): the
// envelope, a lane's rows of the edge weight in registers, the edge term from a slot's raw
// features, the lane shape with its register capacity for De, the capped grid and the dispatch
// over the instantiations.  Lane layout, work items and merges: attn_device.h.
#pragma once
#include "attn_device.h"
#include "common.h"

namespace pygamd {
namespace gine {

using namespace attn;

constexpr int kGineMaxWidth = 512;
constexpr int kGineMaxDe = 32;
constexpr int kGineMaxWeight = 4096;  // F * De: 64 registers per lane at 64 busy lanes
// Linear mode: a wave loads its 64 * EPL * De weights once and then walks items at the stride of
// the grid, so the grid is capped; the caps depend on nothing but these constants, and the number
// of workgroups of a launch on the problem's sizes only (grad_W is reduced in workgroup order).
constexpr unsigned kGineFwdBlocks = 1024;
constexpr unsigned kGineBwdBlocks = 512;

// the column of register e of this lane
template <bool VEC>
__device__ __forceinline__ int lane_col(const Lay& L, int e) {
  if constexpr (VEC) return (L.sub + L.lph * (e >> 2)) * 4 + (e & 3);
  return L.sub + L.lph * e;
}

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

// ---- host side -------------------------------------------------------------------------------
struct GineShape {
  int lph, epl, de;  // de: the register capacity for De (0: wide mode)
  bool vec;
};

inline bool gine_envelope(int64_t F, int64_t De) {
  if (F < 1 || F > kGineMaxWidth || De < 0) return false;
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

inline int gine_check(const pygamd_csr* g, int64_t n_other, int64_t F, int64_t De) {
  if (De < 0) return PYGAMD_ERR_INVALID_ARG;
  const int rc = check_args(g, n_other, 1, F < 1 ? F : 1);
  if (rc != PYGAMD_OK) return rc;
  return gine_envelope(F, De) ? PYGAMD_OK : PYGAMD_ERR_UNSUPPORTED;
}

}  // namespace gine
}  // namespace pygamd
