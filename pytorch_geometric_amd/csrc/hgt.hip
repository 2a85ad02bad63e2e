// hgt.hip — the typed relation transform of nn.HGTConv for gfx950 (MI355X).
//
// Before its attention step the Heterogeneous Graph Transformer sends the key and the value rows
// of every edge type's source nodes through that edge type's own D x D matrix per head
// (hgt_conv.py:118-154).  The arithmetic is a block-diagonal product: D columns of one head times
// one D x D matrix, D / 4 flop per byte moved — memory-bound up to D = 128 on the exact fp32
// matrix instruction (v_mfma_f32_16x16x4_f32: bitwise an fmaf chain, fp32 accumulate).  Here
// every edge type of a layer call shares ONE launch per direction; the per-edge-type operands
// travel in the kernel arguments (at most 64 entries, as in hetero_conv.hip):
//
//   hgt_forward_rows      forward.  A workgroup owns 128 stacked source rows of one edge type; for
//                         every (head, key | value) it stages the D x D matrix in LDS (64 reduction
//                         rows at a time: 33 KB, whatever D), reads its rows in place from the
//                         [N, 3F] projection (row stride given) and writes the packed [S, 2F] table
//                         the attention kernels read.
//   hgt_backward_rows     input gradients.  A workgroup owns 128 rows of one source NODE type and
//                         walks the edge types that read them in the call's order: the products
//                         grad_kv @ W^T accumulate in registers and are written once, at the
//                         caller's row stride (the k and v column blocks of one [N, 3F] buffer).
//   hgt_wgrad_partial     weight gradients.  Workgroup (row chunk of an edge type, head, k | v)
//                         computes rows^T . grad rows into its own D x D slab of the workspace;
//   hgt_wgrad_reduce      sums the slabs of a matrix in chunk order and writes EVERY matrix of the
//                         parameter (zeros where the edge type is not in the call).
//
// No floating-point atomics; the chunking depends on the row counts only, so results are bitwise
// reproducible.  A D that is not a multiple of 16 is zero-padded inside the kernels.
#include "common.h"

namespace pygamd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kHgtMaxTypes = 64;
constexpr int kHgtSub = 2;                          // 16-row MFMA tiles per wave
constexpr int kHgtTileRows = 16 * kHgtSub * kWavesPerBlock;  // 128 rows per workgroup
constexpr int kHgtStageRows = 64;                   // reduction rows of a matrix staged at once
constexpr int kHgtChunkRows = 256;                  // least rows of a weight-gradient chunk
constexpr int kHgtMaxChunks = 512;                  // per call, over all edge types

// forward and weight gradient: per edge type of the call
struct HgtTable {
  const float* k[kHgtMaxTypes];
  const float* v[kHgtMaxTypes];
  int64_t src_off[kHgtMaxTypes + 1];  // stacked source rows of edge type e
  int32_t ld[kHgtMaxTypes];
  int32_t widx[kHgtMaxTypes];         // metadata position of the edge type
  int32_t begin[kHgtMaxTypes + 1];    // workgroups (forward) / chunks (weight gradient) of e
  int32_t chunk_rows[kHgtMaxTypes];   // weight gradient: rows per chunk
  int32_t n_et;
};
static_assert(sizeof(HgtTable) <= 2600, "HgtTable must stay small (kernel arguments: ~4 KB)");

// input gradients: per source node type, with the edge types that read it (call order)
struct HgtBwdTable {
  float* gk[kHgtMaxTypes];
  float* gv[kHgtMaxTypes];
  int32_t n[kHgtMaxTypes];
  int32_t ld[kHgtMaxTypes];
  int32_t begin[kHgtMaxTypes + 1];     // workgroups of node type t
  int32_t et_begin[kHgtMaxTypes + 1];  // entries [et_begin[t], et_begin[t + 1]) of the lists below
  int64_t et_src_off[kHgtMaxTypes];
  int32_t et_widx[kHgtMaxTypes];
  int32_t n_nt;
};
static_assert(sizeof(HgtBwdTable) <= 2900, "HgtBwdTable must stay small");

// the block t with begin[t] <= i < begin[t + 1] (empty blocks are skipped); i < begin[n]
__device__ __forceinline__ int hgt_block_of(const int32_t* begin, int n, int i) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (begin[mid] <= i) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  return lo;
}

// Reduction rows [kbase, kbase + KS) of the B operand into LDS, zero-padded to Dp columns.
// TR = false: B[k][n] = W[k][n] (rows @ W); TR = true: B[k][n] = W[n][k] (rows @ W^T).
template <int NT, bool TR>
__device__ __forceinline__ void hgt_stage(float* wl, const float* __restrict__ W, int D,
                                          int kbase) {
  constexpr int Dp = NT * 16, KS = Dp < kHgtStageRows ? Dp : kHgtStageRows, LDW = Dp + 4;
  for (int i = threadIdx.x; i < KS * Dp; i += kBlock) {
    int kk, n;
    if constexpr (TR) {
      n = i / KS;
      kk = i - n * KS;
    } else {
      kk = i / Dp;
      n = i - kk * Dp;
    }
    const int k = kbase + kk;
    float val = 0.f;
    if (k < D && n < D) val = TR ? W[n * D + k] : W[k * D + n];
    wl[kk * LDW + n] = val;
  }
}

// The A fragments of one 16-row tile: lane (r = l & 15, g = l >> 4) holds columns 16 s + 4 g + j
// (j = 0..3) of row r, so that one 16-byte load serves four reduction steps.  The reduction order
// of a 16-column group is therefore j-major; hgt_mma reads B to match.  p: the row's head slice,
// or NULL for a row outside the block.
template <int NT, bool V4>
__device__ __forceinline__ void hgt_load_a(const float* __restrict__ p, int D, int g,
                                           f32x4 (&a)[NT]) {
#pragma unroll
  for (int s = 0; s < NT; ++s) {
    const int col = 16 * s + 4 * g;
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    if (p != nullptr && col < D) {
      if constexpr (V4) {
        t = *reinterpret_cast<const f32x4*>(p + col);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (col + j < D) t[j] = p[col + j];
        }
      }
    }
    a[s] = t;
  }
}

// acc[sub][n] += A[sub] (16 x KS slice starting at reduction row KB) @ staged B
template <int NT, int KB>
__device__ __forceinline__ void hgt_mma(const float* wl, int r, int g,
                                        const f32x4 (&a)[kHgtSub][NT],
                                        f32x4 (&acc)[kHgtSub][NT]) {
  constexpr int Dp = NT * 16, KS = Dp < kHgtStageRows ? Dp : kHgtStageRows, LDW = Dp + 4;
#pragma unroll
  for (int ss = 0; ss < KS / 16; ++ss) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* brow = wl + (16 * ss + 4 * g + j) * LDW + r;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const float b = brow[16 * n];
#pragma unroll
        for (int sub = 0; sub < kHgtSub; ++sub) {
          acc[sub][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[sub][KB / 16 + ss][j], b,
                                                             acc[sub][n], 0, 0, 0);
        }
      }
    }
  }
}

// one (head, k | v) product of a workgroup's rows against one staged matrix
template <int NT, bool V4, bool TR>
__device__ __forceinline__ void hgt_product(float* wl, const float* __restrict__ W, int D,
                                            const float* (&rows)[kHgtSub], int r, int g,
                                            f32x4 (&acc)[kHgtSub][NT]) {
  constexpr int Dp = NT * 16, KS = Dp < kHgtStageRows ? Dp : kHgtStageRows;
  f32x4 a[kHgtSub][NT];
#pragma unroll
  for (int sub = 0; sub < kHgtSub; ++sub) hgt_load_a<NT, V4>(rows[sub], D, g, a[sub]);
  __syncthreads();  // the previous product has read its matrix
  hgt_stage<NT, TR>(wl, W, D, 0);
  __syncthreads();
  hgt_mma<NT, 0>(wl, r, g, a, acc);
  if constexpr (Dp > KS) {
    static_assert(Dp == 2 * KS, "two stages cover the widest head");
    __syncthreads();
    hgt_stage<NT, TR>(wl, W, D, KS);
    __syncthreads();
    hgt_mma<NT, KS>(wl, r, g, a, acc);
  }
}

// C layout of the 16x16 tile: column l & 15, rows 4 (l >> 4) + 0..3
template <int NT>
__device__ __forceinline__ void hgt_store(float* __restrict__ out, int64_t ld, int64_t row0,
                                          int64_t n_rows, int D, int r, int g,
                                          const f32x4 (&acc)[NT]) {
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = 16 * n + r;
    if (col < D) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = row0 + 4 * g + i;
        if (row < n_rows) out[row * ld + col] = acc[n][i];
      }
    }
  }
}

template <int NT, bool V4>
__global__ void __launch_bounds__(kBlock)
    hgt_forward_rows(const HgtTable tab, const float* __restrict__ wk,
                     const float* __restrict__ wv, int T, int H, int D, float* __restrict__ kv) {
  constexpr int Dp = NT * 16, KS = Dp < kHgtStageRows ? Dp : kHgtStageRows, LDW = Dp + 4;
  __shared__ float wl[KS * LDW];
  const int wg = blockIdx.x;
  const int e = hgt_block_of(tab.begin, tab.n_et, wg);
  const int64_t n_e = tab.src_off[e + 1] - tab.src_off[e];
  const int lane = lane_id(), r = lane & 15, g = lane >> 4;
  const int64_t row0 = static_cast<int64_t>(wg - tab.begin[e]) * kHgtTileRows +
                       wave_in_block() * (16 * kHgtSub);
  const int64_t F = static_cast<int64_t>(H) * D;
  const int64_t ld = tab.ld[e];
  float* __restrict__ out = kv + tab.src_off[e] * 2 * F;
  for (int c = 0; c < 2 * H; ++c) {
    const int h = c >> 1, which = c & 1;
    const float* __restrict__ in = (which ? tab.v[e] : tab.k[e]) + h * D;
    const float* W = (which ? wv : wk) + (static_cast<int64_t>(h) * T + tab.widx[e]) * D * D;
    const float* rows[kHgtSub];
    f32x4 acc[kHgtSub][NT];
#pragma unroll
    for (int sub = 0; sub < kHgtSub; ++sub) {
      const int64_t row = row0 + 16 * sub + r;
      rows[sub] = row < n_e ? in + row * ld : nullptr;
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[sub][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    hgt_product<NT, V4, false>(wl, W, D, rows, r, g, acc);
#pragma unroll
    for (int sub = 0; sub < kHgtSub; ++sub) {
      hgt_store<NT>(out + which * F + h * D, 2 * F, row0 + 16 * sub, n_e, D, r, g, acc[sub]);
    }
  }
}

template <int NT, bool V4>
__global__ void __launch_bounds__(kBlock)
    hgt_backward_rows(const HgtBwdTable tab, const float* __restrict__ wk,
                      const float* __restrict__ wv, int T, int H, int D,
                      const float* __restrict__ grad_kv) {
  constexpr int Dp = NT * 16, KS = Dp < kHgtStageRows ? Dp : kHgtStageRows, LDW = Dp + 4;
  __shared__ float wl[KS * LDW];
  const int wg = blockIdx.x;
  const int t = hgt_block_of(tab.begin, tab.n_nt, wg);
  const int64_t n_t = tab.n[t];
  const int lane = lane_id(), r = lane & 15, g = lane >> 4;
  const int64_t row0 = static_cast<int64_t>(wg - tab.begin[t]) * kHgtTileRows +
                       wave_in_block() * (16 * kHgtSub);
  const int64_t F = static_cast<int64_t>(H) * D;
  for (int c = 0; c < 2 * H; ++c) {
    const int h = c >> 1, which = c & 1;
    f32x4 acc[kHgtSub][NT];
#pragma unroll
    for (int sub = 0; sub < kHgtSub; ++sub) {
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[sub][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // the edge types that read these rows, in the call's order: one fixed summation order
    for (int i = tab.et_begin[t]; i < tab.et_begin[t + 1]; ++i) {
      const float* __restrict__ in = grad_kv + tab.et_src_off[i] * 2 * F + which * F + h * D;
      const float* W = (which ? wv : wk) + (static_cast<int64_t>(h) * T + tab.et_widx[i]) * D * D;
      const float* rows[kHgtSub];
#pragma unroll
      for (int sub = 0; sub < kHgtSub; ++sub) {
        const int64_t row = row0 + 16 * sub + r;
        rows[sub] = row < n_t ? in + row * 2 * F : nullptr;
      }
      hgt_product<NT, V4, true>(wl, W, D, rows, r, g, acc);
    }
    float* __restrict__ out = (which ? tab.gv[t] : tab.gk[t]) + h * D;
#pragma unroll
    for (int sub = 0; sub < kHgtSub; ++sub) {
      hgt_store<NT>(out, tab.ld[t], row0 + 16 * sub, n_t, D, r, g, acc[sub]);
    }
  }
}

// ws[(chunk * 2H + 2 h + which)][D][D] = rows^T . grad rows over the chunk's rows.  The NT x NT
// output tiles are split over the four waves: NT >= 4: NT / 4 tile rows each; NT = 2: one tile
// each; NT = 1: wave 0 alone.
template <int NT>
__global__ void __launch_bounds__(kBlock)
    hgt_wgrad_partial(const HgtTable tab, const float* __restrict__ grad_kv, int H, int D,
                      float* __restrict__ ws) {
  constexpr int MT = NT >= 4 ? NT / 4 : 1;
  constexpr int NN = NT >= 4 ? NT : 1;
  const int cg = blockIdx.x;
  const int e = hgt_block_of(tab.begin, tab.n_et, cg);
  const int64_t n_e = tab.src_off[e + 1] - tab.src_off[e];
  const int h = blockIdx.y >> 1, which = blockIdx.y & 1;
  const int w = wave_in_block();
  const int lane = lane_id(), r = lane & 15, g = lane >> 4;
  const int mb = NT >= 4 ? w * MT : (NT == 2 ? (w >> 1) : 0);
  const int nb = NT == 2 ? (w & 1) : 0;
  if (NT == 1 && w != 0) return;
  const int64_t F = static_cast<int64_t>(H) * D;
  const int64_t lo = static_cast<int64_t>(cg - tab.begin[e]) * tab.chunk_rows[e];
  const int64_t hi = lo + tab.chunk_rows[e] < n_e ? lo + tab.chunk_rows[e] : n_e;
  const int64_t ld = tab.ld[e];
  const float* __restrict__ in = (which ? tab.v[e] : tab.k[e]) + h * D;
  const float* __restrict__ gp = grad_kv + tab.src_off[e] * 2 * F + which * F + h * D;
  f32x4 acc[MT][NN];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int n = 0; n < NN; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t j0 = lo; j0 < hi; j0 += 4) {
    const int64_t j = j0 + g;
    const bool valid = j < hi;
    float am[MT], bn[NN];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int col = 16 * (mb + i) + r;
      am[i] = (valid && col < D) ? in[j * ld + col] : 0.f;
    }
#pragma unroll
    for (int n = 0; n < NN; ++n) {
      const int col = 16 * (nb + n) + r;
      bn[n] = (valid && col < D) ? gp[j * 2 * F + col] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
      for (int n = 0; n < NN; ++n) {
        acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(am[i], bn[n], acc[i][n], 0, 0, 0);
      }
    }
  }
  float* __restrict__ slab = ws + (static_cast<int64_t>(cg) * 2 * H + blockIdx.y) * D * D;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int n = 0; n < NN; ++n) {
      const int col = 16 * (nb + n) + r;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = 16 * (mb + i) + 4 * g + q;
        if (m < D && col < D) slab[m * D + col] = acc[i][n][q];
      }
    }
  }
}

// grad_w[h * T + ti] = the slabs of the edge type with metadata position ti, summed in chunk
// order; zero when the call has no such edge type (or it has no rows)
__global__ void __launch_bounds__(kBlock)
    hgt_wgrad_reduce(const HgtTable tab, const float* __restrict__ ws, int T, int H, int D,
                     float* __restrict__ grad_wk, float* __restrict__ grad_wv) {
  const int slot = blockIdx.y, which = blockIdx.z;
  const int h = slot / T, ti = slot - h * T;
  int e = -1;
  for (int i = 0; i < tab.n_et; ++i) {
    if (tab.widx[i] == ti) e = i;
  }
  const int DD = D * D;
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= DD) return;
  float sum = 0.f;
  if (e >= 0) {
    for (int c = tab.begin[e]; c < tab.begin[e + 1]; ++c) {
      sum += ws[(static_cast<int64_t>(c) * 2 * H + 2 * h + which) * DD + idx];
    }
  }
  (which ? grad_wv : grad_wk)[static_cast<int64_t>(slot) * DD + idx] = sum;
}

static bool hgt_supported(int64_t H, int64_t D) {
  return H >= 1 && D >= 1 && H <= 64 && D <= 128 && H * D <= 512;
}

static int hgt_nt(int64_t D) { return D <= 16 ? 1 : D <= 32 ? 2 : D <= 64 ? 4 : 8; }

// chunks of the weight gradient of an edge type with n rows: a function of (n, n_et) alone
static void hgt_chunking(int64_t n, int n_et, int64_t* chunks, int64_t* rows) {
  if (n <= 0) {
    *chunks = 0;
    *rows = 0;
    return;
  }
  const int64_t cap = kHgtMaxChunks / n_et < 1 ? 1 : kHgtMaxChunks / n_et;
  int64_t c = ceil_div(n, kHgtChunkRows);
  if (c > cap) c = cap;
  *rows = round_up(ceil_div(n, c), 4);
  *chunks = ceil_div(n, *rows);
}

// et_table: host int64 [n_et][4] = ld, n_rows, widx, source node type
static int hgt_fill(const float* const* k, const float* const* v, const int64_t* et_table,
                    int n_et, int64_t T, int64_t H, int64_t D, HgtTable* tab, bool* v4) {
  if (n_et > kHgtMaxTypes) return PYGAMD_ERR_UNSUPPORTED;
  if (!hgt_supported(H, D)) return PYGAMD_ERR_UNSUPPORTED;
  if (n_et <= 0 || !et_table || T < n_et || H * T > 65535) return PYGAMD_ERR_INVALID_ARG;
  const int64_t F = H * D;
  tab->n_et = n_et;
  tab->src_off[0] = 0;
  *v4 = (D % 4 == 0);
  uint64_t seen[(65535 + 63) / 64 + 1] = {};
  for (int e = 0; e < n_et; ++e) {
    const int64_t ld = et_table[4 * e], n = et_table[4 * e + 1], wi = et_table[4 * e + 2];
    if (n < 0 || n > INT32_MAX || ld < F || ld > INT32_MAX || wi < 0 || wi >= T)
      return PYGAMD_ERR_INVALID_ARG;
    if ((seen[wi >> 6] >> (wi & 63)) & 1u) return PYGAMD_ERR_INVALID_ARG;  // one edge type twice
    seen[wi >> 6] |= 1ull << (wi & 63);
    if (n > 0 && (!k || !v || !k[e] || !v[e])) return PYGAMD_ERR_INVALID_ARG;
    tab->k[e] = n > 0 ? k[e] : nullptr;
    tab->v[e] = n > 0 ? v[e] : nullptr;
    tab->ld[e] = static_cast<int32_t>(ld);
    tab->widx[e] = static_cast<int32_t>(wi);
    tab->src_off[e + 1] = tab->src_off[e] + n;
    if (n > 0) {
      *v4 = *v4 && (ld % 4 == 0) && (reinterpret_cast<uintptr_t>(k[e]) % 16 == 0) &&
            (reinterpret_cast<uintptr_t>(v[e]) % 16 == 0);
    }
  }
  return PYGAMD_OK;
}

#define PYGAMD_HGT_DISPATCH(KERNEL, grid, st, ...)                                              \
  do {                                                                                          \
    switch (nt) {                                                                               \
      case 1:                                                                                   \
        if (v4) hipLaunchKernelGGL((KERNEL<1, true>), grid, dim3(kBlock), 0, st, __VA_ARGS__);  \
        else hipLaunchKernelGGL((KERNEL<1, false>), grid, dim3(kBlock), 0, st, __VA_ARGS__);    \
        break;                                                                                  \
      case 2:                                                                                   \
        if (v4) hipLaunchKernelGGL((KERNEL<2, true>), grid, dim3(kBlock), 0, st, __VA_ARGS__);  \
        else hipLaunchKernelGGL((KERNEL<2, false>), grid, dim3(kBlock), 0, st, __VA_ARGS__);    \
        break;                                                                                  \
      case 4:                                                                                   \
        if (v4) hipLaunchKernelGGL((KERNEL<4, true>), grid, dim3(kBlock), 0, st, __VA_ARGS__);  \
        else hipLaunchKernelGGL((KERNEL<4, false>), grid, dim3(kBlock), 0, st, __VA_ARGS__);    \
        break;                                                                                  \
      default:                                                                                  \
        if (v4) hipLaunchKernelGGL((KERNEL<8, true>), grid, dim3(kBlock), 0, st, __VA_ARGS__);  \
        else hipLaunchKernelGGL((KERNEL<8, false>), grid, dim3(kBlock), 0, st, __VA_ARGS__);    \
    }                                                                                           \
  } while (0)

}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_hgt_supported(int64_t H, int64_t D) { return hgt_supported(H, D) ? 1 : 0; }

int pygamd_hgt_workspace_bytes(const int64_t* et_table, int n_et, int64_t H, int64_t D,
                               size_t* bytes) {
  if (n_et > kHgtMaxTypes || !hgt_supported(H, D)) return PYGAMD_ERR_UNSUPPORTED;
  if (n_et <= 0 || !et_table || !bytes) return PYGAMD_ERR_INVALID_ARG;
  int64_t total = 0;
  for (int e = 0; e < n_et; ++e) {
    if (et_table[4 * e + 1] < 0) return PYGAMD_ERR_INVALID_ARG;
    int64_t c, rows;
    hgt_chunking(et_table[4 * e + 1], n_et, &c, &rows);
    total += c;
  }
  *bytes = static_cast<size_t>(total) * 2 * H * D * D * sizeof(float);
  return PYGAMD_OK;
}

int pygamd_hgt_relation_forward(const float* const* k, const float* const* v,
                                const int64_t* et_table, int n_et, const float* wk,
                                const float* wv, int64_t T, int64_t H, int64_t D, float* kv,
                                void* stream) {
  HgtTable tab = {};
  bool v4 = false;
  const int rc = hgt_fill(k, v, et_table, n_et, T, H, D, &tab, &v4);
  if (rc != PYGAMD_OK) return rc;
  const int64_t S = tab.src_off[n_et];
  if (S == 0) return PYGAMD_OK;
  if (!wk || !wv || !kv) return PYGAMD_ERR_INVALID_ARG;
  int64_t wgs = 0;
  for (int e = 0; e < n_et; ++e) {
    tab.begin[e] = static_cast<int32_t>(wgs);
    wgs += ceil_div(tab.src_off[e + 1] - tab.src_off[e], kHgtTileRows);
  }
  tab.begin[n_et] = static_cast<int32_t>(wgs);
  if (wgs > INT32_MAX) return PYGAMD_ERR_UNSUPPORTED;
  const int nt = hgt_nt(D);
  hipStream_t st = as_stream(stream);
  const dim3 grid(static_cast<unsigned>(wgs));
  PYGAMD_HGT_DISPATCH(hgt_forward_rows, grid, st, tab, wk, wv, static_cast<int>(T),
                      static_cast<int>(H), static_cast<int>(D), kv);
  PYGAMD_LAUNCH_CHECK();
  return PYGAMD_OK;
}

int pygamd_hgt_relation_backward(const float* const* k, const float* const* v,
                                 const int64_t* et_table, int n_et, const float* wk,
                                 const float* wv, int64_t T, int64_t H, int64_t D,
                                 const float* grad_kv, float* const* grad_k,
                                 float* const* grad_v, const int64_t* nt_table, int n_nt,
                                 float* grad_wk, float* grad_wv, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  HgtTable tab = {};
  bool v4 = false;
  int rc = hgt_fill(k, v, et_table, n_et, T, H, D, &tab, &v4);
  if (rc != PYGAMD_OK) return rc;
  if (n_nt > kHgtMaxTypes) return PYGAMD_ERR_UNSUPPORTED;
  if (n_nt < 0 || (n_nt > 0 && (!nt_table || !grad_k || !grad_v)))
    return PYGAMD_ERR_INVALID_ARG;
  if ((grad_wk == nullptr) != (grad_wv == nullptr)) return PYGAMD_ERR_INVALID_ARG;
  const int64_t F = H * D;
  const int64_t S = tab.src_off[n_et];
  // input gradients: node types with their edge types in call order
  HgtBwdTable bt = {};
  bt.n_nt = n_nt;
  bool v4b = (D % 4 == 0) && (reinterpret_cast<uintptr_t>(grad_kv) % 16 == 0);
  int64_t wgs = 0;
  int n_list = 0;
  for (int t = 0; t < n_nt; ++t) {
    const int64_t n = nt_table[2 * t], ld = nt_table[2 * t + 1];
    if (n < 0 || n > INT32_MAX || ld < F || ld > INT32_MAX) return PYGAMD_ERR_INVALID_ARG;
    if (n > 0 && (!grad_k[t] || !grad_v[t])) return PYGAMD_ERR_INVALID_ARG;
    bt.gk[t] = grad_k[t];
    bt.gv[t] = grad_v[t];
    bt.n[t] = static_cast<int32_t>(n);
    bt.ld[t] = static_cast<int32_t>(ld);
    bt.begin[t] = static_cast<int32_t>(wgs);
    wgs += ceil_div(n, kHgtTileRows);
    bt.et_begin[t] = n_list;
    for (int e = 0; e < n_et; ++e) {
      if (et_table[4 * e + 3] != t) continue;
      if (et_table[4 * e + 1] != n) return PYGAMD_ERR_INVALID_ARG;  // one row per source node
      bt.et_src_off[n_list] = tab.src_off[e];
      bt.et_widx[n_list] = tab.widx[e];
      ++n_list;
    }
    if (n > 0) {
      v4b = v4b && (ld % 4 == 0) && (reinterpret_cast<uintptr_t>(grad_k[t]) % 16 == 0) &&
            (reinterpret_cast<uintptr_t>(grad_v[t]) % 16 == 0);
    }
  }
  bt.begin[n_nt] = static_cast<int32_t>(wgs);
  bt.et_begin[n_nt] = n_list;
  if (wgs > INT32_MAX) return PYGAMD_ERR_UNSUPPORTED;
  // weight gradients: the chunks
  int64_t chunks = 0;
  for (int e = 0; e < n_et; ++e) {
    int64_t c, rows;
    hgt_chunking(tab.src_off[e + 1] - tab.src_off[e], n_et, &c, &rows);
    tab.begin[e] = static_cast<int32_t>(chunks);
    tab.chunk_rows[e] = static_cast<int32_t>(rows);
    chunks += c;
  }
  tab.begin[n_et] = static_cast<int32_t>(chunks);
  const size_t need = static_cast<size_t>(chunks) * 2 * H * D * D * sizeof(float);
  if (grad_wk && need > 0 && (!workspace || workspace_bytes < need)) return PYGAMD_ERR_WORKSPACE;
  if ((S > 0 || wgs > 0) && (!wk || !wv)) return PYGAMD_ERR_INVALID_ARG;
  if (S > 0 && !grad_kv) return PYGAMD_ERR_INVALID_ARG;
  const int nt = hgt_nt(D);
  hipStream_t st = as_stream(stream);
  if (wgs > 0) {
    const dim3 grid(static_cast<unsigned>(wgs));
    const bool v4 = v4b;
    PYGAMD_HGT_DISPATCH(hgt_backward_rows, grid, st, bt, wk, wv, static_cast<int>(T),
                        static_cast<int>(H), static_cast<int>(D), grad_kv);
    PYGAMD_LAUNCH_CHECK();
  }
  if (grad_wk) {
    float* ws = static_cast<float*>(workspace);
    if (chunks > 0) {
      const dim3 grid(static_cast<unsigned>(chunks), static_cast<unsigned>(2 * H));
#define PYGAMD_HGT_WGRAD(NT)                                                               \
  hipLaunchKernelGGL((hgt_wgrad_partial<NT>), grid, dim3(kBlock), 0, st, tab, grad_kv,     \
                     static_cast<int>(H), static_cast<int>(D), ws)
      switch (nt) {
        case 1: PYGAMD_HGT_WGRAD(1); break;
        case 2: PYGAMD_HGT_WGRAD(2); break;
        case 4: PYGAMD_HGT_WGRAD(4); break;
        default: PYGAMD_HGT_WGRAD(8);
      }
#undef PYGAMD_HGT_WGRAD
      PYGAMD_LAUNCH_CHECK();
    }
    const dim3 grid(static_cast<unsigned>(ceil_div(D * D, kBlock)), static_cast<unsigned>(H * T),
                    2);
    hipLaunchKernelGGL(hgt_wgrad_reduce, grid, dim3(kBlock), 0, st, tab, ws,
                       static_cast<int>(T), static_cast<int>(H), static_cast<int>(D), grad_wk,
                       grad_wv);
    PYGAMD_LAUNCH_CHECK();
  }
  return PYGAMD_OK;
}

}  // extern "C"
