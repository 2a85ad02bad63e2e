// sage_fused_lp.hip — the one-kernel SAGE layer forward on float16 / bfloat16 storage
// (pygamd_sage_layer_lp):
//
//     out[i, :] = narrow( [ aggr_{j->i} x[j] | x[i] ] @ [W_l | W_r]^T + b )
//
// x, W_l, W_r, b and out share ONE 16-bit type T; sums and products are accumulated in float32.
// The aggregated row is rounded once (it is the 16-bit row pygamd_spmm_lp writes, bit for bit: the
// same accumulation code in the same order) and every output is rounded once.
//
// Schedule (wave64, 512 threads = 8 waves, one workgroup per tile of 32 destination rows):
//   LDS      the A tile [32][2 fh + 8] of T, fh = F rounded up to 16: columns [0, fh) hold the
//            aggregated row, [fh, 2 fh) the tile's own row, zeros past F in each half.  The row
//            pitch is fh + 4 dwords — an odd multiple of 16 bytes, so the ds_read_b128 fragment
//            reads of phase 2 (32 rows x 2 k-halves) meet no bank conflict.  2 bytes per element:
//            both halves of K are resident at once for every F <= 512 (66 KB at 512, 33 KB at
//            256), there is no second pass over K and no conversion work.
//   phase 1  the tile's own rows go global -> registers -> LDS in 16-byte pieces (loads issued
//            first); the waves then draw the tile's rows one by one from an LDS counter and
//            gather each with lp_accumulate (spmm_lp_device.h: 8 columns per lane, min(LPR, 8)
//            row loads in flight, float32 accumulators), fold the lane groups with the xor
//            butterfly of lp_sum_rows, apply 1 / deg for mean, round once (lp_narrow2) and write
//            the row to the tile and, when asked, write-only to the global agg buffer [N, F].
//            A hub row (degree above the plan's threshold) is not gathered here: its chunks are
//            summed to float32 partials by a launch in front of this one (one wave per chunk,
//            the same lp_accumulate) and the drawing wave adds the partials in chunk order — the
//            sum pygamd_spmm_lp's merge kernel forms, eight chunks' loads in flight as there —
//            before the one rounding.
//   phase 2  acc[32 x 32] per wave on v_mfma_f32_32x32x16_{bf16,f16}: wave w owns the output
//            columns [32 w, 32 w + 32), Fo > 256 takes a second column pass over the same resident
//            tile.  Per 16-k step one ds_read_b128 (A) and one 16-byte global load (B): lane
//            (j = lane & 31, h = lane >> 5) reads W[col0 + j][k0 + 8 h .. + 7] straight from the
//            16-bit weights (L2-resident; W_l for the aggregated half, W_r for the root half),
//            kept 4 steps ahead in a register ring.  No weight pre-pass and no workspace for
//            weights.  Two accumulators alternate so that consecutive matrix instructions are
//            independent.  Columns past Fo and k past F are predicated weight loads (zeros).
//   epilogue the bias widened once per column, one round-to-nearest-even per output, 2-byte
//            stores masked by row and column (a lane half writes 64 contiguous bytes of a row).
// No float atomics (the LDS row counter is an integer), grids from sizes only, no scratch.
//
// Known costs of this schedule, none measured apart:
//   * a wave owns 32 output columns, so only ceil(Fo / 32) of the 8 waves issue matrix
//     instructions: with Fo <= 64 one or two do and the rest wait at the end of the kernel, and
//     with 256 < Fo < 512 the second column pass runs on ceil(Fo / 32) - 8 waves.
//   * a hub row is merged by the LPR lanes of the one wave that drew it; the tile's other waves
//     go on drawing rows and then wait for it at the barrier in front of phase 2.
//
// Compiler resource report (hipcc -O3, gfx950; profiles/sage_layer_lp.md has the tables): the
// layer kernel takes 109 VGPRs, no AGPRs and no scratch in all 28 instantiations (the matrix phase
// sets the count) — 4 waves per SIMD, two workgroups per CU; LDS 128 (fh + 4) + 16 bytes (33 KB at
// F = 256, 66 KB at 512).  The chunk kernel: 23-84 VGPRs, no LDS, no scratch.
#include "common.h"

#include "spmm_lp_device.h"

namespace pygamd {

constexpr int kLBlock = 512;  // 8 waves
constexpr int kLWaves = kLBlock / kWave;
constexpr int kLTile = 32;    // destination rows per workgroup
constexpr int kLK = 16;       // k per matrix instruction
constexpr int kLRing = 4;     // weight fragments in flight per wave
constexpr int kLPieces = 4;   // 16-byte root pieces per thread: 32 rows x (F <= 512) / 8 / 512
constexpr int kLHubLoads = 8;  // chunk partials of a hub row in flight per lane (as lp_hub_sum)
constexpr size_t kLDefaultLds = 48 * 1024;  // dynamic LDS a launch may ask for without an attribute

typedef uint32_t lp_u32x4 __attribute__((ext_vector_type(4)));
typedef float lp_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 lp_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 lp_f16x8 __attribute__((ext_vector_type(8)));

template <typename IdxT>
struct SageLpArgs {
  LpDev<IdxT> g;  // the graph, x / ldx, F, mean, the hub plan and its partials; g.out: agg or null
  const uint16_t* __restrict__ wl;    // [Fo, F]
  const uint16_t* __restrict__ wr;    // [Fo, F]
  const uint16_t* __restrict__ bias;  // [Fo] or null
  uint16_t* __restrict__ y;           // [n_rows, ldy]
  int64_t ldy;
  int Fo, f_half;
};

inline int sage_lp_f_half(int64_t F) { return static_cast<int>(round_up(F, kLK)); }
inline size_t sage_lp_lds_bytes(int64_t F) {
  return sizeof(uint32_t) * kLTile * (sage_lp_f_half(F) + 4);
}

template <typename T>
__device__ __forceinline__ float lp_widen1(uint16_t bits) {
  if constexpr (__is_same(T, LpBf16)) {
    return __uint_as_float(static_cast<uint32_t>(bits) << 16);
  } else {
    return static_cast<float>(__builtin_bit_cast(_Float16, bits));
  }
}

template <typename T>
__device__ __forceinline__ lp_f32x16 lp_mfma(const lp_u32x4& a, const lp_u32x4& b,
                                             const lp_f32x16& c) {
  if constexpr (__is_same(T, LpBf16)) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(lp_bf16x8, a),
                                                   __builtin_bit_cast(lp_bf16x8, b), c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(lp_f16x8, a),
                                                  __builtin_bit_cast(lp_f16x8, b), c, 0, 0, 0);
  }
}

// the 64 / LPR lane groups of a wave folded in the order of lp_sum_rows (LPR, 2 LPR, .. 32)
template <int LPR>
__device__ __forceinline__ void lp_fold(float (&acc)[kLpCols]) {
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1) {
#pragma unroll
    for (int i = 0; i < kLpCols; ++i) acc[i] += __shfl_xor(acc[i], off, kWave);
  }
}

// One wave per chunk of the hub plan: its float32 partial [F] -> a.partial[chunk].  a.n_rows is 0
// here, so lp_item hands out chunks and nothing else.
template <typename T, typename IdxT, int LPR>
__global__ void __launch_bounds__(kBlock) sage_lp_hub_chunks(LpDev<IdxT> a) {
  const int lane = lane_id();
  LpItem<IdxT> it;
  if (!lp_item(a, it)) return;
  const int fo = (lane % LPR) * kLpCols;
  const uint32_t pm = fo < a.F ? 0xFFu : 0u;  // F % 8 == 0: a lane's 8 columns exist or do not
  float acc[kLpCols];
#pragma unroll
  for (int i = 0; i < kLpCols; ++i) acc[i] = 0.f;
  lp_accumulate<T, IdxT, kLpCols, LPR, false>(a, it.start, it.end, lane, fo, pm, acc);
  lp_fold<LPR>(acc);
  if (lane >= LPR || !pm) return;
  float* __restrict__ prow = a.partial + it.chunk * a.F + fo;
#pragma unroll
  for (int i = 0; i < kLpCols; ++i) prow[i] = acc[i];
}

// the aggregated row `row` (past n_rows: zeros) -> its 16-bit row of the A tile (+ the agg buffer)
template <typename T, typename IdxT, int LPR>
__device__ __forceinline__ void sage_lp_gather_row(const SageLpArgs<IdxT>& a, int64_t row,
                                                   uint32_t* __restrict__ trow, int lane) {
  const LpDev<IdxT>& g = a.g;
  const int fo = (lane % LPR) * kLpCols;
  const uint32_t pm = fo < g.F ? 0xFFu : 0u;
  float acc[kLpCols];
#pragma unroll
  for (int i = 0; i < kLpCols; ++i) acc[i] = 0.f;
  IdxT start = 0, end = 0;
  if (row < g.n_rows) {
    start = g.rowptr[row];
    end = g.rowptr[row + 1];
  }
  const IdxT deg = end - start;
  if (g.n_chunks > 0 && deg > g.hub_threshold) {  // (the test of lp_item)
    int64_t lo = 0, hi = g.n_hub;  // hub_rows ascends: hub_rows[lo] == row
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (static_cast<int64_t>(g.hub_rows[mid]) <= row) {
        lo = mid;
      } else {
        hi = mid;
      }
    }
    const int64_t c0 = g.hub_chunk_ptr[lo];
    int64_t c1 = g.hub_chunk_ptr[lo + 1];
    c1 = c1 < g.n_chunks ? c1 : g.n_chunks;
    if (lane < LPR && pm) {  // float32 partials added in chunk order, as lp_hub_sum adds them
      const float* __restrict__ prow = g.partial + c0 * g.F + fo;
      int64_t c = c0;
      for (; c + kLHubLoads <= c1; c += kLHubLoads) {  // eight chunks' loads in flight, as there
        float v[kLHubLoads][kLpCols];
#pragma unroll
        for (int u = 0; u < kLHubLoads; ++u) {
#pragma unroll
          for (int i = 0; i < kLpCols; ++i) v[u][i] = prow[u * g.F + i];
        }
#pragma unroll
        for (int u = 0; u < kLHubLoads; ++u) {
#pragma unroll
          for (int i = 0; i < kLpCols; ++i) acc[i] += v[u][i];
        }
        prow += kLHubLoads * g.F;
      }
      for (; c < c1; ++c, prow += g.F) {
#pragma unroll
        for (int i = 0; i < kLpCols; ++i) acc[i] += prow[i];
      }
    }
  } else {
    lp_accumulate<T, IdxT, kLpCols, LPR, false>(g, start, end, lane, fo, pm, acc);
    lp_fold<LPR>(acc);
  }
  if (lane >= LPR || !pm) return;
  if (g.mean) {
    const float cntf = static_cast<float>(deg > 0 ? deg : 1);
#pragma unroll
    for (int i = 0; i < kLpCols; ++i) acc[i] = acc[i] / cntf;
  }
  lp_u32x4 t;
  t.x = lp_narrow2<T>(acc[0], acc[1]);
  t.y = lp_narrow2<T>(acc[2], acc[3]);
  t.z = lp_narrow2<T>(acc[4], acc[5]);
  t.w = lp_narrow2<T>(acc[6], acc[7]);
  *reinterpret_cast<lp_u32x4*>(trow + (fo >> 1)) = t;
  if (g.out && row < g.n_rows)  // written once, read by the backward: kept out of the way in L2
    __builtin_nontemporal_store(t, reinterpret_cast<lp_u32x4*>(g.out + row * g.ldo + fo));
}

template <typename T, typename IdxT, int LPR>
__global__ void __launch_bounds__(kLBlock, 4) sage_lp_kernel(SageLpArgs<IdxT> a) {
  extern __shared__ __align__(16) uint32_t tile[];  // [32][fh + 4] dwords
  __shared__ int next_row;
  const int F = static_cast<int>(a.g.F);
  const int fh = a.f_half;
  const int row_dw = fh + 4;
  const int lane = lane_id();
  const int wave = wave_in_block();
  const int64_t row0 = xcd_logical_block() * kLTile;
  if (row0 >= a.g.n_rows) return;

  // ---- phase 1: the tile's own rows (loads first), then the gathered rows
  const int units = F / kLpCols;  // 16-byte pieces per row
  lp_u32x4 rr[kLPieces];
#pragma unroll
  for (int i = 0; i < kLPieces; ++i) {
    rr[i] = lp_u32x4{0u, 0u, 0u, 0u};
    const int t = threadIdx.x + i * kLBlock;
    const int r = t / units;
    const int u = t - r * units;
    int64_t row = row0 + r;
    row = row < a.g.n_rows ? row : a.g.n_rows - 1;  // (a tile row past the end: masked at the store)
    if (t < kLTile * units)
      rr[i] = *reinterpret_cast<const lp_u32x4*>(a.g.x + row * a.g.ldx + kLpCols * u);
  }
  if (threadIdx.x == 0) next_row = 0;
  if (fh > F && threadIdx.x < 2 * kLTile) {  // the 8 zero columns behind each half
    const int r = threadIdx.x >> 1, h = threadIdx.x & 1;
    *reinterpret_cast<lp_u32x4*>(tile + r * row_dw + ((h * fh + F) >> 1)) =
        lp_u32x4{0u, 0u, 0u, 0u};
  }
#pragma unroll
  for (int i = 0; i < kLPieces; ++i) {
    const int t = threadIdx.x + i * kLBlock;
    const int r = t / units;
    const int u = t - r * units;
    if (t < kLTile * units)
      *reinterpret_cast<lp_u32x4*>(tile + r * row_dw + ((fh + kLpCols * u) >> 1)) = rr[i];
  }
  __syncthreads();  // next_row armed
  for (;;) {
    int r = 0;
    if (lane == 0) r = atomicAdd(&next_row, 1);
    r = __builtin_amdgcn_readfirstlane(r);
    if (r >= kLTile) break;
    sage_lp_gather_row<T, IdxT, LPR>(a, row0 + r, tile + r * row_dw, lane);
  }
  __syncthreads();  // both halves of the tile visible to every wave

  // ---- phase 2: this wave's 32 x 32 blocks of columns [32 (wave + 8 p), + 32)
  const int li = lane & 31, lh = lane >> 5;
  const int steps = 2 * fh / kLK;
  const int last = steps - 1;
  const uint32_t* aq = tile + li * row_dw + 4 * lh;
  for (int col0 = wave * 32; col0 < a.Fo; col0 += kLWaves * 32) {
    const int col = col0 + li;
    const bool col_ok = col < a.Fo;
    // lane's 8 weights of step s: A-space columns 16 s + 8 h .. + 7 of output column `col`
    auto wfrag = [&](int s) -> lp_u32x4 {
      const int c = kLK * s + kLpCols * lh;
      const bool root = c >= fh;
      const int k = root ? c - fh : c;
      lp_u32x4 v = {0u, 0u, 0u, 0u};
      if (col_ok && k < F)
        v = *reinterpret_cast<const lp_u32x4*>((root ? a.wr : a.wl) +
                                               static_cast<int64_t>(col) * F + k);
      return v;
    };
    lp_u32x4 rb[kLRing];
#pragma unroll
    for (int q = 0; q < kLRing; ++q) rb[q] = wfrag(q < last ? q : last);
    lp_u32x4 fa = *reinterpret_cast<const lp_u32x4*>(aq);
    lp_f32x16 acc0, acc1;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc0[e] = acc1[e] = 0.f;
    for (int s = 0; s < steps; s += kLRing) {
#pragma unroll
      for (int q = 0; q < kLRing; ++q) {
        if (s + q < steps) {  // (uniform: steps is even, not always a multiple of the ring)
          const int sa = s + q + 1 < last ? s + q + 1 : last;
          const lp_u32x4 fan = *reinterpret_cast<const lp_u32x4*>(aq + sa * (kLK / 2));
          if (q & 1) {
            acc1 = lp_mfma<T>(fa, rb[q], acc1);
          } else {
            acc0 = lp_mfma<T>(fa, rb[q], acc0);
          }
          // the ring slot is refilled behind the instruction that read it (past the end: the last
          // step again, never used)
          const int sn = s + q + kLRing < last ? s + q + kLRing : last;
          rb[q] = wfrag(sn);
          fa = fan;
        }
      }
    }
    // ---- epilogue: acc[e] is row (e & 3) + 8 (e >> 2) + 4 h of the tile, column `col`
    const float bv = (a.bias && col_ok) ? lp_widen1<T>(a.bias[col]) : 0.f;
    const int64_t rbase = row0 + 4 * lh;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t row = rbase + (e & 3) + 8 * (e >> 2);
      const float v = acc0[e] + acc1[e] + bv;
      if (col_ok && row < a.g.n_rows) a.y[row * a.ldy + col] = lp_narrow<T>(v);
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------
struct SageLpCall {
  const pygamd_csr* g;
  const void* x;
  const void* wl;
  const void* wr;
  const void* bias;
  void* y;
  void* agg;
  int64_t ldx, ldy, F, Fo;
  int reduce;
  void* workspace;
  hipStream_t st;
};

template <typename T, typename IdxT, int LPR>
static int sage_lp_launch(const SageLpCall& c) {
  const pygamd_csr* g = c.g;
  SageLpArgs<IdxT> a = {};
  a.g.rowptr = static_cast<const IdxT*>(g->rowptr);
  a.g.col = static_cast<const IdxT*>(g->col);
  a.g.x = static_cast<const uint16_t*>(c.x);
  a.g.out = static_cast<uint16_t*>(c.agg);
  a.g.n_rows = g->n_rows;
  a.g.F = c.F;
  a.g.ldx = c.ldx;
  a.g.ldo = c.F;
  a.g.mean = c.reduce == PYGAMD_MEAN;
  const bool hubs = g->n_hub > 0;
  if (hubs) {
    a.g.hub_rows = static_cast<const IdxT*>(g->hub_rows);
    a.g.hub_chunk_ptr = static_cast<const IdxT*>(g->hub_chunk_ptr);
    a.g.n_hub = g->n_hub;
    a.g.n_chunks = g->n_chunks;
  }
  a.g.hub_threshold = g->hub_threshold;
  a.g.hub_chunk = g->hub_chunk;
  a.g.partial = static_cast<float*>(c.workspace);
  a.wl = static_cast<const uint16_t*>(c.wl);
  a.wr = static_cast<const uint16_t*>(c.wr);
  a.bias = static_cast<const uint16_t*>(c.bias);
  a.y = static_cast<uint16_t*>(c.y);
  a.ldy = c.ldy;
  a.Fo = static_cast<int>(c.Fo);
  a.f_half = sage_lp_f_half(c.F);
  if (hubs) {
    LpDev<IdxT> chunks = a.g;
    chunks.n_rows = 0;
    hipLaunchKernelGGL((sage_lp_hub_chunks<T, IdxT, LPR>), dim3(wave_grid(a.g.n_chunks)),
                       dim3(kBlock), 0, c.st, chunks);
    PYGAMD_LAUNCH_CHECK();
  }
  const size_t lds = sage_lp_lds_bytes(c.F);
  void (*k)(SageLpArgs<IdxT>) = sage_lp_kernel<T, IdxT, LPR>;
  if (lds > kLDefaultLds)  // F > 368 only: the common widths make no host call but the launch
    PYGAMD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k),
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         static_cast<int>(lds)));
  const unsigned grid = static_cast<unsigned>(round_up(ceil_div(g->n_rows, kLTile), 8));
  hipLaunchKernelGGL(k, dim3(grid), dim3(kLBlock), lds, c.st, a);
  PYGAMD_LAUNCH_CHECK();
  return PYGAMD_OK;
}

template <typename T, typename IdxT>
static int sage_lp_launch_lanes(const SageLpCall& c) {
  const int64_t units = c.F / kLpCols;  // LPR = next_pow2(F / 8): the lanes of pygamd_spmm_lp
  if (units <= 1) return sage_lp_launch<T, IdxT, 1>(c);
  if (units <= 2) return sage_lp_launch<T, IdxT, 2>(c);
  if (units <= 4) return sage_lp_launch<T, IdxT, 4>(c);
  if (units <= 8) return sage_lp_launch<T, IdxT, 8>(c);
  if (units <= 16) return sage_lp_launch<T, IdxT, 16>(c);
  if (units <= 32) return sage_lp_launch<T, IdxT, 32>(c);
  return sage_lp_launch<T, IdxT, 64>(c);
}

}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_sage_layer_lp_supported(int dtype, int64_t F, int64_t Fo, int reduce) {
  return (dtype == PYGAMD_DTYPE_F16 || dtype == PYGAMD_DTYPE_BF16) && F >= 8 && F <= 512 &&
         F % 8 == 0 && Fo >= 1 && Fo <= 512 && (reduce == PYGAMD_SUM || reduce == PYGAMD_MEAN);
}

size_t pygamd_sage_layer_lp_workspace_size(const pygamd_csr* g, int64_t F) {
  if (!g || g->n_hub <= 0 || g->n_chunks <= 0 || F <= 0) return 0;
  return static_cast<size_t>(g->n_chunks) * static_cast<size_t>(F) * sizeof(float);
}

int pygamd_sage_layer_lp(const pygamd_csr* g, const void* x, int64_t ldx, const void* w_l,
                         const void* w_r, const void* bias, void* out, int64_t ldo, void* agg,
                         int dtype, int64_t F, int64_t Fo, int reduce, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (!g) return PYGAMD_ERR_INVALID_ARG;
  if (g->idx_dtype != PYGAMD_IDX_I32 && g->idx_dtype != PYGAMD_IDX_I64)
    return PYGAMD_ERR_INVALID_ARG;
  if (g->n_rows < 0 || F < 0 || Fo < 0) return PYGAMD_ERR_INVALID_ARG;
  if (!pygamd_sage_layer_lp_supported(dtype, F, Fo, reduce)) return PYGAMD_ERR_UNSUPPORTED;
  if (ldx < F || ldo < Fo || ldx % kLpCols != 0) return PYGAMD_ERR_INVALID_ARG;
  if (g->n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !x || !w_l || !w_r || !out) return PYGAMD_ERR_INVALID_ARG;
  const uintptr_t p16 = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w_l) |
                        reinterpret_cast<uintptr_t>(w_r) | reinterpret_cast<uintptr_t>(agg);
  const uintptr_t p2 = reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(bias);
  if ((p16 & 15u) != 0 || (p2 & 1u) != 0) return PYGAMD_ERR_INVALID_ARG;
  if (g->n_hub > 0 && (!g->hub_rows || !g->hub_chunk_ptr || g->hub_chunk < 1 ||
                       g->hub_threshold < 1 || g->n_chunks < g->n_hub))
    return PYGAMD_ERR_INVALID_ARG;
  if (g->n_hub <= 0 && g->n_chunks != 0) return PYGAMD_ERR_INVALID_ARG;
  const size_t need = pygamd_sage_layer_lp_workspace_size(g, F);
  if (need > 0 && (!workspace || workspace_bytes < need ||
                   (reinterpret_cast<uintptr_t>(workspace) & 3u) != 0))
    return PYGAMD_ERR_WORKSPACE;
  SageLpCall c = {g, x, w_l, w_r, bias, out, agg, ldx, ldo, F, Fo, reduce, workspace,
                  as_stream(stream)};
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    return dtype == PYGAMD_DTYPE_BF16 ? sage_lp_launch_lanes<LpBf16, IdxT>(c)
                                      : sage_lp_launch_lanes<LpHalf, IdxT>(c);
  });
}

}  // extern "C"
