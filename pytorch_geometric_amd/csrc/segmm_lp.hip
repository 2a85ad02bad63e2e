// segmm_lp.hip — segment_matmul (grouped GEMM over row segments) on float16 / bfloat16 storage
// (pygamd_segment_matmul_lp, pygamd_segment_matmul_lp_wgrad):
//
//     out[seg] = narrow( x[seg] @ W[g] )                 (forward; with W^T: the input gradient)
//     grad_W[g] = narrow( x[seg]^T @ grad[seg] )         (weight gradient)
//
// x, W, out / grad share ONE 16-bit type T; products are exact in float32, sums are accumulated in
// float32 by v_mfma_f32_32x32x16_{f16,bf16} and every output is rounded once, to nearest even.
// No term planes, no weight pre-pass, no float atomics: half the operand bytes of csrc/segmm.hip
// and none of the conversion work of its split path.
//
// Both kernels share one schedule (wave64, 256 threads = 2 x 2 waves, each 64 x 64 outputs in four
// 32 x 32 accumulators; a workgroup owns a 128 x 128 output tile):
//   LDS      two operand images [128][64 + 8] of T, one per matrix operand, BOTH "reduction-minor":
//            row i of an image holds 64 consecutive reduction elements of output row (A) or output
//            column (B) i.  That is the operand order of the matrix instruction — lane
//            (i = lane & 31, h = lane >> 5) supplies the 8 consecutive k = 16 s + 8 h .. + 7 of row
//            / column i — so a fragment is ONE ds_read_b128.  The pitch is 72 elements = 144
//            bytes, an odd multiple of 16 bytes: the 16 lanes of a ds_read_b128 phase (16
//            consecutive rows, one k-half) start at banks 36 i mod 64 = sixteen different
//            multiples of 4 and meet no conflict.  36,864 bytes per workgroup.
//   staging  global -> registers -> LDS in 8-element pieces, two shapes chosen per launch from the
//            operand's strides:
//              direct      the source is reduction-contiguous (x of the product; W^T of the input
//                          gradient, read where it lies through swapped strides): a piece already
//                          IS a fragment half, stored with one ds_write_b128.  Thread -> (k-group
//                          tid % 8, rows tid / 8 + 32 q): 8 lanes cover 128 contiguous bytes.
//              transposed  the source is [reduction][column], column-contiguous (W of the forward;
//                          x and grad of the weight gradient, which reduces along rows): a thread
//                          loads 4 consecutive reduction rows x 8 columns, transposes the 4 x 8
//                          block in registers (and / shift / or pairs) and stores 8 ds_write_b64.
//                          Lane -> (reduction quad lane % 16, column group 4 wave + lane / 16): the
//                          16 quads of a store cover 32 different banks and the 4 column groups
//                          fold onto them twice — 128 dwords through 64 banks, the minimum.
//            The next chunk's pieces are loaded into registers before the matrix instructions of
//            the current one are issued (and g_rows, the gathered gradient rows' index, one chunk
//            further ahead), as csrc/segmm.hip does.
//   widths   VW, per launch as in csrc/spmm_lp.hip: 8 (16-byte loads) when base pointers and
//            pitches are 16-byte aligned and the contiguous extent is a multiple of 8; 2 (4-byte
//            loads) when all of that holds for 4 bytes / multiples of 2 — K = N = 100, the
//            FB15k-237 layer; 1 (2-byte loads) otherwise, e.g. a column slice that starts at an odd
//            element.  A piece past the end of its row, a reduction element past K (or past the
//            chunk) is a predicated load that yields zeros; nothing is read past a row.
//   epilogue reg e of lane l is D[(e & 3) + 8 (e >> 2) + 4 (l >> 5)][l & 31]: 2-byte stores, a
//            lane half writes 64 contiguous bytes of a row (any alignment of out).  out_rows
//            sends row s to out[out_rows[s]].
// Weight gradient: a workgroup owns (row chunk of a segment) x (128 x 128 of grad_W) and writes a
// float32 partial [K, N] per chunk into the workspace; a merge kernel adds the partials of each
// group in chunk-table order and rounds once.  Every partial element is written by exactly one
// lane, so nothing is zeroed first and the result is bit-identical from run to run.
//
// Compiler resource report (hipcc -O3, gfx950), no scratch in any instantiation: the product kernel
// takes 84-88 VGPRs + 64 AGPRs (the four accumulators), the weight-gradient kernel 88-90 + 64 —
// 3 waves per SIMD, 36,864 bytes of LDS; the merge kernel 8 VGPRs, no LDS, 8 waves per SIMD.
// profiles/segmm_lp.md has the table per instantiation and the timings.
#include "common.h"

#include "spmm_lp_device.h"

namespace pygamd {

typedef uint32_t sg_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t sg_u32x2 __attribute__((ext_vector_type(2)));
typedef float sg_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 sg_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 sg_f16x8 __attribute__((ext_vector_type(8)));

constexpr int kGT = 128;        // rows / columns of an output tile (= pygamd_segment_matmul_tile_rows)
constexpr int kGK = 64;         // reduction elements staged per chunk
constexpr int kGP = kGK + 8;    // LDS pitch in elements: 144 bytes
constexpr int kGQ = kGT / 32;   // pieces per thread and operand: 128 x 64 / 8 / 256
constexpr int64_t kGMaxDim = int64_t{1} << 22;   // K, N: ceil(. / 128) fits a grid dimension

template <typename T>
__device__ __forceinline__ sg_f32x16 sg_mfma(const sg_u32x4& a, const sg_u32x4& b,
                                             const sg_f32x16& c) {
  if constexpr (__is_same(T, LpBf16)) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(sg_bf16x8, a),
                                                   __builtin_bit_cast(sg_bf16x8, b), c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sg_f16x8, a),
                                                  __builtin_bit_cast(sg_f16x8, b), c, 0, 0, 0);
  }
}

// elements [0, cnt) of the 8 at p, zeros behind them; cnt <= 0 reads nothing (p may point anywhere).
// VW 8: cnt is 0 or 8; VW 2: cnt is even.
template <int VW>
__device__ __forceinline__ sg_u32x4 sg_ld8(const uint16_t* __restrict__ p, int cnt) {
  sg_u32x4 v = {0u, 0u, 0u, 0u};
  if constexpr (VW == 8) {
    if (cnt >= 8) v = *reinterpret_cast<const sg_u32x4*>(p);
  } else if constexpr (VW == 2) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (cnt >= 2 * q + 2) v[q] = *reinterpret_cast<const uint32_t*>(p + 2 * q);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < cnt) v[i >> 1] |= static_cast<uint32_t>(p[i]) << (16 * (i & 1));
  }
  return v;
}

// how many of the 8 elements from `at` lie below `end`
__device__ __forceinline__ int sg_left(int end, int at) {
  const int left = end - at;
  return left > 8 ? 8 : left;
}

// The thread's slots of the two staging shapes (see the header): direct -> image row dr + 32 q,
// elements [8 dg, 8 dg + 8); transposed -> reduction elements 4 tq + q, image rows 8 tc .. 8 tc + 7.
struct SgSlots {
  int dg, dr, tq, tc;
};
__device__ __forceinline__ SgSlots sg_slots() {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  return {static_cast<int>(threadIdx.x & 7), static_cast<int>(threadIdx.x >> 3), lane & 15,
          4 * wave + (lane >> 4)};
}

__device__ __forceinline__ void sg_store_direct(uint16_t* img, const SgSlots& s,
                                                const sg_u32x4 (&v)[kGQ]) {
#pragma unroll
  for (int q = 0; q < kGQ; ++q)
    *reinterpret_cast<sg_u32x4*>(img + (s.dr + 32 * q) * kGP + 8 * s.dg) = v[q];
}

// v[q] = 8 columns of reduction element 4 tq + q -> column c's four elements, one 8-byte store
__device__ __forceinline__ void sg_store_transposed(uint16_t* img, const SgSlots& s,
                                                    const sg_u32x4 (&v)[kGQ]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    sg_u32x2 o;
    if (c & 1) {
      o[0] = (v[0][c >> 1] >> 16) | (v[1][c >> 1] & 0xFFFF0000u);
      o[1] = (v[2][c >> 1] >> 16) | (v[3][c >> 1] & 0xFFFF0000u);
    } else {
      o[0] = (v[0][c >> 1] & 0xFFFFu) | (v[1][c >> 1] << 16);
      o[1] = (v[2][c >> 1] & 0xFFFFu) | (v[3][c >> 1] << 16);
    }
    *reinterpret_cast<sg_u32x2*>(img + (8 * s.tc + c) * kGP + 4 * s.tq) = o;
  }
}

// this wave's 64 x 64 piece of the staged chunk: `steps` 16-element steps hold data; a0 / a1 (b0 /
// b1): the wave's first / second 32 rows (columns) exist at all (wave-uniform)
template <typename T>
__device__ __forceinline__ void sg_chunk_mma(const uint16_t* As, const uint16_t* Bs, int wm, int wn,
                                             int steps, bool a1, bool b1, sg_f32x16 (&acc)[2][2]) {
  const int lane = lane_id();
  const uint16_t* fa = As + (wm * 64 + (lane & 31)) * kGP + 8 * (lane >> 5);
  const uint16_t* fb = Bs + (wn * 64 + (lane & 31)) * kGP + 8 * (lane >> 5);
#pragma unroll
  for (int s = 0; s < kGK / 16; ++s) {
    if (s < steps) {   // scalar guard: no matrix work on the reduction padding
      const sg_u32x4 va0 = *reinterpret_cast<const sg_u32x4*>(fa + 16 * s);
      const sg_u32x4 vb0 = *reinterpret_cast<const sg_u32x4*>(fb + 16 * s);
      acc[0][0] = sg_mfma<T>(va0, vb0, acc[0][0]);
      sg_u32x4 vb1 = {0u, 0u, 0u, 0u};
      if (b1) {
        vb1 = *reinterpret_cast<const sg_u32x4*>(fb + 32 * kGP + 16 * s);
        acc[0][1] = sg_mfma<T>(va0, vb1, acc[0][1]);
      }
      if (a1) {
        const sg_u32x4 va1 = *reinterpret_cast<const sg_u32x4*>(fa + 32 * kGP + 16 * s);
        acc[1][0] = sg_mfma<T>(va1, vb0, acc[1][0]);
        if (b1) acc[1][1] = sg_mfma<T>(va1, vb1, acc[1][1]);
      }
    }
  }
}

__device__ __forceinline__ void sg_zero(sg_f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}

// ---- product: out[seg] = x[seg] @ W[g] -----------------------------------------------------------
// WT: W is k-contiguous (w[g * w_seg + n * w_ld + k]: the input gradient's W^T) and staged
// directly; otherwise n-contiguous (w[g * w_seg + k * w_ld + n]) and staged transposed.
template <typename T, int VW, bool WT>
__global__ void __launch_bounds__(kBlock)
    segmm_lp_kernel(const uint16_t* __restrict__ x, int64_t ldx, const int64_t* __restrict__ x_rows,
                    const uint16_t* __restrict__ w, int64_t w_seg, int64_t w_ld,
                    const int32_t* __restrict__ tiles, int K, int N, int blocks,
                    uint16_t* __restrict__ out, int64_t ldo, const int64_t* __restrict__ out_rows) {
  __shared__ __align__(16) uint16_t As[kGT * kGP];
  __shared__ __align__(16) uint16_t Bs[kGT * kGP];
  const int t = blockIdx.x;
  const int seg = tiles[3 * t];
  const int64_t row0 = tiles[3 * t + 1];
  const int rows = tiles[3 * t + 2] < kGT ? tiles[3 * t + 2] : kGT;
  if (rows <= 0) return;   // (the whole workgroup: nothing to read, x_rows included)
  const int n0 = blockIdx.y * kGT;
  const int wave = wave_in_block(), lane = lane_id();
  const int wm = wave >> 1, wn = wave & 1;
  // block-diagonal weights: group seg = relation * blocks + b works on column block b
  const int blk = blocks > 1 ? seg % blocks : 0;
  x += static_cast<int64_t>(blk) * K;
  out += static_cast<int64_t>(blk) * N;
  w += static_cast<int64_t>(seg) * w_seg;
  const SgSlots s = sg_slots();
  // A pieces: the thread's four operand rows (x_rows: gathered on the fly), k-group s.dg
  const uint16_t* pa[kGQ];
  bool a_ok[kGQ];
#pragma unroll
  for (int q = 0; q < kGQ; ++q) {
    const int r = s.dr + 32 * q;
    a_ok[q] = r < rows;
    const int64_t rr = row0 + (a_ok[q] ? r : 0);
    pa[q] = x + (x_rows ? x_rows[rr] : rr) * ldx + 8 * s.dg;
  }
  sg_u32x4 a_nx[kGQ], b_nx[kGQ];
  auto prefetch = [&](int k0) {
    const int ka = sg_left(K, k0 + 8 * s.dg);
#pragma unroll
    for (int q = 0; q < kGQ; ++q) a_nx[q] = sg_ld8<VW>(pa[q] + k0, a_ok[q] ? ka : 0);
    if constexpr (WT) {
#pragma unroll
      for (int q = 0; q < kGQ; ++q) {
        const int n = n0 + s.dr + 32 * q;
        b_nx[q] = sg_ld8<VW>(w + static_cast<int64_t>(n) * w_ld + k0 + 8 * s.dg, n < N ? ka : 0);
      }
    } else {
      const int nb = sg_left(N, n0 + 8 * s.tc);
#pragma unroll
      for (int q = 0; q < kGQ; ++q) {
        const int k = k0 + 4 * s.tq + q;
        b_nx[q] = sg_ld8<VW>(w + static_cast<int64_t>(k) * w_ld + n0 + 8 * s.tc, k < K ? nb : 0);
      }
    }
  };
  sg_f32x16 acc[2][2];
  sg_zero(acc);
  // wave-uniform: which 32-wide halves of this wave's rows / columns exist
  const bool ra0 = wm * 64 < rows, ra1 = wm * 64 + 32 < rows;
  const bool cb0 = n0 + wn * 64 < N, cb1 = n0 + wn * 64 + 32 < N;
  prefetch(0);
  for (int k0 = 0; k0 < K; k0 += kGK) {
    sg_store_direct(As, s, a_nx);
    if constexpr (WT) {
      sg_store_direct(Bs, s, b_nx);
    } else {
      sg_store_transposed(Bs, s, b_nx);
    }
    __syncthreads();
    if (k0 + kGK < K) prefetch(k0 + kGK);   // in flight during the matrix instructions below
    if (ra0 && cb0) sg_chunk_mma<T>(As, Bs, wm, wn, (K - k0 + 15) >> 4, ra1, cb1, acc);
    __syncthreads();
  }
  if (!(ra0 && cb0)) return;
  const int col0 = n0 + wn * 64 + (lane & 31), col1 = col0 + 32;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = wm * 64 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
      if (r < rows) {
        const int64_t ro = out_rows ? out_rows[row0 + r] : row0 + r;
        uint16_t* __restrict__ orow = out + ro * ldo;
        if (col0 < N) orow[col0] = lp_narrow<T>(acc[i][0][e]);
        if (col1 < N) orow[col1] = lp_narrow<T>(acc[i][1][e]);
      }
    }
  }
}

// ---- weight gradient: partial[chunk] = x[chunk]^T @ grad[chunk] ------------------------------------
// The reduction runs along rows: both operands are staged transposed.  grid = (chunks, K tiles, N
// tiles); partial is [n_chunks, K, N] float32, every element written by exactly one lane.
template <typename T, int VW>
__global__ void __launch_bounds__(kBlock)
    segmm_lp_wgrad_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                          const int64_t* __restrict__ x_rows, const uint16_t* __restrict__ g,
                          int64_t ldg, const int64_t* __restrict__ g_rows, const int32_t* __restrict__ chunks,
                          int K, int N, int blocks, float* __restrict__ partial) {
  __shared__ __align__(16) uint16_t Xs[kGT * kGP];
  __shared__ __align__(16) uint16_t Gs[kGT * kGP];
  const int c = blockIdx.x;
  const int seg = chunks[3 * c];
  const int64_t ra = chunks[3 * c + 1];
  const int64_t rb = ra + chunks[3 * c + 2];
  const int kt0 = blockIdx.y * kGT, n0 = blockIdx.z * kGT;
  const int wave = wave_in_block(), lane = lane_id();
  const int wk = wave >> 1, wn = wave & 1;
  const int blk = blocks > 1 ? seg % blocks : 0;
  x += static_cast<int64_t>(blk) * K + kt0;
  g += static_cast<int64_t>(blk) * N + n0;
  const SgSlots s = sg_slots();
  const int kx = sg_left(K, kt0 + 8 * s.tc), ng = sg_left(N, n0 + 8 * s.tc);
  sg_u32x4 x_nx[kGQ], g_nx[kGQ];
  int64_t xi[kGQ], gi[kGQ];
  // the gathered rows' indices, loaded one chunk ahead of the row loads that depend on it (past the
  // end it re-reads the chunk's first row: never used)
  auto load_index = [&](int64_t r) {
#pragma unroll
    for (int q = 0; q < kGQ; ++q) {
      const int64_t rr = r + 4 * s.tq + q;
      const int64_t rs = rr < rb ? rr : ra;
      xi[q] = (x_rows && ra < rb) ? x_rows[rs] : rs;
      gi[q] = (g_rows && ra < rb) ? g_rows[rs] : rs;
    }
  };
  auto prefetch = [&](int64_t r) {
#pragma unroll
    for (int q = 0; q < kGQ; ++q) {
      const int64_t rr = r + 4 * s.tq + q;
      const bool ok = rr < rb;
      x_nx[q] = sg_ld8<VW>(x + xi[q] * ldx + 8 * s.tc, ok ? kx : 0);
      g_nx[q] = sg_ld8<VW>(g + gi[q] * ldg + 8 * s.tc, ok ? ng : 0);
    }
    load_index(r + kGK);
  };
  sg_f32x16 acc[2][2];
  sg_zero(acc);
  const bool ka0 = kt0 + wk * 64 < K, ka1 = kt0 + wk * 64 + 32 < K;
  const bool cb0 = n0 + wn * 64 < N, cb1 = n0 + wn * 64 + 32 < N;
  load_index(ra);
  prefetch(ra);
  for (int64_t r = ra; r < rb; r += kGK) {
    sg_store_transposed(Xs, s, x_nx);
    sg_store_transposed(Gs, s, g_nx);
    __syncthreads();
    if (r + kGK < rb) prefetch(r + kGK);   // in flight during the matrix instructions below
    const int64_t left = rb - r;
    if (ka0 && cb0)
      sg_chunk_mma<T>(Xs, Gs, wk, wn, left >= kGK ? kGK / 16 : static_cast<int>((left + 15) >> 4),
                      ka1, cb1, acc);
    __syncthreads();
  }
  if (!(ka0 && cb0)) return;
  float* __restrict__ pc = partial + static_cast<int64_t>(c) * K * N;
  const int col0 = n0 + wn * 64 + (lane & 31), col1 = col0 + 32;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int kr = kt0 + wk * 64 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
      if (kr < K) {
        if (col0 < N) pc[static_cast<int64_t>(kr) * N + col0] = acc[i][0][e];
        if (col1 < N) pc[static_cast<int64_t>(kr) * N + col1] = acc[i][1][e];
      }
    }
  }
}

// grad_w[grp] = narrow( sum of the partials of grp's chunks, in chunk-table order ); a group
// without chunks gives 0.  The table lists the chunks by non-decreasing segment (= group / blocks):
// the workgroup finds its segment's first chunk by bisection (scalar) and walks to its last.
template <typename T>
__global__ void __launch_bounds__(kBlock)
    segmm_lp_merge_kernel(const float* __restrict__ partial, const int32_t* __restrict__ chunks,
                          int n_chunks, int blocks, int64_t KN, uint16_t* __restrict__ gw) {
  const int grp = blockIdx.x;
  const int seg = grp / blocks;
  int lo = 0, hi = n_chunks;   // first chunk whose segment is >= seg
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (chunks[3 * mid] / blocks < seg) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  for (int64_t e = static_cast<int64_t>(blockIdx.y) * kBlock + threadIdx.x; e < KN;
       e += static_cast<int64_t>(gridDim.y) * kBlock) {
    float acc = 0.f;
    for (int c = lo; c < n_chunks; ++c) {
      const int gc = chunks[3 * c];
      if (gc / blocks != seg) break;
      if (gc == grp) acc += partial[static_cast<int64_t>(c) * KN + e];
    }
    gw[static_cast<int64_t>(grp) * KN + e] = lp_narrow<T>(acc);
  }
}

// widest access (8, 2 or 1 elements) that base pointer, pitches and the contiguous extent allow
static int sg_width(const void* p, int64_t extent, int64_t pitch0, int64_t pitch1) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (a % 16 == 0 && extent % 8 == 0 && pitch0 % 8 == 0 && pitch1 % 8 == 0) return 8;
  if (a % 4 == 0 && extent % 2 == 0 && pitch0 % 2 == 0 && pitch1 % 2 == 0) return 2;
  return 1;
}

// the tile table is cut for pygamd_segment_matmul_tile_rows() rows (csrc/segmm.hip); the kernels
// here own kGT of them and would drop the rest of a taller tile
static bool sg_tiles_fit() { return pygamd_segment_matmul_tile_rows() <= kGT; }

static bool sg_dims_ok(int dtype, int64_t K, int64_t N) {
  return (dtype == PYGAMD_DTYPE_F16 || dtype == PYGAMD_DTYPE_BF16) && K >= 1 && K <= kGMaxDim &&
         N >= 1 && N <= kGMaxDim;
}

struct SgCall {
  const uint16_t* x;
  int64_t ldx;
  const int64_t* x_rows;
  const uint16_t* w;
  int64_t w_seg, w_ld;
  const int32_t* tiles;
  int64_t n_tiles;
  int K, N, blocks;
  uint16_t* out;
  int64_t ldo;
  const int64_t* out_rows;
  hipStream_t st;
};

template <typename T, int VW, bool WT>
static int sg_launch(const SgCall& c) {
  const dim3 grid(static_cast<unsigned>(c.n_tiles), static_cast<unsigned>(ceil_div(c.N, kGT)));
  hipLaunchKernelGGL((segmm_lp_kernel<T, VW, WT>), grid, dim3(kBlock), 0, c.st, c.x, c.ldx,
                     c.x_rows, c.w, c.w_seg, c.w_ld, c.tiles, c.K, c.N, c.blocks, c.out, c.ldo,
                     c.out_rows);
  PYGAMD_LAUNCH_CHECK();
  return PYGAMD_OK;
}

template <typename T, bool WT>
static int sg_launch_width(const SgCall& c, int vw) {
  if (vw == 8) return sg_launch<T, 8, WT>(c);
  if (vw == 2) return sg_launch<T, 2, WT>(c);
  return sg_launch<T, 1, WT>(c);
}

template <typename T>
static int sg_wgrad_launch(const uint16_t* x, int64_t ldx, const int64_t* x_rows,
                           const uint16_t* g, int64_t ldg, const int64_t* g_rows, const int32_t* chunks, int64_t n_chunks,
                           int64_t n_seg, int K, int N, int blocks, uint16_t* gw, float* partial,
                           hipStream_t st) {
  if (n_chunks > 0) {
    const int vx = sg_width(x, K, ldx, 8), vg = sg_width(g, N, ldg, 8);
    const int vw = vx < vg ? vx : vg;
    const dim3 grid(static_cast<unsigned>(n_chunks), static_cast<unsigned>(ceil_div(K, kGT)),
                    static_cast<unsigned>(ceil_div(N, kGT)));
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, st, x, ldx, x_rows, g, ldg, g_rows, chunks,
                         K, N, blocks, partial);
    };
    if (vw == 8) {
      launch(segmm_lp_wgrad_kernel<T, 8>);
    } else if (vw == 2) {
      launch(segmm_lp_wgrad_kernel<T, 2>);
    } else {
      launch(segmm_lp_wgrad_kernel<T, 1>);
    }
    PYGAMD_LAUNCH_CHECK();
  }
  const int64_t KN = static_cast<int64_t>(K) * N;
  const int64_t per_group = ceil_div(KN, kBlock);
  const dim3 mgrid(static_cast<unsigned>(n_seg),
                   static_cast<unsigned>(per_group < 65535 ? per_group : 65535));
  hipLaunchKernelGGL(segmm_lp_merge_kernel<T>, mgrid, dim3(kBlock), 0, st, partial, chunks,
                     static_cast<int>(n_chunks), blocks, KN, gw);
  PYGAMD_LAUNCH_CHECK();
  return PYGAMD_OK;
}

}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_segment_matmul_lp_supported(int dtype, int64_t K, int64_t N) {
  return sg_dims_ok(dtype, K, N) ? 1 : 0;
}

int pygamd_segment_matmul_lp(const void* x, int dtype, int64_t ldx, const int64_t* x_rows,
                             const void* w, int64_t w_seg_stride, int64_t w_stride_k,
                             int64_t w_stride_n, int64_t n_groups, const int32_t* tiles,
                             int64_t n_tiles, int64_t K, int64_t N, int64_t blocks, void* out,
                             int64_t ldo, const int64_t* out_rows, void* stream) {
  if (n_tiles < 0 || n_tiles > INT32_MAX || n_groups < 0 || K < 0 || N < 0 || blocks < 1 ||
      blocks > INT32_MAX || ldx < 0 || ldo < 0 || w_seg_stride < 0 || w_stride_k < 0 ||
      w_stride_n < 0)
    return PYGAMD_ERR_INVALID_ARG;
  if (dtype != PYGAMD_DTYPE_F16 && dtype != PYGAMD_DTYPE_BF16) return PYGAMD_ERR_UNSUPPORTED;
  if (n_tiles == 0 || N == 0) return PYGAMD_OK;
  if (!sg_dims_ok(dtype, K, N) || !sg_tiles_fit()) return PYGAMD_ERR_UNSUPPORTED;
  if (ldx < blocks * K || ldo < blocks * N) return PYGAMD_ERR_INVALID_ARG;
  if (!x || !w || !tiles || !out) return PYGAMD_ERR_INVALID_ARG;
  // one of the weight's two strides is 1: the other is the pitch of the staged rows
  const bool wt = w_stride_n != 1;
  if (wt && w_stride_k != 1) return PYGAMD_ERR_UNSUPPORTED;
  const int64_t w_ld = wt ? w_stride_n : w_stride_k;
  if (w_ld < (wt ? K : N)) return PYGAMD_ERR_INVALID_ARG;
  const int vx = sg_width(x, K, ldx, 8);
  const int vw_w = sg_width(w, wt ? K : N, w_ld, w_seg_stride);
  const int vw = vx < vw_w ? vx : vw_w;
  const SgCall c{static_cast<const uint16_t*>(x), ldx, x_rows, static_cast<const uint16_t*>(w),
                 w_seg_stride, w_ld, tiles, n_tiles, static_cast<int>(K), static_cast<int>(N),
                 static_cast<int>(blocks), static_cast<uint16_t*>(out), ldo, out_rows,
                 as_stream(stream)};
  if (dtype == PYGAMD_DTYPE_BF16)
    return wt ? sg_launch_width<LpBf16, true>(c, vw) : sg_launch_width<LpBf16, false>(c, vw);
  return wt ? sg_launch_width<LpHalf, true>(c, vw) : sg_launch_width<LpHalf, false>(c, vw);
}

size_t pygamd_segment_matmul_lp_wgrad_workspace_size(int64_t n_chunks, int64_t K, int64_t N) {
  if (n_chunks <= 0 || K <= 0 || N <= 0) return 0;
  return sizeof(float) * static_cast<size_t>(n_chunks) * static_cast<size_t>(K) *
         static_cast<size_t>(N);
}

int pygamd_segment_matmul_lp_wgrad(const void* x, int64_t ldx, const int64_t* x_rows,
                                   const void* g, int64_t ldg, const int64_t* g_rows, const int32_t* chunks, int64_t n_chunks,
                                   int64_t n_seg, int64_t K, int64_t N, int64_t blocks, int dtype,
                                   void* grad_w, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  if (n_seg < 0 || n_seg > INT32_MAX || n_chunks < 0 || n_chunks > INT32_MAX || K < 0 || N < 0 ||
      blocks < 1 || blocks > INT32_MAX || ldx < 0 || ldg < 0)
    return PYGAMD_ERR_INVALID_ARG;
  if (dtype != PYGAMD_DTYPE_F16 && dtype != PYGAMD_DTYPE_BF16) return PYGAMD_ERR_UNSUPPORTED;
  if (n_seg == 0 || K == 0 || N == 0) return PYGAMD_OK;
  if (!sg_dims_ok(dtype, K, N)) return PYGAMD_ERR_UNSUPPORTED;
  if (ldx < blocks * K || ldg < blocks * N) return PYGAMD_ERR_INVALID_ARG;
  if (!grad_w) return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0) {
    if (!x || !g || !chunks || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 3u) != 0)
      return PYGAMD_ERR_INVALID_ARG;
    if (workspace_bytes < pygamd_segment_matmul_lp_wgrad_workspace_size(n_chunks, K, N))
      return PYGAMD_ERR_WORKSPACE;
  }
  const auto* xs = static_cast<const uint16_t*>(x);
  const auto* gs = static_cast<const uint16_t*>(g);
  auto* gw = static_cast<uint16_t*>(grad_w);
  auto* ws = static_cast<float*>(workspace);
  const int k = static_cast<int>(K), n = static_cast<int>(N), b = static_cast<int>(blocks);
  if (dtype == PYGAMD_DTYPE_BF16)
    return sg_wgrad_launch<LpBf16>(xs, ldx, x_rows, gs, ldg, g_rows, chunks, n_chunks, n_seg, k,
                                   n, b, gw, ws, as_stream(stream));
  return sg_wgrad_launch<LpHalf>(xs, ldx, x_rows, gs, ldg, g_rows, chunks, n_chunks, n_seg, k, n,
                                 b, gw, ws, as_stream(stream));
}

}  // extern "C"
