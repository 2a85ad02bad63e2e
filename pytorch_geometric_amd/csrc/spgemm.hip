// spgemm.hip — the sparse-sparse product C[M x N] = A[M x K] * B[K x N] on CSR operands
// (torch_geometric/models/graph_unet.py:138-148 `augment_adj`, edge_index.py:2011 `adj @ adj` of the
// reference, which hands both to torch.sparse).  Row-wise Gustavson: row i of C is the sum of the
// rows B_k scaled by A[i, k].  The size of C is not known before the work is done, so the product
// runs twice over the same walk: SYMBOLIC counts the distinct columns of every row (-> rowptr_c),
// NUMERIC accumulates the values, orders every row by column and writes it at rowptr_c[i].
//
// Rows are tiered by ub[i] = sum over the stored entries k of A_i of |B_k|, the number of products
// of the row.  ub overestimates the row's length badly when columns collide (a dense 64 x 64 block:
// ub = 4096, nnz = 64), but the WORK of a row is its products, and a table sized for ub can never
// overflow, so ub is the right key:
//   empty       ub = 0: nothing runs, nnz = 0.
//   wave        ub <= PYGAMD_SPGEMM_WAVE_UB: one wave per row, four rows per workgroup; the wave's
//               key table (2 * WAVE_UB slots, load <= 1/2) and its values live in the wave's own
//               slice of LDS.  Keys are claimed with an integer compare-and-swap.  The wave walks
//               A_i SERIALLY in k and its lanes stride over B_k: B_k has unique columns, so no two
//               lanes of a step share a slot and val[slot] += a * b is a plain LDS read-modify-write.
//               Occupied slots are compacted by ballot + prefix popcount and ordered by counting
//               (rank = number of smaller keys), as the select kernel of pool.hip does.
//   workgroup   ub <= PYGAMD_SPGEMM_GROUP_SMALL_UB / PYGAMD_SPGEMM_GROUP_UB (two table sizes: 40 KB
//               and 80 KB of the 160 KB of LDS, so that mid-sized rows keep 3 / 2 workgroups on a
//               CU): one workgroup per row, one shared key table; wave w takes the entries
//               k = w, w + 4, ... of A_i, serially, and accumulates into ITS OWN value plane.  The
//               four planes are summed in wave order, then the table is sorted in place (bitonic,
//               empty slots are the largest key) and its head is the row.
//   long        anything above: expand - sort - compress over these rows only.  Symbolic counts the
//               row's columns with a bitmap window in LDS (PYGAMD_SPGEMM_BITMAP_COLS columns per
//               pass: no memory in proportion to the products before their number is known to the
//               host); numeric writes (local_row * N + j, a * b) for every product, orders them
//               with the stable pygamd_index_sort, takes the runs from pygamd_run_flags +
//               pygamd_cumsum and sums every run in order.  The only memory in proportion to the
//               number of products.
//
// NO FLOAT ATOMICS.  The value of C[i, j] is a fixed-order sum, bit-identical from run to run:
//   wave tier: the products a_ik * b_kj in the order the entries k are stored in A_i;
//   workgroup: plane w holds that ordered sum over the entries at positions w, w + 4, ... of A_i;
//              the result is ((p0 + p1) + p2) + p3;
//   long:      the stored order of A_i again (the sort is stable, a run keeps product order).
// The price of the serial-k rule: a step of the walk uses |B_k| of 64 lanes (profiles/spgemm.md).
#include "common.h"
#include "scan_device.h"

namespace pygamd {
namespace {

constexpr int kTiers = PYGAMD_SPGEMM_TIERS;
enum { kTierEmpty = 0, kTierWave = 1, kTierGroupS = 2, kTierGroupL = 3, kTierLong = 4 };
static_assert(kTiers == kTierLong + 1, "five tiers");

constexpr uint32_t kEmpty = 0xFFFFFFFFu;   // no column: N < 2^31
constexpr int kWaveLog2 = 9;               // the wave tier's table: 512 slots
constexpr int kWaveSlots = 1 << kWaveLog2;
constexpr int kWaveRow = PYGAMD_SPGEMM_WAVE_UB;            // the longest row it can produce
constexpr int kWaveRowPerLane = kWaveRow / kWave;
constexpr int kGroupSmallLog2 = 11, kGroupLog2 = 12;       // 2,048 and 4,096 slots
static_assert(2 * PYGAMD_SPGEMM_WAVE_UB <= kWaveSlots, "load factor <= 1/2");
static_assert(2 * PYGAMD_SPGEMM_GROUP_SMALL_UB <= (1 << kGroupSmallLog2), "load factor <= 1/2");
static_assert(2 * PYGAMD_SPGEMM_GROUP_UB <= (1 << kGroupLog2), "load factor <= 1/2");
static_assert(kWaveRow % kWave == 0, "whole keys per lane");
constexpr int kBitmapWords = PYGAMD_SPGEMM_BITMAP_COLS / 32;   // 64 KB of LDS
constexpr int kTotals = 3;   // nnz of C, products of the long rows, long rows

template <typename IdxT>
struct Mat {
  const IdxT* ptr;
  const IdxT* col;
  const float* val;   // NULL: all ones
  int64_t rows;
  int64_t nnz;
};

// the stored entries [b, e) of row r, clamped to the arrays
template <typename IdxT>
__device__ __forceinline__ void row_range(const Mat<IdxT>& m, int64_t r, int64_t& b, int64_t& e) {
  b = static_cast<int64_t>(m.ptr[r]);
  e = static_cast<int64_t>(m.ptr[r + 1]);
  b = b < 0 ? 0 : (b > m.nnz ? m.nnz : b);
  e = e < b ? b : (e > m.nnz ? m.nnz : e);
}

// entry p of A: its row of B ([kb, ke), empty when the column is outside [0, K)) and its value
template <typename IdxT>
__device__ __forceinline__ float a_entry(const Mat<IdxT>& A, const Mat<IdxT>& B, int64_t p,
                                         int64_t& kb, int64_t& ke) {
  const int64_t k = static_cast<int64_t>(A.col[p]);
  kb = ke = 0;
  if (k >= 0 && k < B.rows) row_range(B, k, kb, ke);
  return A.val ? A.val[p] : 1.f;
}

__device__ __forceinline__ int tier_of(int64_t ub) {
  if (ub <= 0) return kTierEmpty;
  if (ub <= PYGAMD_SPGEMM_WAVE_UB) return kTierWave;
  if (ub <= PYGAMD_SPGEMM_GROUP_SMALL_UB) return kTierGroupS;
  if (ub <= PYGAMD_SPGEMM_GROUP_UB) return kTierGroupL;
  return kTierLong;
}

// LDS written by one lane and read by another lane of the same wave
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = kWave >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// The slot of column c in a table of 2^LOG2 keys (multiplicative hash, linear probing); `fresh`
// says that this call claimed it.  The table is never more than half full, so a probe ends; the
// bound on the probes keeps malformed input from spinning (-1: not placed).
template <int LOG2>
__device__ __forceinline__ int table_insert(uint32_t* keys, uint32_t c, bool& fresh) {
  constexpr int kMask = (1 << LOG2) - 1;
  int s = static_cast<int>((c * 0x9E3779B1u) >> (32 - LOG2));
  fresh = false;
  for (int probe = 0; probe <= kMask; ++probe) {
    const uint32_t old = atomicCAS(&keys[s], kEmpty, c);
    if (old == kEmpty) {
      fresh = true;
      return s;
    }
    if (old == c) return s;
    s = (s + 1) & kMask;
  }
  return -1;
}

// The walk both phases share: the entries first, first + step, ... of A's row [ab, ae), one after
// the other; the lanes of the wave stride over B_k.  Returns the slots this lane claimed.
template <typename IdxT, int LOG2, bool NUMERIC>
__device__ __forceinline__ int walk_row(const Mat<IdxT>& A, const Mat<IdxT>& B, int64_t ab,
                                        int64_t ae, int first, int step, uint32_t* keys,
                                        float* vals, int lane) {
  int claimed = 0;
  for (int64_t p = ab + first; p < ae; p += step) {
    int64_t kb, ke;
    const float a = a_entry(A, B, p, kb, ke);
    for (int64_t q = kb + lane; q < ke; q += kWave) {
      bool fresh;
      const int s = table_insert<LOG2>(keys, static_cast<uint32_t>(B.col[q]), fresh);
      if (NUMERIC) {
        if (s >= 0) vals[s] += a * (B.val ? B.val[q] : 1.f);
      } else {
        claimed += fresh ? 1 : 0;
      }
    }
  }
  return claimed;
}

// ---- bound -------------------------------------------------------------------------------------
// one wave per row of A: ub, the tier, and nnz = 0 until a tier kernel says otherwise
template <typename IdxT>
__global__ __launch_bounds__(kBlock) void spgemm_bound_kernel(Mat<IdxT> A, Mat<IdxT> B,
                                                              int64_t* __restrict__ ub,
                                                              int64_t* __restrict__ tier,
                                                              IdxT* __restrict__ rowptr_c) {
  const int lane = lane_id();
  if (blockIdx.x == 0 && threadIdx.x == 0) rowptr_c[0] = 0;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block(); i < A.rows;
       i += step) {
    int64_t ab, ae;
    row_range(A, i, ab, ae);
    int64_t s = 0;
    for (int64_t p = ab + lane; p < ae; p += kWave) {
      int64_t kb, ke;
      a_entry(A, B, p, kb, ke);
      s += ke - kb;
    }
#pragma unroll
    for (int off = kWave >> 1; off > 0; off >>= 1) {
      s += bcast_lane(s, lane ^ off);
    }
    if (lane == 0) {
      ub[i] = s;
      tier[i] = tier_of(s);
      rowptr_c[i + 1] = 0;
    }
  }
}

// ---- wave tier ---------------------------------------------------------------------------------
template <typename IdxT, bool NUMERIC>
__global__ __launch_bounds__(kBlock) void spgemm_wave_kernel(
    Mat<IdxT> A, Mat<IdxT> B, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ tier_ptr, IdxT* __restrict__ nnz_out,
    const IdxT* __restrict__ rowptr_c, IdxT* __restrict__ col_c, float* __restrict__ val_c,
    int64_t nnz_c) {
  __shared__ uint32_t keys_s[kWavesPerBlock][kWaveSlots];
  __shared__ float vals_s[NUMERIC ? kWavesPerBlock : 1][NUMERIC ? kWaveSlots : 1];
  __shared__ uint32_t ckeys_s[NUMERIC ? kWavesPerBlock : 1][NUMERIC ? kWaveRow : 1];
  __shared__ float cvals_s[NUMERIC ? kWavesPerBlock : 1][NUMERIC ? kWaveRow : 1];
  const int wave = wave_in_block(), lane = lane_id();
  uint32_t* keys = keys_s[wave];
  float* vals = vals_s[NUMERIC ? wave : 0];
  const int64_t t0 = tier_ptr[kTierWave], n = tier_ptr[kTierWave + 1] - t0;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave; r < n; r += step) {
    const int64_t i = perm[t0 + r];
    if (i < 0 || i >= A.rows) continue;
    for (int s = lane; s < kWaveSlots; s += kWave) {
      keys[s] = kEmpty;
      if (NUMERIC) vals[s] = 0.f;
    }
    wave_lds_sync();
    int64_t ab, ae;
    row_range(A, i, ab, ae);
    const int claimed = walk_row<IdxT, kWaveLog2, NUMERIC>(A, B, ab, ae, 0, 1, keys, vals, lane);
    wave_lds_sync();
    if (!NUMERIC) {
      const int total = wave_sum(claimed);
      if (lane == 0) nnz_out[i] = static_cast<IdxT>(total);
      continue;
    }
    uint32_t* ck = ckeys_s[NUMERIC ? wave : 0];
    float* cv = cvals_s[NUMERIC ? wave : 0];
    const uint64_t below = (1ull << lane) - 1ull;
    int cnt = 0;
    for (int s0 = 0; s0 < kWaveSlots; s0 += kWave) {
      const uint32_t key = keys[s0 + lane];
      const float v = vals[s0 + lane];
      const uint64_t m = __ballot(key != kEmpty);
      const int pos = cnt + __popcll(m & below);
      if (key != kEmpty && pos < kWaveRow) {
        ck[pos] = key;
        cv[pos] = v;
      }
      cnt += __popcll(m);
    }
    wave_lds_sync();
    const int64_t base = static_cast<int64_t>(rowptr_c[i]);
    int64_t len = static_cast<int64_t>(rowptr_c[i + 1]) - base;
    if (len > cnt) len = cnt;
    if (len > kWaveRow) len = kWaveRow;
    const int m = static_cast<int>(len < 0 ? 0 : len);
    uint32_t myk[kWaveRowPerLane];
    float myv[kWaveRowPerLane];
    int rank[kWaveRowPerLane];
#pragma unroll
    for (int q = 0; q < kWaveRowPerLane; ++q) {
      const int idx = q * kWave + lane;
      myk[q] = idx < m ? ck[idx] : kEmpty;
      myv[q] = idx < m ? cv[idx] : 0.f;
      rank[q] = 0;
    }
    for (int j = 0; j < m; ++j) {
      const uint32_t kj = ck[j];   // (every lane reads the same address: a broadcast)
#pragma unroll
      for (int q = 0; q < kWaveRowPerLane; ++q) rank[q] += kj < myk[q] ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < kWaveRowPerLane; ++q) {
      const int64_t o = base + rank[q];
      if (q * kWave + lane < m && o >= 0 && o < nnz_c) {
        col_c[o] = static_cast<IdxT>(myk[q]);
        val_c[o] = myv[q];
      }
    }
    wave_lds_sync();   // the compacted row has been read before the next one is written
  }
}

// ---- workgroup tier ----------------------------------------------------------------------------
template <typename IdxT, int LOG2, int TIER, bool NUMERIC>
__global__ __launch_bounds__(kBlock) void spgemm_group_kernel(
    Mat<IdxT> A, Mat<IdxT> B, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ tier_ptr, IdxT* __restrict__ nnz_out,
    const IdxT* __restrict__ rowptr_c, IdxT* __restrict__ col_c, float* __restrict__ val_c,
    int64_t nnz_c) {
  constexpr int kSlots = 1 << LOG2;
  __shared__ uint32_t keys[kSlots];
  __shared__ float planes[NUMERIC ? kWavesPerBlock * kSlots : 1];
  __shared__ int wave_cnt[kWavesPerBlock];
  const int wave = wave_in_block(), lane = lane_id(), tid = static_cast<int>(threadIdx.x);
  const int64_t t0 = tier_ptr[TIER], n = tier_ptr[TIER + 1] - t0;
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t i = perm[t0 + r];
    if (i < 0 || i >= A.rows) continue;   // (the same in every thread)
    __syncthreads();                      // the previous row has left the table
    for (int s = tid; s < kSlots; s += kBlock) {
      keys[s] = kEmpty;
      if (NUMERIC) {
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) planes[w * kSlots + s] = 0.f;
      }
    }
    __syncthreads();
    int64_t ab, ae;
    row_range(A, i, ab, ae);
    const int claimed = walk_row<IdxT, LOG2, NUMERIC>(
        A, B, ab, ae, wave, kWavesPerBlock, keys, planes + (NUMERIC ? wave * kSlots : 0), lane);
    if (!NUMERIC) {
      const int total = wave_sum(claimed);
      if (lane == 0) wave_cnt[wave] = total;
      __syncthreads();
      if (tid == 0) {
        int t = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) t += wave_cnt[w];
        nnz_out[i] = static_cast<IdxT>(t);
      }
      continue;
    }
    __syncthreads();
    for (int s = tid; s < kSlots; s += kBlock) {   // the four planes, in wave order
      if (keys[s] != kEmpty) {
        planes[s] = ((planes[s] + planes[kSlots + s]) + planes[2 * kSlots + s]) +
                    planes[3 * kSlots + s];
      }
    }
    __syncthreads();
    // bitonic sort of (key, value) over the whole table, ascending: empty slots are the largest key
    for (int k = 2; k <= kSlots; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < kSlots / 2; t += kBlock) {
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int hi = lo | j;
          const uint32_t klo = keys[lo], khi = keys[hi];
          const bool up = (lo & k) == 0;
          if ((klo > khi) == up && klo != khi) {
            keys[lo] = khi;
            keys[hi] = klo;
            const float v = planes[lo];
            planes[lo] = planes[hi];
            planes[hi] = v;
          }
        }
        __syncthreads();
      }
    }
    const int64_t base = static_cast<int64_t>(rowptr_c[i]);
    int64_t len = static_cast<int64_t>(rowptr_c[i + 1]) - base;
    if (len > kSlots) len = kSlots;
    for (int t = tid; t < len; t += kBlock) {
      const int64_t o = base + t;
      if (keys[t] != kEmpty && o >= 0 && o < nnz_c) {
        col_c[o] = static_cast<IdxT>(keys[t]);
        val_c[o] = planes[t];
      }
    }
  }
}

// ---- long tier ---------------------------------------------------------------------------------
__device__ __forceinline__ int64_t clamp_col(int64_t j, int64_t N) {
  return j < 0 ? 0 : (j >= N ? N - 1 : j);
}

// symbolic: the distinct columns of a long row, one window of the column range at a time
template <typename IdxT>
__global__ __launch_bounds__(kBlock) void spgemm_long_count_kernel(
    Mat<IdxT> A, Mat<IdxT> B, int64_t N, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ tier_ptr, IdxT* __restrict__ nnz_out) {
  __shared__ uint32_t bitmap[kBitmapWords];
  __shared__ int64_t wave_tot[kWavesPerBlock];
  const int wave = wave_in_block(), lane = lane_id(), tid = static_cast<int>(threadIdx.x);
  const int64_t t0 = tier_ptr[kTierLong], n = tier_ptr[kTierLong + 1] - t0;
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t i = perm[t0 + r];
    if (i < 0 || i >= A.rows) continue;
    int64_t ab, ae;
    row_range(A, i, ab, ae);
    int64_t mine = 0;
    for (int64_t c0 = 0; c0 < N; c0 += PYGAMD_SPGEMM_BITMAP_COLS) {
      __syncthreads();
      for (int w = tid; w < kBitmapWords; w += kBlock) bitmap[w] = 0u;
      __syncthreads();
      for (int64_t p = ab + wave; p < ae; p += kWavesPerBlock) {
        int64_t kb, ke;
        a_entry(A, B, p, kb, ke);
        for (int64_t q = kb + lane; q < ke; q += kWave) {
          const int64_t d = clamp_col(static_cast<int64_t>(B.col[q]), N) - c0;
          if (d >= 0 && d < PYGAMD_SPGEMM_BITMAP_COLS) {
            atomicOr(&bitmap[d >> 5], 1u << (d & 31));
          }
        }
      }
      __syncthreads();
      for (int w = tid; w < kBitmapWords; w += kBlock) mine += __popc(bitmap[w]);
    }
    int64_t total;
    block_inclusive_scan(mine, wave_tot, total);
    if (tid == 0) nnz_out[i] = static_cast<IdxT>(total);
  }
}

// long_off[r] = ub of the r-th long row, 0 behind the last one (its inclusive scan follows)
__global__ __launch_bounds__(kBlock) void spgemm_long_ub_kernel(
    const int64_t* __restrict__ ub, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ tier_ptr, int64_t M, int64_t* __restrict__ long_off) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r >= M) return;
  const int64_t t0 = tier_ptr[kTierLong], n = tier_ptr[kTierLong + 1] - t0;
  int64_t v = 0;
  if (r < n) {
    const int64_t i = perm[t0 + r];
    if (i >= 0 && i < M) v = ub[i];
  }
  long_off[r] = v;
}

template <typename IdxT>
__global__ void spgemm_totals_kernel(const IdxT* __restrict__ rowptr_c,
                                     const int64_t* __restrict__ long_off,
                                     const int64_t* __restrict__ tier_ptr, int64_t M,
                                     int64_t* __restrict__ totals) {
  totals[0] = M > 0 ? static_cast<int64_t>(rowptr_c[M]) : 0;
  totals[1] = M > 0 ? long_off[M - 1] : 0;
  totals[2] = M > 0 ? tier_ptr[kTierLong + 1] - tier_ptr[kTierLong] : 0;
}

// numeric, step 1: every product of the long rows, in the order (entry of A_i, entry of B_k), as
// (local_row * N + j, a * b) at the row's offset + the products of the entries before
template <typename IdxT>
__global__ __launch_bounds__(kBlock) void spgemm_expand_kernel(
    Mat<IdxT> A, Mat<IdxT> B, int64_t N, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ tier_ptr, const int64_t* __restrict__ ub,
    const int64_t* __restrict__ long_off, int64_t L, int64_t P, int64_t* __restrict__ key,
    float* __restrict__ val) {
  __shared__ int64_t wave_tot[kWavesPerBlock];
  __shared__ int64_t off[kBlock];
  const int wave = wave_in_block(), lane = lane_id(), tid = static_cast<int>(threadIdx.x);
  const int64_t t0 = tier_ptr[kTierLong];
  int64_t n = tier_ptr[kTierLong + 1] - t0;
  if (n > L) n = L;
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t i = perm[t0 + r];
    if (i < 0 || i >= A.rows) continue;
    int64_t ab, ae;
    row_range(A, i, ab, ae);
    int64_t carry = long_off[r] - ub[i];   // (the scan is inclusive)
    for (int64_t c0 = ab; c0 < ae; c0 += kBlock) {
      int64_t kb = 0, ke = 0;
      if (c0 + tid < ae) a_entry(A, B, c0 + tid, kb, ke);
      int64_t total;
      const int64_t incl = block_inclusive_scan(ke - kb, wave_tot, total);
      off[tid] = carry + incl - (ke - kb);
      __syncthreads();
      const int64_t here = ae - c0 < kBlock ? ae - c0 : kBlock;
      for (int64_t t = wave; t < here; t += kWavesPerBlock) {
        const float a = a_entry(A, B, c0 + t, kb, ke);
        const int64_t o = off[t];
        for (int64_t q = kb + lane; q < ke; q += kWave) {
          const int64_t pos = o + (q - kb);
          if (pos >= 0 && pos < P) {
            key[pos] = r * N + clamp_col(static_cast<int64_t>(B.col[q]), N);
            val[pos] = a * (B.val ? B.val[q] : 1.f);
          }
        }
      }
      carry += total;
      __syncthreads();   // off[] has been read
    }
  }
}

// numeric, step 2: the run slot of every long row's first entry
__global__ __launch_bounds__(kBlock) void spgemm_row_base_kernel(
    const int64_t* __restrict__ key, const int64_t* __restrict__ scan, int64_t P, int64_t N,
    int64_t L, int64_t* __restrict__ row_base) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= P) return;
  const int64_t r = key[t] / N;
  if (r < 0 || r >= L) return;
  if (t == 0 || key[t - 1] / N != r) row_base[r] = scan[t] - 1;
}

// numeric, step 3: the head of every run sums it in order and writes the entry of C
template <typename IdxT>
__global__ __launch_bounds__(kBlock) void spgemm_sum_runs_kernel(
    const int64_t* __restrict__ key, const int64_t* __restrict__ scan,
    const int64_t* __restrict__ order, const float* __restrict__ val, int64_t P, int64_t N,
    int64_t L, const int64_t* __restrict__ row_base, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ tier_ptr, int64_t M, const IdxT* __restrict__ rowptr_c,
    IdxT* __restrict__ col_c, float* __restrict__ val_c, int64_t nnz_c) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= P) return;
  const int64_t k = key[t];
  if (t > 0 && key[t - 1] == k) return;
  const int64_t r = k / N;
  if (r < 0 || r >= L) return;
  const int64_t slot = tier_ptr[kTierLong] + r;
  if (slot < 0 || slot >= M) return;
  const int64_t i = perm[slot];
  if (i < 0 || i >= M) return;
  float acc = 0.f;
  for (int64_t u = t; u < P && key[u] == k; ++u) {
    const int64_t src = order[u];
    if (src >= 0 && src < P) acc += val[src];
  }
  const int64_t o = static_cast<int64_t>(rowptr_c[i]) + (scan[t] - 1 - row_base[r]);
  if (o >= 0 && o < nnz_c) {
    col_c[o] = static_cast<IdxT>(k - r * N);
    val_c[o] = acc;
  }
}

// ---- workspaces --------------------------------------------------------------------------------
inline size_t align256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }

struct PlanLayout {   // of the plan workspace, in bytes from its start
  size_t totals, ub, tier, tier_sorted, perm, tier_ptr, long_off, scratch, scratch_bytes, bytes;
};

int plan_layout(int64_t M, PlanLayout* p) {
  const size_t rows = align256(static_cast<size_t>(M) * sizeof(int64_t));
  size_t sort_b = 0, scan_b = 0;
  int rc = pygamd_index_sort_workspace_bytes(PYGAMD_IDX_I64, M, &sort_b);
  if (rc != PYGAMD_OK) return rc;
  rc = pygamd_cumsum_workspace_bytes(PYGAMD_IDX_I64, M + 1, &scan_b);
  if (rc != PYGAMD_OK) return rc;
  size_t at = 0;
  p->totals = at, at += 256;
  p->tier_ptr = at, at += 256;
  p->ub = at, at += rows;
  p->tier = at, at += rows;
  p->tier_sorted = at, at += rows;
  p->perm = at, at += rows;
  p->long_off = at, at += rows;
  p->scratch = at;
  p->scratch_bytes = align256(sort_b > scan_b ? sort_b : scan_b);
  p->bytes = at + p->scratch_bytes;
  return PYGAMD_OK;
}

struct LongLayout {   // of the long tier's workspace
  size_t key_a, key_b, order, val, row_base, scratch, scratch_bytes, bytes;
};

int long_layout(int64_t L, int64_t P, LongLayout* p) {
  const size_t prod = align256(static_cast<size_t>(P) * sizeof(int64_t));
  size_t sort_b = 0, scan_b = 0;
  int rc = pygamd_index_sort_workspace_bytes(PYGAMD_IDX_I64, P, &sort_b);
  if (rc != PYGAMD_OK) return rc;
  rc = pygamd_cumsum_workspace_bytes(PYGAMD_IDX_I64, P, &scan_b);
  if (rc != PYGAMD_OK) return rc;
  size_t at = 0;
  p->key_a = at, at += prod;   // the products' keys; after the sort the run flags and their scan
  p->key_b = at, at += prod;   // the sorted keys
  p->order = at, at += prod;   // the sort's permutation
  p->val = at, at += align256(static_cast<size_t>(P) * sizeof(float));
  p->row_base = at, at += align256(static_cast<size_t>(L) * sizeof(int64_t));
  p->scratch = at;
  p->scratch_bytes = align256(sort_b > scan_b ? sort_b : scan_b);
  p->bytes = at + p->scratch_bytes;
  return PYGAMD_OK;
}

template <typename T>
T* at(void* base, size_t off) {
  return reinterpret_cast<T*>(static_cast<char*>(base) + off);
}

// the grids stride over their tier's rows, whose number only the device knows
unsigned capped(int64_t n, int64_t cap) {
  return static_cast<unsigned>(n < 1 ? 1 : (n > cap ? cap : n));
}
constexpr int64_t kWaveGridCap = 8192, kGroupGridCap = 4096, kLongGridCap = 1024;

int check_operands(const void* rowptr_a, const void* col_a, const void* rowptr_b,
                   const void* col_b, int idx_dtype, int64_t M, int64_t K, int64_t N,
                   int64_t nnz_a, int64_t nnz_b) {
  if (idx_dtype != PYGAMD_IDX_I32 && idx_dtype != PYGAMD_IDX_I64) return PYGAMD_ERR_INVALID_ARG;
  if (M < 0 || K < 0 || N < 0 || nnz_a < 0 || nnz_b < 0) return PYGAMD_ERR_INVALID_ARG;
  if (!rowptr_a || !rowptr_b) return PYGAMD_ERR_INVALID_ARG;
  if ((nnz_a > 0 && !col_a) || (nnz_b > 0 && !col_b)) return PYGAMD_ERR_INVALID_ARG;
  if ((nnz_a > 0 && K == 0) || (nnz_b > 0 && N == 0)) return PYGAMD_ERR_INVALID_ARG;
  if (N > INT32_MAX || M >= (int64_t{1} << 31)) return PYGAMD_ERR_UNSUPPORTED;
  return PYGAMD_OK;
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_spgemm_workspace_size(int idx_dtype, int64_t M, int64_t long_rows,
                                  int64_t long_products, size_t* plan_bytes, size_t* long_bytes) {
  if (idx_dtype != PYGAMD_IDX_I32 && idx_dtype != PYGAMD_IDX_I64) return PYGAMD_ERR_INVALID_ARG;
  if (M < 0 || long_rows < 0 || long_products < 0 || !plan_bytes || !long_bytes)
    return PYGAMD_ERR_INVALID_ARG;
  if (long_products > INT32_MAX || long_rows > M) return PYGAMD_ERR_UNSUPPORTED;
  PlanLayout pl;
  LongLayout ll;
  int rc = plan_layout(M, &pl);
  if (rc != PYGAMD_OK) return rc;
  rc = long_layout(long_rows, long_products, &ll);
  if (rc != PYGAMD_OK) return rc;
  *plan_bytes = pl.bytes;
  *long_bytes = long_products > 0 ? ll.bytes : 0;
  return PYGAMD_OK;
}

int pygamd_spgemm_symbolic(const void* rowptr_a, const void* col_a, const void* rowptr_b,
                           const void* col_b, int idx_dtype, int64_t M, int64_t K, int64_t N,
                           int64_t nnz_a, int64_t nnz_b, void* rowptr_c, int64_t* totals,
                           void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_operands(rowptr_a, col_a, rowptr_b, col_b, idx_dtype, M, K, N, nnz_a, nnz_b);
  if (rc != PYGAMD_OK) return rc;
  if (!rowptr_c || !totals || !workspace) return PYGAMD_ERR_INVALID_ARG;
  PlanLayout pl;
  rc = plan_layout(M, &pl);
  if (rc != PYGAMD_OK) return rc;
  if (workspace_bytes < pl.bytes) return PYGAMD_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  int64_t* d_totals = at<int64_t>(workspace, pl.totals);
  int64_t* tier_ptr = at<int64_t>(workspace, pl.tier_ptr);
  int64_t* ub = at<int64_t>(workspace, pl.ub);
  int64_t* tier = at<int64_t>(workspace, pl.tier);
  int64_t* tier_sorted = at<int64_t>(workspace, pl.tier_sorted);
  int64_t* perm = at<int64_t>(workspace, pl.perm);
  int64_t* long_off = at<int64_t>(workspace, pl.long_off);
  void* scratch = at<char>(workspace, pl.scratch);
  const dim3 block(kBlock);
  rc = PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    const Mat<IdxT> A{static_cast<const IdxT*>(rowptr_a), static_cast<const IdxT*>(col_a), nullptr,
                      M, nnz_a};
    const Mat<IdxT> B{static_cast<const IdxT*>(rowptr_b), static_cast<const IdxT*>(col_b), nullptr,
                      K, nnz_b};
    IdxT* ptr_c = static_cast<IdxT*>(rowptr_c);
    hipLaunchKernelGGL((spgemm_bound_kernel<IdxT>),
                       dim3(capped(ceil_div(M, kWavesPerBlock), kWaveGridCap)), block, 0, st, A, B,
                       ub, tier, ptr_c);
    PYGAMD_LAUNCH_CHECK();
    if (M == 0) return PYGAMD_OK;
    int r = pygamd_index_sort(tier, PYGAMD_IDX_I64, M, kTiers - 1, tier_sorted, perm, scratch,
                              pl.scratch_bytes, stream);
    if (r != PYGAMD_OK) return r;
    r = pygamd_index2ptr(tier_sorted, PYGAMD_IDX_I64, M, kTiers, tier_ptr, stream);
    if (r != PYGAMD_OK) return r;
    IdxT* nnz_out = ptr_c + 1;
    hipLaunchKernelGGL((spgemm_wave_kernel<IdxT, false>),
                       dim3(capped(ceil_div(M, kWavesPerBlock), kWaveGridCap)), block, 0, st, A, B,
                       perm, tier_ptr, nnz_out, static_cast<const IdxT*>(nullptr),
                       static_cast<IdxT*>(nullptr), static_cast<float*>(nullptr), int64_t{0});
    PYGAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((spgemm_group_kernel<IdxT, kGroupSmallLog2, kTierGroupS, false>),
                       dim3(capped(M, kGroupGridCap)), block, 0, st, A, B, perm, tier_ptr, nnz_out,
                       static_cast<const IdxT*>(nullptr), static_cast<IdxT*>(nullptr),
                       static_cast<float*>(nullptr), int64_t{0});
    PYGAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((spgemm_group_kernel<IdxT, kGroupLog2, kTierGroupL, false>),
                       dim3(capped(M, kGroupGridCap)), block, 0, st, A, B, perm, tier_ptr, nnz_out,
                       static_cast<const IdxT*>(nullptr), static_cast<IdxT*>(nullptr),
                       static_cast<float*>(nullptr), int64_t{0});
    PYGAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((spgemm_long_count_kernel<IdxT>), dim3(capped(M, kLongGridCap)), block, 0,
                       st, A, B, N, perm, tier_ptr, nnz_out);
    PYGAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(spgemm_long_ub_kernel, dim3(static_cast<unsigned>(ceil_div(M, kBlock))),
                       block, 0, st, ub, perm, tier_ptr, M, long_off);
    PYGAMD_LAUNCH_CHECK();
    r = pygamd_cumsum(long_off, PYGAMD_IDX_I64, M, long_off, scratch, pl.scratch_bytes, stream);
    if (r != PYGAMD_OK) return r;
    r = pygamd_cumsum(nnz_out, idx_dtype, M, nnz_out, scratch, pl.scratch_bytes, stream);
    if (r != PYGAMD_OK) return r;
    hipLaunchKernelGGL((spgemm_totals_kernel<IdxT>), dim3(1), dim3(1), 0, st, ptr_c, long_off,
                       tier_ptr, M, d_totals);
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
  if (rc != PYGAMD_OK) return rc;
  int64_t host[kTotals] = {0, 0, 0};
  if (M > 0) {
    PYGAMD_HIP_CHECK(hipMemcpyAsync(host, d_totals, sizeof(host), hipMemcpyDeviceToHost, st));
  }
  PYGAMD_HIP_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < kTotals; ++i) totals[i] = host[i];
  totals[kTotals] = 0;
  if (host[1] > INT32_MAX || host[0] < 0 || host[2] > M) return PYGAMD_ERR_UNSUPPORTED;
  LongLayout ll;
  rc = long_layout(host[2], host[1], &ll);
  if (rc != PYGAMD_OK) return rc;
  totals[kTotals] = host[1] > 0 ? static_cast<int64_t>(ll.bytes) : 0;
  return PYGAMD_OK;
}

int pygamd_spgemm_numeric(const void* rowptr_a, const void* col_a, const float* val_a,
                          const void* rowptr_b, const void* col_b, const float* val_b,
                          int idx_dtype, int64_t M, int64_t K, int64_t N, int64_t nnz_a,
                          int64_t nnz_b, const void* rowptr_c, int64_t nnz_c, void* col_c,
                          float* val_c, int64_t long_rows, int64_t long_products, void* workspace,
                          size_t workspace_bytes, void* long_workspace,
                          size_t long_workspace_bytes, void* stream) {
  int rc = check_operands(rowptr_a, col_a, rowptr_b, col_b, idx_dtype, M, K, N, nnz_a, nnz_b);
  if (rc != PYGAMD_OK) return rc;
  if (nnz_c < 0 || long_rows < 0 || long_products < 0 || long_rows > M || !rowptr_c || !workspace)
    return PYGAMD_ERR_INVALID_ARG;
  if (nnz_c > 0 && (!col_c || !val_c)) return PYGAMD_ERR_INVALID_ARG;
  if ((long_rows > 0) != (long_products > 0)) return PYGAMD_ERR_INVALID_ARG;
  if (long_products > INT32_MAX) return PYGAMD_ERR_UNSUPPORTED;
  PlanLayout pl;
  LongLayout ll;
  rc = plan_layout(M, &pl);
  if (rc != PYGAMD_OK) return rc;
  rc = long_layout(long_rows, long_products, &ll);
  if (rc != PYGAMD_OK) return rc;
  if (workspace_bytes < pl.bytes) return PYGAMD_ERR_WORKSPACE;
  if (long_products > 0 && (!long_workspace || long_workspace_bytes < ll.bytes))
    return PYGAMD_ERR_WORKSPACE;
  if (M == 0 || nnz_c == 0) return PYGAMD_OK;
  hipStream_t st = as_stream(stream);
  const int64_t* tier_ptr = at<int64_t>(workspace, pl.tier_ptr);
  const int64_t* ub = at<int64_t>(workspace, pl.ub);
  const int64_t* perm = at<int64_t>(workspace, pl.perm);
  const int64_t* long_off = at<int64_t>(workspace, pl.long_off);
  const dim3 block(kBlock);
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    const Mat<IdxT> A{static_cast<const IdxT*>(rowptr_a), static_cast<const IdxT*>(col_a), val_a,
                      M, nnz_a};
    const Mat<IdxT> B{static_cast<const IdxT*>(rowptr_b), static_cast<const IdxT*>(col_b), val_b,
                      K, nnz_b};
    const IdxT* ptr_c = static_cast<const IdxT*>(rowptr_c);
    IdxT* cc = static_cast<IdxT*>(col_c);
    hipLaunchKernelGGL((spgemm_wave_kernel<IdxT, true>),
                       dim3(capped(ceil_div(M, kWavesPerBlock), kWaveGridCap)), block, 0, st, A, B,
                       perm, tier_ptr, static_cast<IdxT*>(nullptr), ptr_c, cc, val_c, nnz_c);
    PYGAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((spgemm_group_kernel<IdxT, kGroupSmallLog2, kTierGroupS, true>),
                       dim3(capped(M, kGroupGridCap)), block, 0, st, A, B, perm, tier_ptr,
                       static_cast<IdxT*>(nullptr), ptr_c, cc, val_c, nnz_c);
    PYGAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((spgemm_group_kernel<IdxT, kGroupLog2, kTierGroupL, true>),
                       dim3(capped(M, kGroupGridCap)), block, 0, st, A, B, perm, tier_ptr,
                       static_cast<IdxT*>(nullptr), ptr_c, cc, val_c, nnz_c);
    PYGAMD_LAUNCH_CHECK();
    if (long_products == 0) return PYGAMD_OK;
    const int64_t L = long_rows, P = long_products;
    int64_t* key_a = at<int64_t>(long_workspace, ll.key_a);
    int64_t* key_b = at<int64_t>(long_workspace, ll.key_b);
    int64_t* order = at<int64_t>(long_workspace, ll.order);
    float* val = at<float>(long_workspace, ll.val);
    int64_t* row_base = at<int64_t>(long_workspace, ll.row_base);
    void* scratch = at<char>(long_workspace, ll.scratch);
    hipLaunchKernelGGL((spgemm_expand_kernel<IdxT>), dim3(capped(L, kLongGridCap)), block, 0, st,
                       A, B, N, perm, tier_ptr, ub, long_off, L, P, key_a, val);
    PYGAMD_LAUNCH_CHECK();
    int r = pygamd_index_sort(key_a, PYGAMD_IDX_I64, P, L * N - 1, key_b, order, scratch,
                              ll.scratch_bytes, stream);
    if (r != PYGAMD_OK) return r;
    int64_t* scan = key_a;   // (the unsorted keys are done with)
    r = pygamd_run_flags(key_b, P, scan, stream);
    if (r != PYGAMD_OK) return r;
    r = pygamd_cumsum(scan, PYGAMD_IDX_I64, P, scan, scratch, ll.scratch_bytes, stream);
    if (r != PYGAMD_OK) return r;
    const dim3 grid(static_cast<unsigned>(ceil_div(P, kBlock)));
    hipLaunchKernelGGL(spgemm_row_base_kernel, grid, block, 0, st, key_b, scan, P, N, L, row_base);
    PYGAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((spgemm_sum_runs_kernel<IdxT>), grid, block, 0, st, key_b, scan, order, val,
                       P, N, L, row_base, perm, tier_ptr, M, ptr_c, cc, val_c, nnz_c);
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

}  // extern "C"
