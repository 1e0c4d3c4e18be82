// test_tables.hip -- the integer counts behind the three tables of `orcai test` for gfx950 (orcai_test_counts): probabilities and labels of one
// batch -> the per-label confusion counts and the histogram the two misclassification tables are formed from.
//
// Replaces the host arithmetic of reference src/orcAI/test.py:37-225 (compute_confusion_table's L boolean passes, the two np.add.at passes of
// compute_misclassification_tables) behind the forward pass.  Everything accumulated is an integer: the result does not depend on the order of
// execution, two runs leave the same bytes, and the host forms the tables' float64 values from the counts (orcai_amd/device_tables.py).
//
// One launch, one lane per row (ROW_TILE = 256 rows per tile, four waves); a workgroup takes tiles_per_wg consecutive tiles.  Per row the L floats of
// p and of y are contiguous; they are folded once into 64-bit words (pred, true1, neg1 and the two truth words of the confusion table) and both
// directions of the misclassification histogram are derived from those words.
//
// Reduction, from the row to global memory:
//   conf     4 ballots per label and wave (the 64 x 64 bit transpose of labels.hip): lane l keeps TN / FP / FN / TP of label l in registers over
//            all tiles of the workgroup; the four waves meet in LDS; one 64-bit atomic add per (label, entry) and workgroup, zeros skipped.
//   hot bin  a row without a true label and without a prediction is NOLABEL -> NOLABEL in BOTH directions (n1 = n2 = 0 either way round) -- in real
//            data almost every row.  One ballot + popcount per wave and tile, summed in a wave-uniform register; one atomic add per direction and
//            workgroup.
//   the rest L <= HIST_L_MAX: a u32 LDS histogram of all 2 (L+1)^2 L bins (LDS atomic adds), flushed with one 64-bit atomic add per non-zero bin and
//            workgroup.  Larger L (the histogram of L = 64 is 2 MiB): one 64-bit global atomic add per (row, set column) of the rows that are NOT
//            in the hot bin -- correct for every L, and only as fast as such rows are rare.
// A workgroup sees at most MAX_TILES_PER_WG * 256 = 2^28 rows, so its 32-bit partial counts cannot wrap; every global accumulator is 64 bits wide.
//
// orcai_threshold_counts (below the first kernel) takes the counts of the threshold sweep in the same way: per label and class a histogram over the
// position of the probability in a table of thresholds, privatised per workgroup in LDS one label tile at a time.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orcai_hip.h"

namespace {

constexpr int ROW_TILE = 256;  // rows per tile = threads per workgroup
constexpr int WAVES = ROW_TILE / 64;
constexpr int HIST_L_MAX = 16;                     // 2 * 17 * 17 * 16 bins * 4 bytes = 36 992 bytes of LDS
constexpr size_t STATIC_LDS = WAVES * 4 * 64 * 4 + 64;  // wconf and whot of the kernel, rounded up
constexpr int64_t MAX_GRID = 1024;                // workgroups before a workgroup takes more than one tile (4 per CU)
constexpr int64_t MAX_TILES_PER_WG = 1ll << 20;    // 2^28 rows: the bound behind the 32-bit partial counts

typedef unsigned long long u64;

// One direction of one row: matrix 1 has its ones in m1, matrix 2 in m2; neg2 marks the columns where matrix 2 is -1.
template <bool HIST>
__device__ __forceinline__ void count_direction(int d, u64 m1, u64 m2, u64 neg2, int L, unsigned* __restrict__ hist, u64* __restrict__ mis) {
  const int n1 = __popcll(m1), n2 = __popcll(m2);
  if (n1 > 1) return;  // the at-most-one-1 mask
  int src = L;         // NOLABEL
  if (n1 == 1) {
    src = __builtin_ctzll(m1);
    if ((neg2 >> src) & 1) return;
  }
  const int64_t base = ((int64_t)(d * (L + 1) + src) * (L + 1)) * L;
  if (n2 == 0) {
    const int64_t i = base + (int64_t)L * L;
    if (HIST) atomicAdd(&hist[i], 1u); else atomicAdd(&mis[i], 1ull);
    return;
  }
  for (u64 m = m2; m; m &= m - 1) {
    const int64_t i = base + (int64_t)__builtin_ctzll(m) * L + (n2 - 1);
    if (HIST) atomicAdd(&hist[i], 1u); else atomicAdd(&mis[i], 1ull);
  }
}

template <bool HIST>
__global__ __launch_bounds__(256) void test_counts_kernel(const float* __restrict__ p, const float* __restrict__ y, int64_t M, int L, float mask_value,
                                                           int64_t tiles_per_wg, u64* __restrict__ conf, u64* __restrict__ mis) {
  extern __shared__ unsigned hist[];  // HIST: u32 [2][L+1][L+1][L]
  __shared__ int wconf[WAVES][4][64];
  __shared__ unsigned whot[WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int bins = 2 * (L + 1) * (L + 1) * L;
  if (HIST) {
    for (int i = tid; i < bins; i += ROW_TILE) hist[i] = 0;
    __syncthreads();
  }
  int tn = 0, fp = 0, fn = 0, tp = 0;  // lane = label
  unsigned nhot = 0;                   // wave-uniform
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_wg;
  for (int64_t t = 0; t < tiles_per_wg; ++t) {
    const int64_t first = (tile0 + t) * ROW_TILE;
    if (first >= M) break;  // the whole workgroup
    const int64_t row = first + tid;
    const bool valid = row < M;
    u64 pred = 0, true1 = 0, neg1 = 0, is0 = 0, is1 = 0;
    if (valid) {
      const float* __restrict__ pr = p + row * L;
      const float* __restrict__ yr = y + row * L;
      for (int l = 0; l < L; ++l) {
        const float pv = pr[l], yv = yr[l];
        const int yi = (int)yv;  // astype(int): truncation
        const bool unmasked = yv != mask_value;
        pred |= (u64)(pv >= 0.5f) << l;  // NaN: not predicted
        true1 |= (u64)(yi == 1) << l;
        neg1 |= (u64)(yi == -1) << l;
        is0 |= (u64)(unmasked && yv == 0.0f) << l;
        is1 |= (u64)(unmasked && yv == 1.0f) << l;
      }
    }
    const u64 fp_w = is0 & pred, tp_w = is1 & pred;
    for (int l = 0; l < L; ++l) {
      const u64 b0 = __ballot((is0 >> l) & 1), bfp = __ballot((fp_w >> l) & 1), b1 = __ballot((is1 >> l) & 1), btp = __ballot((tp_w >> l) & 1);
      if (lane == l) {
        const int cfp = __popcll(bfp), ctp = __popcll(btp);
        tn += __popcll(b0) - cfp;
        fp += cfp;
        fn += __popcll(b1) - ctp;
        tp += ctp;
      }
    }
    const bool hot = valid && true1 == 0 && pred == 0;
    nhot += (unsigned)__popcll(__ballot(hot));
    if (valid && !hot) {
      count_direction<HIST>(0, true1, pred, 0, L, hist, mis);  // true_pred: the prediction bits are never -1
      count_direction<HIST>(1, pred, true1, neg1, L, hist, mis);  // pred_true
    }
  }
  wconf[wave][0][lane] = tn;
  wconf[wave][1][lane] = fp;
  wconf[wave][2][lane] = fn;
  wconf[wave][3][lane] = tp;
  if (lane == 0) whot[wave] = nhot;
  __syncthreads();
  {
    const int k = tid >> 6, l = tid & 63;
    if (l < L) {
      int sum = 0;
      for (int w = 0; w < WAVES; ++w) sum += wconf[w][k][l];
      if (sum) atomicAdd(&conf[l * 4 + k], (u64)sum);
    }
  }
  if (tid < 2) {
    unsigned sum = 0;
    for (int w = 0; w < WAVES; ++w) sum += whot[w];
    if (sum) atomicAdd(&mis[((int64_t)(tid * (L + 1) + L) * (L + 1) + L) * L], (u64)sum);
  }
  if (HIST)
    for (int i = tid; i < bins; i += ROW_TILE) {
      const unsigned v = hist[i];
      if (v) atomicAdd(&mis[i], (u64)v);
    }
}

// ---------------------------------------------------------------- orcai_threshold_counts
// The threshold sweep of `orcai test --threshold-sweep`: hist[l][c][k] counts the elements of label l and class c whose probability lies above exactly
// k entries of the threshold table.  grid = (row workgroups, label tiles): a workgroup takes tiles_per_wg row tiles of 256 rows and `lt` consecutive
// labels, one lane per (row, label) element -- with one label tile (L <= SWEEP_LT_MAX and the image fits) the lanes of a wave read consecutive floats.
// LDS: the table f32[T], then the image u32[lt][2][T + 1] of the tile; k by binary search in the LDS copy of the table (strict f32 comparison, NaN
// above nothing), one LDS atomic add per element, one 64-bit global atomic add per non-zero bin and workgroup.  A workgroup sees at most 2^28 rows, so
// a u32 bin cannot wrap.
constexpr int SWEEP_LT_MAX = 16;               // labels per tile at most: T = 200 -> 16 * 2 * 201 * 4 = 25 728 bytes; T = 1024 -> 7 labels, 57 400 bytes
constexpr size_t SWEEP_LDS_MAX = 64 * 1024;    // table + image stay inside the default 64 KiB of a workgroup

__global__ __launch_bounds__(256) void threshold_counts_kernel(const float* __restrict__ p, const float* __restrict__ y, int64_t M, int L, float mask_value,
                                                                const float* __restrict__ thresholds, int T, int lt_max, int64_t tiles_per_wg,
                                                                u64* __restrict__ out) {
  extern __shared__ unsigned sweep_lds[];
  float* __restrict__ table = reinterpret_cast<float*>(sweep_lds);  // f32 [T]
  unsigned* __restrict__ image = sweep_lds + T;                     // u32 [lt][2][T + 1]
  const int tid = threadIdx.x;
  const int l0 = blockIdx.y * lt_max;
  const int lt = L - l0 < lt_max ? L - l0 : lt_max;
  const int bins = lt * 2 * (T + 1);
  for (int i = tid; i < T; i += ROW_TILE) table[i] = thresholds[i];
  for (int i = tid; i < bins; i += ROW_TILE) image[i] = 0;
  __syncthreads();
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_wg;
  for (int64_t t = 0; t < tiles_per_wg; ++t) {
    const int64_t first = (tile0 + t) * ROW_TILE;
    if (first >= M) break;  // the whole workgroup
    const int rows = M - first < ROW_TILE ? (int)(M - first) : ROW_TILE;
    const int n = rows * lt;  // <= 256 * 16
    for (int e = tid; e < n; e += ROW_TILE) {
      const int r = e / lt, j = e - r * lt;
      const int64_t at = (first + r) * L + l0 + j;
      const float yv = y[at];
      if (!(yv != mask_value) || !(yv == 0.0f || yv == 1.0f)) continue;
      const float pv = p[at];
      int lo = 0, hi = T;  // k = the number of entries below pv: the table ascends strictly
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pv > table[mid]) lo = mid + 1; else hi = mid;
      }
      atomicAdd(&image[(j * 2 + (yv == 1.0f)) * (T + 1) + lo], 1u);
    }
  }
  __syncthreads();
  u64* __restrict__ dst = out + (int64_t)l0 * 2 * (T + 1);
  for (int i = tid; i < bins; i += ROW_TILE) {
    const unsigned v = image[i];
    if (v) atomicAdd(&dst[i], (u64)v);
  }
}

}  // namespace

extern "C" int orcai_test_counts(const float* p, const float* y, int64_t M, int L, float mask_value, int64_t* conf, int64_t* mis, void* stream) {
  if (!p || !y || !conf || !mis || M < 1 || L < 1 || L > 64) return ORCAI_E_BADARG;
  const int64_t tiles = (M - 1) / ROW_TILE + 1;
  int64_t tiles_per_wg = (tiles - 1) / MAX_GRID + 1;
  if (tiles_per_wg > MAX_TILES_PER_WG) tiles_per_wg = MAX_TILES_PER_WG;
  const int64_t grid = (tiles - 1) / tiles_per_wg + 1;
  if (grid > 0x7fffffff) return ORCAI_E_UNSUPPORTED;
  const hipStream_t st = (hipStream_t)stream;
  u64* c = reinterpret_cast<u64*>(conf);
  u64* m = reinterpret_cast<u64*>(mis);
  const size_t lds = (size_t)2 * (L + 1) * (L + 1) * L * sizeof(unsigned);
  if (L <= HIST_L_MAX && lds <= 64 * 1024 - STATIC_LDS) {  // the histogram beside the kernel's static arrays, inside the default 64 KiB
    hipLaunchKernelGGL(test_counts_kernel<true>, dim3((unsigned)grid), dim3(ROW_TILE), lds, st, p, y, M, L, mask_value, tiles_per_wg, c, m);
  } else {
    hipLaunchKernelGGL(test_counts_kernel<false>, dim3((unsigned)grid), dim3(ROW_TILE), 0, st, p, y, M, L, mask_value, tiles_per_wg, c, m);
  }
  return (int)hipGetLastError();
}

extern "C" int orcai_threshold_counts(const float* p, const float* y, int64_t M, int L, float mask_value, const float* thresholds, int T, int64_t* hist,
                                      void* stream) {
  if (!p || !y || !thresholds || !hist || M < 1 || L < 1 || L > 64 || T < 1 || T > 1024) return ORCAI_E_BADARG;
  const int64_t tiles = (M - 1) / ROW_TILE + 1;
  int64_t tiles_per_wg = (tiles - 1) / MAX_GRID + 1;
  if (tiles_per_wg > MAX_TILES_PER_WG) tiles_per_wg = MAX_TILES_PER_WG;
  const int64_t grid = (tiles - 1) / tiles_per_wg + 1;
  if (grid > 0x7fffffff) return ORCAI_E_UNSUPPORTED;
  const size_t per_label = (size_t)2 * (T + 1) * sizeof(unsigned);
  int lt = (int)((SWEEP_LDS_MAX - (size_t)T * sizeof(float)) / per_label);  // >= 7 at T = 1024
  if (lt > SWEEP_LT_MAX) lt = SWEEP_LT_MAX;
  if (lt > L) lt = L;
  const size_t lds = (size_t)T * sizeof(float) + lt * per_label;
  hipLaunchKernelGGL(threshold_counts_kernel, dim3((unsigned)grid, (unsigned)((L + lt - 1) / lt)), dim3(ROW_TILE), lds, (hipStream_t)stream, p, y, M, L,
                     mask_value, thresholds, T, lt, tiles_per_wg, reinterpret_cast<u64*>(hist));
  return (int)hipGetLastError();
}
