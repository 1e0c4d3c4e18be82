// labels.hip -- label extraction of the predict path for gfx950 (orcai_extract_labels): the averaged probabilities of one recording or of a batch of
// recordings -> the label intervals, in the order of the label file, with the verdict of the duration filter.
//
// Replaces the host arithmetic behind the overlap average (reference src/orcAI/predict.py:298-340 compute_binary_predictions + compute_labels, and
// the per-interval _check_duration of :14-66): threshold / max(count), the strict comparison, find_consecutive_ones per label, the stable
// sort_values(by=["start", "stop", "label"]) and the too short / too long decision.  Everything compared and written is an integer, so the
// output equals the host route exactly.
//
// Tiles.  ROW_TILE = 256 rows per workgroup (one lane per row, four waves); SCAN_TILE = 64 row tiles (16384 rows) per pass of the scan
// (one wave per sequence, one lane per row tile, a carry between passes).
//
// Launches, all on the caller's stream, none of them walks a run:
//   1 threshold  one workgroup per recording: max of its counts (NaN kept, as np.max), thr_r = threshold / max as one f64 division
//                (+inf, "nothing is a one", for no rows or a zero maximum).
//   2 mask       one lane per row: the L doubles of the row are contiguous, b[l] = agg > thr_r (strict, NaN false) -> one 64-bit word per row.
//                orcai_extract_labels_per_label: launch 1 hands on max(cnt) itself and this one compares with thr_r[l] = thresholds[l] / max(cnt),
//                the same single f64 division per label; everything behind the mask is shared.
//   3 count      per row tile: start = m & ~m[row - 1], stop = m & ~m[row + 1] (neighbours inside the recording only).  Column counts come from
//                L ballots per wave (the 64 x 64 bit transpose), summed over the four waves: 2 L + 1 counts per tile (starts of all columns,
//                starts per column, stops per column), stored sequence-major.
//   4 scan       exclusive scan of every sequence over the row tiles, in place; the total of sequence 0 is offsets[R].
//   5 stops      the k-th stop of column l writes its row to stops[l][k] (k = scanned tile count + waves before + lanes below in the ballot).
//   6 emit       the k-th start of column l reads stops[l][k]: a run.  Its output position is the scanned start count of the rows before
//                it plus its rank among the at most 64 runs that start in its row, by (stop, label_rank, label): the wave takes its rows that
//                start something one by one, lane = column, and compares through readlane -- n^2 / 64 steps for a row of n starts.  One 16-byte
//                store per run.  The lane of a recording's first row writes offsets[r].
// The output position of every run is computed, never claimed: no atomics, two calls give the same bytes.  Recordings tile [0, S_total) in
// ascending row order (the ragged overlap average's table), so the global order (row, stop, rank, label) is the per-recording order.
//
// orcai_extract_labels_refined (hysteresis thresholds and gap merging; the second half of this file) first computes, per row, in which
// columns a FINAL run starts and stops -- candidates from the low mask, kept iff they hold a row above the high threshold, chains of kept candidates
// at most g rows apart joined -- and then runs launches 3-6 on those two edge words (REFINED) instead of on the mask.
//
// Worst cases this was laid out against: one run as long as the recording (two edges in the whole matrix: nothing iterates over its length) and
// all 64 columns alternating every row (every second row starts 64 runs: 64 readlane steps per such row, spread over all waves).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orcai_hip.h"

namespace {

constexpr int ROW_TILE = 256;  // rows per workgroup
constexpr int SCAN_TILE = 64;  // row tiles per scan pass (one wave)
constexpr int WAVES = ROW_TILE / 64;

typedef unsigned long long u64;

struct Layout {
  size_t thr, mask, counts, stops, total;  // byte offsets into the workspace
  int64_t tiles, colcap;
};

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

inline Layout layout(int L, int R, int64_t S_total) {
  Layout a;
  a.tiles = (S_total + ROW_TILE - 1) / ROW_TILE;
  a.colcap = S_total / 2 + R;  // runs one column can hold: the sum of ceil(S_r / 2)
  a.thr = 0;                                                          // f64 [R]
  a.mask = a.thr + up256((size_t)R * 8);                              // u64 [S_total]
  a.counts = a.mask + up256((size_t)S_total * 8);                     // i64 [2 L + 1][tiles]
  a.stops = a.counts + up256((size_t)(2 * L + 1) * a.tiles * 8);      // i32 [L][colcap]
  a.total = a.stops + up256((size_t)L * (size_t)a.colcap * 4);
  return a;
}

// the last recording whose first output row is <= row (overlap_average_ragged_kernel's search)
__device__ __forceinline__ int locate(const int64_t* __restrict__ table, int R, int64_t row) {
  int lo = 0, hi = R - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[4 * mid + 3] <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int read_lane(int v, int i) { return __builtin_amdgcn_readlane(v, i); }
__device__ __forceinline__ u64 read_lane64(u64 v, int i) {
  return ((u64)(uint32_t)read_lane((int)(v >> 32), i) << 32) | (uint32_t)read_lane((int)(uint32_t)v, i);
}
__device__ __forceinline__ u64 lanes_below(int i) { return i >= 64 ? ~0ull : ((1ull << i) - 1); }

struct Edges {
  u64 start, stop;  // columns in which a run starts / ends (inclusive) in this row
  int rel;          // the row, counted from its recording's first
};

// REFINED (orcai_extract_labels_refined's second half): `mask` holds the two edge words of every row, {starts, stops}, as refine_edges_kernel left them
template <bool REFINED>
__device__ __forceinline__ Edges row_edges(const u64* __restrict__ mask, const int64_t* __restrict__ table, int R, int64_t S_total, int64_t row) {
  Edges e = {0, 0, 0};
  if (row >= S_total) return e;
  if (REFINED) {
    e.start = mask[2 * row];
    e.stop = mask[2 * row + 1];
    if ((e.start | e.stop) == 0) return e;
    e.rel = (int)(row - table[4 * locate(table, R, row) + 3]);
    return e;
  }
  const u64 m = mask[row];
  if (m == 0) return e;
  const int r = locate(table, R, row);  // m != 0: the row lies inside recording r (mask kernel)
  const int64_t s = row - table[4 * r + 3], S = table[4 * r + 2];
  const u64 prev = (s > 0 && row > 0) ? mask[row - 1] : 0;
  const u64 next = (s + 1 < S && row + 1 < S_total) ? mask[row + 1] : 0;
  e.start = m & ~prev;
  e.stop = m & ~next;
  e.rel = (int)s;
  return e;
}

// ---------------------------------------------------------------- 1 threshold
__global__ __launch_bounds__(256) void labels_threshold_kernel(const double* __restrict__ cnt, const int64_t* __restrict__ table, int64_t S_total,
                                                                double threshold, bool per_label, double* __restrict__ thr) {
  __shared__ double part[WAVES];
  __shared__ int part_nan[WAVES];
  const int r = blockIdx.x;
  int64_t lo = table[4 * r + 3], hi = lo + table[4 * r + 2];
  if (lo < 0) lo = 0;
  if (hi > S_total) hi = S_total;
  double m = -__builtin_inf();
  int nan = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const double c = cnt[i];
    nan |= (c != c);
    m = c > m ? c : m;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const double o = __shfl_xor(m, d);
    nan |= __shfl_xor(nan, d);
    m = o > m ? o : m;
  }
  if (lane_id() == 0) {
    part[threadIdx.x >> 6] = m;
    part_nan[threadIdx.x >> 6] = nan;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < WAVES; ++w) {
      m = part[w] > m ? part[w] : m;
      nan |= part_nan[w];
    }
    double t = __builtin_inf();  // no rows, or a zero maximum: nothing is a one
    if (hi > lo) {
      if (nan) t = __builtin_nan("");  // np.max keeps a NaN: every comparison is false
      else if (m != 0.0) t = threshold / m;
    }
    if (per_label) {  // the mask kernel divides per label: it gets the maximum itself, 0 standing for "nothing is a one"
      t = 0.0;
      if (hi > lo) t = nan ? __builtin_nan("") : m;
    }
    thr[r] = t;
  }
}

// ---------------------------------------------------------------- 2 mask
__global__ __launch_bounds__(256) void labels_mask_kernel(const double* __restrict__ agg, int L, const int64_t* __restrict__ table, int R, int64_t S_total,
                                                           const double* __restrict__ thr, const double* __restrict__ thresholds, u64* __restrict__ mask) {
  const int64_t row = (int64_t)blockIdx.x * ROW_TILE + threadIdx.x;
  if (row >= S_total) return;
  const int r = locate(table, R, row);
  const int64_t s = row - table[4 * r + 3];
  u64 m = 0;
  if (s >= 0 && s < table[4 * r + 2]) {
    const double t = thr[r];
    const double* __restrict__ p = agg + row * L;
    if (!thresholds) {
      for (int l = 0; l < L; ++l) m |= (u64)(p[l] > t) << l;
    } else if (t != 0.0) {  // t is max(cnt) here (NaN kept: every comparison is false); thr_r[l] = thresholds[l] / max(cnt), one f64 division
      for (int l = 0; l < L; ++l) m |= (u64)(p[l] > thresholds[l] / t) << l;
    }
  }
  mask[row] = m;
}

// ---------------------------------------------------------------- 3 count
template <bool REFINED>
__global__ __launch_bounds__(256) void labels_count_kernel(const u64* __restrict__ mask, int L, const int64_t* __restrict__ table, int R, int64_t S_total,
                                                            int64_t tiles, int64_t* __restrict__ counts) {
  __shared__ int wc[WAVES][2][64];
  __shared__ int wr[WAVES];
  const int64_t tile = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const Edges e = row_edges<REFINED>(mask, table, R, S_total, tile * ROW_TILE + threadIdx.x);
  int cs = 0, ce = 0;
  for (int l = 0; l < L; ++l) {
    const u64 bs = __ballot((e.start >> l) & 1), be = __ballot((e.stop >> l) & 1);
    if (lane == l) {
      cs = __popcll(bs);
      ce = __popcll(be);
    }
  }
  wc[wave][0][lane] = cs;
  wc[wave][1][lane] = ce;
  int n = __popcll(e.start);
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
  if (lane == 0) wr[wave] = n;
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 128) {
    const int which = t >> 6, l = t & 63;
    if (l < L) {
      int sum = 0;
      for (int w = 0; w < WAVES; ++w) sum += wc[w][which][l];
      counts[(int64_t)(1 + which * L + l) * tiles + tile] = sum;
    }
  } else if (t == 128) {
    int sum = 0;
    for (int w = 0; w < WAVES; ++w) sum += wr[w];
    counts[tile] = sum;
  }
}

// ---------------------------------------------------------------- 4 scan
__global__ __launch_bounds__(256) void labels_scan_kernel(int64_t* __restrict__ counts, int sequences, int64_t tiles, int64_t* __restrict__ total) {
  const int q = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (q >= sequences) return;  // a whole wave
  const int lane = lane_id();
  int64_t* __restrict__ seq = counts + (int64_t)q * tiles;
  int64_t carry = 0;
  for (int64_t base = 0; base < tiles; base += SCAN_TILE) {
    const int64_t i = base + lane;
    const int64_t v = i < tiles ? seq[i] : 0;
    int64_t incl = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    if (i < tiles) seq[i] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
  if (q == 0 && lane == 0) *total = carry;
}

// ---------------------------------------------------------------- 5 stops
template <bool REFINED>
__global__ __launch_bounds__(256) void labels_stops_kernel(const u64* __restrict__ mask, int L, const int64_t* __restrict__ table, int R, int64_t S_total,
                                                            int64_t tiles, const int64_t* __restrict__ counts, int64_t colcap, int* __restrict__ stops) {
  __shared__ int wc[WAVES][64];
  __shared__ int64_t colbase[WAVES][64];
  const int64_t tile = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const Edges e = row_edges<REFINED>(mask, table, R, S_total, tile * ROW_TILE + threadIdx.x);
  int ce = 0;
  for (int l = 0; l < L; ++l) {
    const u64 be = __ballot((e.stop >> l) & 1);
    if (lane == l) ce = __popcll(be);
  }
  wc[wave][lane] = ce;
  __syncthreads();
  int64_t b = 0;
  if (lane < L) {
    b = counts[(int64_t)(1 + L + lane) * tiles + tile];
    for (int w = 0; w < wave; ++w) b += wc[w][lane];
  }
  colbase[wave][lane] = b;
  __syncthreads();
  for (int l = 0; l < L; ++l) {
    const u64 be = __ballot((e.stop >> l) & 1);
    if (be == 0) continue;
    if ((e.stop >> l) & 1) {
      const int64_t k = colbase[wave][l] + __popcll(be & lanes_below(lane));
      if (k < colcap) stops[(int64_t)l * colcap + k] = e.rel;
    }
  }
}

// ---------------------------------------------------------------- 6 emit
template <bool REFINED>
__global__ __launch_bounds__(256) void labels_emit_kernel(const u64* __restrict__ mask, int L, const int64_t* __restrict__ table, int R, int64_t S_total,
                                                           int64_t tiles, const int64_t* __restrict__ counts, int64_t colcap,
                                                           const int* __restrict__ stops, const int* __restrict__ label_rank,
                                                           const double* __restrict__ limits, double frame_seconds, int tpo, int4* __restrict__ runs,
                                                           int64_t capacity, int64_t* __restrict__ offsets) {
  __shared__ int wc[WAVES][64];
  __shared__ int wr[WAVES];
  const int64_t tile = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int64_t row = tile * ROW_TILE + threadIdx.x;
  const Edges e = row_edges<REFINED>(mask, table, R, S_total, row);
  u64 mycol = 0;  // lane = column: the rows of this wave that start a run in it
  for (int l = 0; l < L; ++l) {
    const u64 bs = __ballot((e.start >> l) & 1);
    if (lane == l) mycol = bs;
  }
  wc[wave][lane] = __popcll(mycol);
  const int n = __popcll(e.start);
  int incl = n;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wr[wave] = incl;
  __syncthreads();
  int64_t cb = 0;  // lane = column: runs of the column that start before this wave's rows
  int rk = 0;
  double mn = 0.0, mx = __builtin_inf();
  if (lane < L) {
    cb = counts[(int64_t)(1 + lane) * tiles + tile];
    for (int w = 0; w < wave; ++w) cb += wc[w][lane];
    rk = label_rank[lane];
    if (limits) {
      mn = limits[2 * lane];
      mx = limits[2 * lane + 1];
    }
  }
  int64_t rb = counts[tile] + (incl - n);  // lane = row: runs that start before this row
  for (int w = 0; w < wave; ++w) rb += wr[w];

  // offsets: the first row of a recording knows how many runs lie before it; recordings without rows share the next one's first row
  if (row < S_total) {
    const int r = locate(table, R, row);
    if (table[4 * r + 3] == row)
      for (int q = r; q >= 0 && table[4 * q + 3] == row; --q) offsets[q] = rb;
  }
  if (tile == 0) {  // recordings without rows behind the last row (offsets[R], the total, is the scan's)
    const int64_t total = offsets[R];
    for (int q = threadIdx.x; q < R; q += 256)
      if (table[4 * q + 3] >= S_total) offsets[q] = total;
  }

  u64 ne = __ballot(e.start != 0);
  while (ne) {
    const int i = __builtin_ctzll(ne);  // wave-uniform: the next row of this wave that starts a run
    ne &= ne - 1;
    const u64 m = read_lane64(e.start, i);
    const int srel = read_lane(e.rel, i);
    const int64_t base = (int64_t)read_lane64((u64)rb, i);
    const bool act = (m >> lane) & 1;
    int stop = srel;
    if (act) {
      const int64_t k = cb + __popcll(mycol & lanes_below(i));
      if (k < colcap) stop = stops[(int64_t)lane * colcap + k];
    }
    int c = 0;  // runs of this row that sort before this lane's
    for (u64 mm = m; mm; mm &= mm - 1) {
      const int j = __builtin_ctzll(mm);
      const int sj = read_lane(stop, j), rj = read_lane(rk, j);
      c += (sj < stop) || (sj == stop && (rj < rk || (rj == rk && j < lane)));
    }
    if (act) {
      const int64_t pos = base + c;
      if (pos < capacity) {
        int status = 0;
        if (limits) {
          const double d = (double)((int64_t)(stop - srel) * tpo) * frame_seconds;
          status = d < mn ? 1 : (d > mx ? 2 : 0);
        }
        runs[pos] = make_int4(srel, stop, lane, status);
      }
    }
  }
}

// Both entry points: thresholds == nullptr is the scalar call (threshold / max(cnt) once per recording), else thresholds f64[L] on the device.
int extract_labels(const double* agg, const double* cnt, int L, const int64_t* table, int R, int64_t S_total, double threshold, const double* thresholds,
                   const int* label_rank, const double* limits, double frame_seconds, int tpo, int* runs, int64_t capacity, int64_t* offsets,
                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!agg || !cnt || !table || !label_rank || !runs || !offsets || !workspace) return ORCAI_E_BADARG;
  if (L < 1 || L > 64 || R < 1 || S_total < 1 || capacity < 0 || tpo < 1) return ORCAI_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(runs) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 255)) return ORCAI_E_BADARG;
  const Layout a = layout(L, R, S_total);
  if (workspace_bytes < a.total) return ORCAI_E_BADARG;
  if (a.tiles > 0x7fffffff) return ORCAI_E_UNSUPPORTED;
  char* ws = static_cast<char*>(workspace);
  double* thr = reinterpret_cast<double*>(ws + a.thr);
  u64* mask = reinterpret_cast<u64*>(ws + a.mask);
  int64_t* counts = reinterpret_cast<int64_t*>(ws + a.counts);
  int* stops = reinterpret_cast<int*>(ws + a.stops);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)a.tiles), block(ROW_TILE);
  const int sequences = 2 * L + 1;
  hipLaunchKernelGGL(labels_threshold_kernel, dim3((unsigned)R), block, 0, st, cnt, table, S_total, threshold, thresholds != nullptr, thr);
  hipLaunchKernelGGL(labels_mask_kernel, grid, block, 0, st, agg, L, table, R, S_total, thr, thresholds, mask);
  hipLaunchKernelGGL(labels_count_kernel<false>, grid, block, 0, st, mask, L, table, R, S_total, a.tiles, counts);
  hipLaunchKernelGGL(labels_scan_kernel, dim3((unsigned)((sequences + WAVES - 1) / WAVES)), block, 0, st, counts, sequences, a.tiles, offsets + R);
  hipLaunchKernelGGL(labels_stops_kernel<false>, grid, block, 0, st, mask, L, table, R, S_total, a.tiles, counts, a.colcap, stops);
  hipLaunchKernelGGL(labels_emit_kernel<false>, grid, block, 0, st, mask, L, table, R, S_total, a.tiles, counts, a.colcap, stops, label_rank, limits,
                     frame_seconds, tpo, reinterpret_cast<int4*>(runs), capacity, offsets);
  return (int)hipGetLastError();
}

// ================================================================ orcai_extract_labels_refined: hysteresis and gap merging
// The first half works on the CANDIDATES, the maximal stretches of the low mask: launches 1-4 above with two masks (lo, and hi = above the high
// threshold AND lo) and a third counted sequence per column, the hi rows.  Then
//   R5 lists  the k-th start of column l writes its global row to cstart[l][k] and the number of hi rows of the column before it to hs[l][k]; the
//             k-th stop writes cstop[l][k] and the number of hi rows up to and including it to he[l][k].  Candidate k is KEPT iff he > hs: a
//             difference of two prefix counts, whatever the length of the candidate.
//   R6 keep   one lane per candidate: the kept flags as 64-bit words (one ballot per wave), keepbits[l][k / 64].
//   R7 words  one wave per column over its words, 64 per pass with a carry: the last non-zero word before every word and the first one behind it.
//   R8 edges  one lane per row.  A kept candidate's start finds the kept candidate before it (the bits below its own in its word, else the top bit
//             of the word R7 points to) and starts a final run unless that one lies in the same recording at most g rows away; its stop looks at
//             the next kept candidate likewise.  Dropped candidates have no bit, so they are skipped, and a chain of any length has one start
//             and one stop left: nothing walks it.  Two edge words per row.
// The second half is launches 3-6 above on those edge words (REFINED): the same scans, the same order, the same 16 bytes per run.
// Global rows are kept as int32, so S_total >= 2^31 is ORCAI_E_UNSUPPORTED here.
struct RefineLayout {
  size_t thr, lo, hi, cnt3, cstart, cstop, hs, he, keep, prevnz, nextnz, edges, counts, stops, dummy, total;
  int64_t tiles, tiles1, colcap, words;
};

inline RefineLayout refine_layout(int L, int R, int64_t S_total) {
  RefineLayout a;
  a.tiles = (S_total + ROW_TILE - 1) / ROW_TILE;
  a.tiles1 = a.tiles + 1;  // one slot behind the last tile: the exclusive scan leaves the column's total there
  a.colcap = S_total / 2 + R;
  a.words = (a.colcap + 63) / 64;
  const size_t list = up256((size_t)L * (size_t)a.colcap * 4), word = up256((size_t)L * (size_t)a.words * 8);
  a.thr = 0;                                                         // f64 [R]
  a.lo = a.thr + up256((size_t)R * 8);                               // u64 [S_total]
  a.hi = a.lo + up256((size_t)S_total * 8);                          // u64 [S_total]
  a.cnt3 = a.hi + up256((size_t)S_total * 8);                        // i64 [3 L][tiles + 1]
  a.cstart = a.cnt3 + up256((size_t)(3 * L) * a.tiles1 * 8);         // i32 [L][colcap], as cstop, hs, he and stops
  a.cstop = a.cstart + list;
  a.hs = a.cstop + list;
  a.he = a.hs + list;
  a.keep = a.he + list;                                              // u64 [L][words]
  a.prevnz = a.keep + word;                                          // i32 [L][words], as nextnz
  a.nextnz = a.prevnz + word;
  a.edges = a.nextnz + word;                                         // u64 [S_total][2]
  a.counts = a.edges + up256((size_t)S_total * 16);                  // i64 [2 L + 1][tiles]
  a.stops = a.counts + up256((size_t)(2 * L + 1) * a.tiles * 8);
  a.dummy = a.stops + list;                                          // i64: the total the first scan has no use for
  a.total = a.dummy + 256;
  return a;
}

// ---------------------------------------------------------------- R2 masks
__global__ __launch_bounds__(256) void refine_mask_kernel(const double* __restrict__ agg, int L, const int64_t* __restrict__ table, int R, int64_t S_total,
                                                           const double* __restrict__ thr, const double* __restrict__ thresholds,
                                                           const double* __restrict__ high, u64* __restrict__ lo, u64* __restrict__ hi) {
  const int64_t row = (int64_t)blockIdx.x * ROW_TILE + threadIdx.x;
  if (row >= S_total) return;
  const int r = locate(table, R, row);
  const int64_t s = row - table[4 * r + 3];
  u64 a = 0, b = 0;
  if (s >= 0 && s < table[4 * r + 2]) {
    const double t = thr[r];  // max(cnt), NaN kept, 0: nothing is a one (labels_threshold_kernel, per_label)
    const double* __restrict__ p = agg + row * L;
    if (t != 0.0) {
      for (int l = 0; l < L; ++l) {
        const double v = p[l];
        const bool low = v > thresholds[l] / t;
        a |= (u64)low << l;
        b |= (u64)(low && v > high[l] / t) << l;  // hi counts only where lo is set
      }
    }
  }
  lo[row] = a;
  hi[row] = b;
}

// ---------------------------------------------------------------- R3 count: starts, stops and hi rows per column and tile
__global__ __launch_bounds__(256) void refine_count_kernel(const u64* __restrict__ lo, const u64* __restrict__ hi, int L, const int64_t* __restrict__ table, int R,
                                                            int64_t S_total, int64_t tiles, int64_t* __restrict__ cnt3) {
  __shared__ int wc[WAVES][3][64];
  const int64_t tile = blockIdx.x, row = tile * ROW_TILE + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const Edges e = row_edges<false>(lo, table, R, S_total, row);
  const u64 h = row < S_total ? hi[row] : 0;
  int cs = 0, ce = 0, ch = 0;
  for (int l = 0; l < L; ++l) {
    const u64 bs = __ballot((e.start >> l) & 1), be = __ballot((e.stop >> l) & 1), bh = __ballot((h >> l) & 1);
    if (lane == l) {
      cs = __popcll(bs);
      ce = __popcll(be);
      ch = __popcll(bh);
    }
  }
  wc[wave][0][lane] = cs;
  wc[wave][1][lane] = ce;
  wc[wave][2][lane] = ch;
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 192) {
    const int which = t >> 6, l = t & 63;
    if (l < L) {
      int sum = 0;
      for (int w = 0; w < WAVES; ++w) sum += wc[w][which][l];
      int64_t* __restrict__ seq = cnt3 + (int64_t)(which * L + l) * (tiles + 1);
      seq[tile] = sum;
      if (tile == 0) seq[tiles] = 0;
    }
  }
}

// ---------------------------------------------------------------- R5 lists
__global__ __launch_bounds__(256) void refine_lists_kernel(const u64* __restrict__ lo, const u64* __restrict__ hi, int L, const int64_t* __restrict__ table, int R,
                                                            int64_t S_total, int64_t tiles, const int64_t* __restrict__ cnt3, int64_t colcap,
                                                            int* __restrict__ cstart, int* __restrict__ cstop, int* __restrict__ hs, int* __restrict__ he) {
  __shared__ int wc[WAVES][3][64];
  __shared__ int64_t base[WAVES][3][64];
  const int64_t tile = blockIdx.x, row = tile * ROW_TILE + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const Edges e = row_edges<false>(lo, table, R, S_total, row);
  const u64 h = row < S_total ? hi[row] : 0;
  int cs = 0, ce = 0, ch = 0;
  for (int l = 0; l < L; ++l) {
    const u64 bs = __ballot((e.start >> l) & 1), be = __ballot((e.stop >> l) & 1), bh = __ballot((h >> l) & 1);
    if (lane == l) {
      cs = __popcll(bs);
      ce = __popcll(be);
      ch = __popcll(bh);
    }
  }
  wc[wave][0][lane] = cs;
  wc[wave][1][lane] = ce;
  wc[wave][2][lane] = ch;
  __syncthreads();
  for (int which = 0; which < 3; ++which) {
    int64_t b = 0;
    if (lane < L) {
      b = cnt3[(int64_t)(which * L + lane) * (tiles + 1) + tile];
      for (int w = 0; w < wave; ++w) b += wc[w][which][lane];
    }
    base[wave][which][lane] = b;
  }
  __syncthreads();
  for (int l = 0; l < L; ++l) {
    const u64 bs = __ballot((e.start >> l) & 1), be = __ballot((e.stop >> l) & 1);
    if ((bs | be) == 0) continue;
    const u64 bh = __ballot((h >> l) & 1);
    const int64_t hb = base[wave][2][l];
    if ((e.start >> l) & 1) {
      const int64_t k = base[wave][0][l] + __popcll(bs & lanes_below(lane));
      if (k < colcap) {
        cstart[(int64_t)l * colcap + k] = (int)row;
        hs[(int64_t)l * colcap + k] = (int)(hb + __popcll(bh & lanes_below(lane)));
      }
    }
    if ((e.stop >> l) & 1) {
      const int64_t k = base[wave][1][l] + __popcll(be & lanes_below(lane));
      if (k < colcap) {
        cstop[(int64_t)l * colcap + k] = (int)row;
        he[(int64_t)l * colcap + k] = (int)(hb + __popcll(bh & lanes_below(lane + 1)));
      }
    }
  }
}

// candidates of column l: the total the scan left behind the last tile of its starts, never more than the lists hold
__device__ __forceinline__ int64_t candidates(const int64_t* __restrict__ cnt3, int l, int64_t tiles, int64_t colcap) {
  const int64_t n = cnt3[(int64_t)l * (tiles + 1) + tiles];
  return n < colcap ? n : colcap;
}

// ---------------------------------------------------------------- R6 keep
__global__ __launch_bounds__(256) void refine_keep_kernel(const int64_t* __restrict__ cnt3, int64_t tiles, int64_t colcap, int64_t words,
                                                           const int* __restrict__ hs, const int* __restrict__ he, u64* __restrict__ keepbits) {
  const int l = blockIdx.y;
  const int64_t n = candidates(cnt3, l, tiles, colcap);
  if ((int64_t)blockIdx.x * 256 >= n) return;  // words behind the last candidate are never read
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool kept = k < n && he[(int64_t)l * colcap + k] > hs[(int64_t)l * colcap + k];
  const u64 b = __ballot(kept);
  if (lane_id() == 0 && (k >> 6) < words) keepbits[(int64_t)l * words + (k >> 6)] = b;
}

// ---------------------------------------------------------------- R7 words: nearest non-zero word before and behind every word
__global__ __launch_bounds__(256) void refine_words_kernel(const int64_t* __restrict__ cnt3, int L, int64_t tiles, int64_t colcap, int64_t words,
                                                            const u64* __restrict__ keepbits, int* __restrict__ prevnz, int* __restrict__ nextnz) {
  const int l = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (l >= L) return;  // a whole wave
  const int lane = lane_id();
  const int64_t nw = (candidates(cnt3, l, tiles, colcap) + 63) >> 6;
  const u64* __restrict__ kb = keepbits + (int64_t)l * words;
  const int NONE = 0x7fffffff;
  int carry = -1;
  for (int64_t first = 0; first < nw; first += SCAN_TILE) {
    const int64_t w = first + lane;
    int incl = (w < nw && kb[w] != 0) ? (int)w : -1;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl = o > incl ? o : incl;
    }
    int excl = __shfl_up(incl, 1);
    if (lane == 0) excl = -1;
    excl = carry > excl ? carry : excl;
    if (w < nw) prevnz[(int64_t)l * words + w] = excl;
    const int last = __shfl(incl, 63);
    carry = last > carry ? last : carry;
  }
  carry = NONE;
  for (int64_t first = nw > 0 ? ((nw - 1) / SCAN_TILE) * SCAN_TILE : -1; first >= 0; first -= SCAN_TILE) {
    const int64_t w = first + lane;
    int incl = (w < nw && kb[w] != 0) ? (int)w : NONE;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_down(incl, d);
      if (lane + d < 64) incl = o < incl ? o : incl;
    }
    int excl = __shfl_down(incl, 1);
    if (lane == 63) excl = NONE;
    excl = carry < excl ? carry : excl;
    if (w < nw) nextnz[(int64_t)l * words + w] = excl == NONE ? -1 : excl;
    const int head = __shfl(incl, 0);
    carry = head < carry ? head : carry;
  }
}

// ---------------------------------------------------------------- R8 edges
__global__ __launch_bounds__(256) void refine_edges_kernel(const u64* __restrict__ lo, int L, const int64_t* __restrict__ table, int R, int64_t S_total,
                                                            int64_t tiles, const int64_t* __restrict__ cnt3, int64_t colcap, int64_t words,
                                                            const int* __restrict__ cstart, const int* __restrict__ cstop, const u64* __restrict__ keepbits,
                                                            const int* __restrict__ prevnz, const int* __restrict__ nextnz, const int* __restrict__ gap_rows,
                                                            u64* __restrict__ edges) {
  __shared__ int wc[WAVES][2][64];
  __shared__ int64_t base[WAVES][2][64];
  const int64_t tile = blockIdx.x, row = tile * ROW_TILE + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const Edges e = row_edges<false>(lo, table, R, S_total, row);
  int cs = 0, ce = 0;
  for (int l = 0; l < L; ++l) {
    const u64 bs = __ballot((e.start >> l) & 1), be = __ballot((e.stop >> l) & 1);
    if (lane == l) {
      cs = __popcll(bs);
      ce = __popcll(be);
    }
  }
  wc[wave][0][lane] = cs;
  wc[wave][1][lane] = ce;
  __syncthreads();
  for (int which = 0; which < 2; ++which) {
    int64_t b = 0;
    if (lane < L) {
      b = cnt3[(int64_t)(which * L + lane) * (tiles + 1) + tile];
      for (int w = 0; w < wave; ++w) b += wc[w][which][lane];
    }
    base[wave][which][lane] = b;
  }
  __syncthreads();
  int64_t first = 0, last = -1;  // the recording of this row
  if (e.start | e.stop) {
    const int r = locate(table, R, row);
    first = table[4 * r + 3];
    last = first + table[4 * r + 2] - 1;
  }
  u64 fs = 0, fe = 0;
  for (int l = 0; l < L; ++l) {
    const u64 bs = __ballot((e.start >> l) & 1), be = __ballot((e.stop >> l) & 1);
    if ((bs | be) == 0) continue;
    const u64* __restrict__ kb = keepbits + (int64_t)l * words;
    const int64_t g = gap_rows[l];
    if ((e.start >> l) & 1) {
      const int64_t k = base[wave][0][l] + __popcll(bs & lanes_below(lane));
      const u64 word = k < colcap ? kb[k >> 6] : 0;
      if ((word >> (k & 63)) & 1) {
        const u64 below = word & lanes_below((int)(k & 63));
        int64_t pk = -1;  // the kept candidate before this one
        if (below) {
          pk = (k & ~(int64_t)63) + 63 - __builtin_clzll(below);
        } else {
          const int pw = prevnz[(int64_t)l * words + (k >> 6)];
          if (pw >= 0) pk = (int64_t)pw * 64 + 63 - __builtin_clzll(kb[pw]);
        }
        bool join = false;
        if (pk >= 0) {
          const int64_t p = cstop[(int64_t)l * colcap + pk];
          join = p >= first && row - p - 1 <= g;
        }
        if (!join) fs |= 1ull << l;
      }
    }
    if ((e.stop >> l) & 1) {
      const int64_t k = base[wave][1][l] + __popcll(be & lanes_below(lane));
      const u64 word = k < colcap ? kb[k >> 6] : 0;
      if ((word >> (k & 63)) & 1) {
        const u64 above = word & ~lanes_below((int)(k & 63) + 1);
        int64_t nk = -1;  // the kept candidate behind this one
        if (above) {
          nk = (k & ~(int64_t)63) + __builtin_ctzll(above);
        } else {
          const int nw = nextnz[(int64_t)l * words + (k >> 6)];
          if (nw >= 0) nk = (int64_t)nw * 64 + __builtin_ctzll(kb[nw]);
        }
        bool join = false;
        if (nk >= 0) {
          const int64_t q = cstart[(int64_t)l * colcap + nk];
          join = q <= last && q - row - 1 <= g;
        }
        if (!join) fe |= 1ull << l;
      }
    }
  }
  if (row < S_total) {
    edges[2 * row] = fs;
    edges[2 * row + 1] = fe;
  }
}

// ================================================================ orcai_interval_scores: peak, peak row and fixed-point sum per run
// A segmented reduction over the runs an extraction call left in `runs` / `offsets`, in two launches.  Tiles are cut on GLOBAL rows (tile t = rows
// 256 t .. 256 t + 255 of agg, whatever recording they lie in): a run lies inside one recording, so every tile wholly inside a run does too.
//   S1 tiles  one workgroup per row tile reads its 256 x L slab once: per (tile, label) the maximum (NaN skipped), the first row that attains it and
//             the sum of q32(p) = rint(clamp(p, 0, 1) * 2^32) as u64.  Thread = (row part, label), the labels of a row in neighbouring lanes, so a
//             wave's load is a contiguous stretch of the slab; a thread reads at most 64 rows.
//   S2 runs   SCORE_LANES = 16 lanes per run (a fixed grid strides over the runs; their number is only known on the device).  The recording of run i
//             is a binary search of i in offsets.  The lanes share the head piece (the rows before the first whole tile, at most 255), the whole
//             tiles (from S1's table) and the tail piece (at most 255 rows; a run without a whole tile is one piece of at most 510 rows), then merge
//             through four xor shuffles.  A lane's work: at most 2 * 16 rows + (tiles of the run) / 16 table entries.
// Merging keeps the larger value and, among equal values, the lower row; the sums are integers: every order of reduction gives the same bytes, and
// nothing is claimed with an atomic.  agg is read once by S1 and, element for element, at most once more by S2 (the head and tail rows of a run).
constexpr int SCORE_LANES = 16;
constexpr int SCORE_GRID = 2048;  // workgroups of the run launch at most: 16 runs each per sweep

struct ScoreLayout {
  size_t tmax, tsum, trow, total;  // byte offsets into the workspace
  int64_t tiles;
};

inline ScoreLayout score_layout(int L, int64_t S_total) {
  ScoreLayout a;
  a.tiles = (S_total + ROW_TILE - 1) / ROW_TILE;
  a.tmax = 0;                                                   // f64 [tiles][L]
  a.tsum = a.tmax + up256((size_t)a.tiles * L * 8);             // u64 [tiles][L]
  a.trow = a.tsum + up256((size_t)a.tiles * L * 8);             // i32 [tiles][L]: the global row of the maximum, -1: every row of the tile is NaN
  a.total = a.trow + up256((size_t)a.tiles * L * 4);
  return a;
}

struct Score {
  double m;  // the maximum so far; meaningless while r < 0
  int r;     // its global row, -1: nothing but NaN so far
  u64 s;     // sum of q32
};

__device__ __forceinline__ u64 q32(double p) {
  if (!(p == p)) return 0;
  p = p < 0.0 ? 0.0 : (p > 1.0 ? 1.0 : p);
  return (u64)__builtin_rint(p * 4294967296.0);  // the product is exact (a power of two), rint is round-half-even
}

__device__ __forceinline__ void score_merge(Score& a, double m, int r, u64 s) {
  a.s += s;
  if (r >= 0 && (a.r < 0 || m > a.m || (m == a.m && r < a.r))) {
    a.m = m;
    a.r = r;
  }
}

__device__ __forceinline__ void score_row(Score& a, double p, int row) { score_merge(a, p, p == p ? row : -1, q32(p)); }

__device__ __forceinline__ void score_shuffle(Score& a, int d) {  // every lane of the wave takes part
  const double m = __shfl_xor(a.m, d);
  const int r = __shfl_xor(a.r, d);
  const u64 s = __shfl_xor(a.s, d);
  score_merge(a, m, r, s);
}

// ---------------------------------------------------------------- S1 tiles.  lg = log2 of L rounded up to a power of two (Lp): thread = part * Lp + l
__global__ __launch_bounds__(256) void scores_tile_kernel(const double* __restrict__ agg, int L, int lg, int64_t S_total, double* __restrict__ tmax,
                                                           u64* __restrict__ tsum, int* __restrict__ trow) {
  __shared__ double wm[WAVES][64];
  __shared__ u64 wsum[WAVES][64];
  __shared__ int wrow[WAVES][64];
  const int64_t tile = blockIdx.x;
  const int Lp = 1 << lg, parts = ROW_TILE >> lg;
  const int l = threadIdx.x & (Lp - 1), part = threadIdx.x >> lg;
  Score a = {0.0, -1, 0};
  if (l < L) {
    const int64_t row0 = tile * ROW_TILE + part;  // rows row0, row0 + parts, ...: ascending, so the first maximum stays
    for (int k0 = 0; k0 < Lp; k0 += 8) {           // eight loads in flight, then their eight rows in order
      double v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t row = row0 + (int64_t)(k0 + j) * parts;
        v[j] = (k0 + j < Lp && row < S_total) ? agg[row * L + l] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t row = row0 + (int64_t)(k0 + j) * parts;
        if (k0 + j < Lp && row < S_total) score_row(a, v[j], (int)row);
      }
    }
  }
  for (int d = Lp; d < 64; d <<= 1) score_shuffle(a, d);  // the parts of this wave: lanes of equal l
  const int wave = threadIdx.x >> 6, lane = lane_id();
  wm[wave][lane] = a.m;
  wsum[wave][lane] = a.s;
  wrow[wave][lane] = a.r;
  __syncthreads();
  if (threadIdx.x < L) {  // lane l of every wave holds that wave's result for label l
    Score b = {0.0, -1, 0};
    for (int w = 0; w < WAVES; ++w) score_merge(b, wm[w][threadIdx.x], wrow[w][threadIdx.x], wsum[w][threadIdx.x]);
    tmax[tile * L + threadIdx.x] = b.m;
    tsum[tile * L + threadIdx.x] = b.s;
    trow[tile * L + threadIdx.x] = b.r;
  }
}

// ---------------------------------------------------------------- S2 runs
__global__ __launch_bounds__(256) void scores_run_kernel(const double* __restrict__ agg, int L, const int64_t* __restrict__ table, int R, int64_t S_total,
                                                          const int4* __restrict__ runs, const int64_t* __restrict__ offsets, int64_t capacity,
                                                          const double* __restrict__ tmax, const u64* __restrict__ tsum, const int* __restrict__ trow,
                                                          u64* __restrict__ scores, u64* __restrict__ eager, int64_t eager_runs) {
  constexpr int GROUPS = 256 / SCORE_LANES;
  int64_t n = offsets[R];
  if (n > capacity) n = capacity;  // runs behind the capacity were counted, not stored
  const int group = threadIdx.x / SCORE_LANES, g = threadIdx.x % SCORE_LANES;
  for (int64_t base = (int64_t)blockIdx.x * GROUPS; base < n; base += (int64_t)gridDim.x * GROUPS) {  // the same trips for every lane of the workgroup
    const int64_t i = base + group;
    Score a = {0.0, -1, 0};
    int64_t first = 0;
    if (i < n) {
      const int4 run = runs[i];
      int lo = 0, hi = R - 1;  // the last recording whose first run is <= i: the one that holds run i
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid - 1;
      }
      first = table[4 * lo + 3];
      const int l = run.z;
      int64_t b = first + run.x, e = first + run.y + 1;  // global rows [b, e)
      if (b < 0) b = 0;
      if (e > S_total) e = S_total;
      if (l >= 0 && l < L && b < e) {
        int64_t t0 = (b + ROW_TILE - 1) / ROW_TILE, t1 = e / ROW_TILE;  // whole tiles [t0, t1)
        int64_t head = t0 * ROW_TILE, tail = t1 * ROW_TILE;
        if (t0 >= t1) {  // no whole tile: one piece
          head = tail = e;
          t0 = t1 = 0;
        }
        for (int64_t row = b + g; row < head; row += SCORE_LANES) score_row(a, agg[row * L + l], (int)row);
        for (int64_t t = t0 + g; t < t1; t += SCORE_LANES) score_merge(a, tmax[t * L + l], trow[t * L + l], tsum[t * L + l]);
        for (int64_t row = tail + g; row < e; row += SCORE_LANES) score_row(a, agg[row * L + l], (int)row);
      }
    }
    for (int d = 1; d < SCORE_LANES; d <<= 1) score_shuffle(a, d);  // every lane of the group ends with the run's result
    if (i < n && g < 3) {
      const u64 word = g == 0 ? (u64)__double_as_longlong(a.r < 0 ? __builtin_nan("") : a.m) : (g == 1 ? a.s : (u64)(a.r < 0 ? (int64_t)-1 : (int64_t)a.r - first));
      scores[3 * i + g] = word;
      if (eager && i < eager_runs) eager[3 * i + g] = word;
    }
  }
}

}  // namespace

extern "C" {

size_t orcai_interval_scores_workspace_bytes(int L, int R, int64_t S_total) {
  if (L < 1 || L > 64 || R < 1 || S_total < 1 || S_total > 0x7fffffff) return 0;
  return score_layout(L, S_total).total;
}

int orcai_interval_scores(const double* agg, int L, const int64_t* table, int R, int64_t S_total, const int* runs, const int64_t* offsets, int64_t capacity,
                          void* scores, void* eager, int64_t eager_runs, void* workspace, size_t workspace_bytes, void* stream) {
  if (!agg || !table || !runs || !offsets || !scores || !workspace) return ORCAI_E_BADARG;
  if (L < 1 || L > 64 || R < 1 || S_total < 1 || capacity < 0 || eager_runs < 0) return ORCAI_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(runs) & 15) || (reinterpret_cast<uintptr_t>(scores) & 7) || (reinterpret_cast<uintptr_t>(eager) & 7) ||
      (reinterpret_cast<uintptr_t>(workspace) & 255))
    return ORCAI_E_BADARG;
  if (S_total > 0x7fffffff) return ORCAI_E_UNSUPPORTED;  // global rows are int32 in the tile table
  const ScoreLayout a = score_layout(L, S_total);
  if (workspace_bytes < a.total) return ORCAI_E_BADARG;
  char* ws = static_cast<char*>(workspace);
  double* tmax = reinterpret_cast<double*>(ws + a.tmax);
  u64* tsum = reinterpret_cast<u64*>(ws + a.tsum);
  int* trow = reinterpret_cast<int*>(ws + a.trow);
  int lg = 0;
  while ((1 << lg) < L) ++lg;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(scores_tile_kernel, dim3((unsigned)a.tiles), dim3(ROW_TILE), 0, st, agg, L, lg, S_total, tmax, tsum, trow);
  if (capacity > 0) {
    const int64_t want = (capacity + 256 / SCORE_LANES - 1) / (256 / SCORE_LANES);
    hipLaunchKernelGGL(scores_run_kernel, dim3((unsigned)(want < SCORE_GRID ? want : SCORE_GRID)), dim3(256), 0, st, agg, L, table, R, S_total,
                       reinterpret_cast<const int4*>(runs), offsets, capacity, tmax, tsum, trow, reinterpret_cast<u64*>(scores),
                       reinterpret_cast<u64*>(eager), eager_runs);
  }
  return (int)hipGetLastError();
}

size_t orcai_extract_labels_refined_workspace_bytes(int L, int R, int64_t S_total) {
  if (L < 1 || L > 64 || R < 1 || S_total < 1 || S_total > 0x7fffffff) return 0;
  return refine_layout(L, R, S_total).total;
}

int orcai_extract_labels_refined(const double* agg, const double* cnt, int L, const int64_t* table, int R, int64_t S_total, const double* thresholds,
                                 const double* high_thresholds, const int* gap_rows, const int* label_rank, const double* limits, double frame_seconds,
                                 int tpo, int* runs, int64_t capacity, int64_t* offsets, void* workspace, size_t workspace_bytes, void* stream) {
  if (!agg || !cnt || !table || !label_rank || !runs || !offsets || !workspace || !thresholds || !high_thresholds || !gap_rows) return ORCAI_E_BADARG;
  if (L < 1 || L > 64 || R < 1 || S_total < 1 || capacity < 0 || tpo < 1) return ORCAI_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(runs) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 255)) return ORCAI_E_BADARG;
  if (S_total > 0x7fffffff) return ORCAI_E_UNSUPPORTED;  // global rows are int32 in the candidate lists
  const RefineLayout a = refine_layout(L, R, S_total);
  if (workspace_bytes < a.total) return ORCAI_E_BADARG;
  char* ws = static_cast<char*>(workspace);
  double* thr = reinterpret_cast<double*>(ws + a.thr);
  u64 *lo = reinterpret_cast<u64*>(ws + a.lo), *hi = reinterpret_cast<u64*>(ws + a.hi), *keepbits = reinterpret_cast<u64*>(ws + a.keep);
  u64* edges = reinterpret_cast<u64*>(ws + a.edges);
  int64_t *cnt3 = reinterpret_cast<int64_t*>(ws + a.cnt3), *counts = reinterpret_cast<int64_t*>(ws + a.counts);
  int64_t* dummy = reinterpret_cast<int64_t*>(ws + a.dummy);
  int *cstart = reinterpret_cast<int*>(ws + a.cstart), *cstop = reinterpret_cast<int*>(ws + a.cstop), *hs = reinterpret_cast<int*>(ws + a.hs);
  int *he = reinterpret_cast<int*>(ws + a.he), *prevnz = reinterpret_cast<int*>(ws + a.prevnz), *nextnz = reinterpret_cast<int*>(ws + a.nextnz);
  int* stops = reinterpret_cast<int*>(ws + a.stops);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)a.tiles), block(ROW_TILE);
  const auto waves = [](int sequences) { return dim3((unsigned)((sequences + WAVES - 1) / WAVES)); };
  hipLaunchKernelGGL(labels_threshold_kernel, dim3((unsigned)R), block, 0, st, cnt, table, S_total, 0.0, true, thr);
  hipLaunchKernelGGL(refine_mask_kernel, grid, block, 0, st, agg, L, table, R, S_total, thr, thresholds, high_thresholds, lo, hi);
  hipLaunchKernelGGL(refine_count_kernel, grid, block, 0, st, lo, hi, L, table, R, S_total, a.tiles, cnt3);
  hipLaunchKernelGGL(labels_scan_kernel, waves(3 * L), block, 0, st, cnt3, 3 * L, a.tiles1, dummy);
  hipLaunchKernelGGL(refine_lists_kernel, grid, block, 0, st, lo, hi, L, table, R, S_total, a.tiles, cnt3, a.colcap, cstart, cstop, hs, he);
  hipLaunchKernelGGL(refine_keep_kernel, dim3((unsigned)((a.colcap + 255) / 256), (unsigned)L), block, 0, st, cnt3, a.tiles, a.colcap, a.words, hs, he, keepbits);
  hipLaunchKernelGGL(refine_words_kernel, waves(L), block, 0, st, cnt3, L, a.tiles, a.colcap, a.words, keepbits, prevnz, nextnz);
  hipLaunchKernelGGL(refine_edges_kernel, grid, block, 0, st, lo, L, table, R, S_total, a.tiles, cnt3, a.colcap, a.words, cstart, cstop, keepbits, prevnz, nextnz,
                     gap_rows, edges);
  hipLaunchKernelGGL(labels_count_kernel<true>, grid, block, 0, st, edges, L, table, R, S_total, a.tiles, counts);
  hipLaunchKernelGGL(labels_scan_kernel, waves(2 * L + 1), block, 0, st, counts, 2 * L + 1, a.tiles, offsets + R);
  hipLaunchKernelGGL(labels_stops_kernel<true>, grid, block, 0, st, edges, L, table, R, S_total, a.tiles, counts, a.colcap, stops);
  hipLaunchKernelGGL(labels_emit_kernel<true>, grid, block, 0, st, edges, L, table, R, S_total, a.tiles, counts, a.colcap, stops, label_rank, limits,
                     frame_seconds, tpo, reinterpret_cast<int4*>(runs), capacity, offsets);
  return (int)hipGetLastError();
}


size_t orcai_extract_labels_workspace_bytes(int L, int R, int64_t S_total) {
  if (L < 1 || L > 64 || R < 1 || S_total < 1) return 0;
  return layout(L, R, S_total).total;
}

int orcai_extract_labels(const double* agg, const double* cnt, int L, const int64_t* table, int R, int64_t S_total, double threshold,
                         const int* label_rank, const double* limits, double frame_seconds, int tpo, int* runs, int64_t capacity, int64_t* offsets,
                         void* workspace, size_t workspace_bytes, void* stream) {
  return extract_labels(agg, cnt, L, table, R, S_total, threshold, nullptr, label_rank, limits, frame_seconds, tpo, runs, capacity, offsets, workspace,
                        workspace_bytes, stream);
}

int orcai_extract_labels_per_label(const double* agg, const double* cnt, int L, const int64_t* table, int R, int64_t S_total, const double* thresholds,
                                   const int* label_rank, const double* limits, double frame_seconds, int tpo, int* runs, int64_t capacity,
                                   int64_t* offsets, void* workspace, size_t workspace_bytes, void* stream) {
  if (!thresholds) return ORCAI_E_BADARG;
  return extract_labels(agg, cnt, L, table, R, S_total, 0.0, thresholds, label_rank, limits, frame_seconds, tpo, runs, capacity, offsets, workspace,
                        workspace_bytes, stream);
}

}  // extern "C"
