// column_select.hip -- segmented radix select for gfx950 (MI355X): the exact rank-th smallest of EVERY COLUMN of an f32 [rows][cols] array in one call,
// the streaming subtraction of a per-column value, and the denoised front end built from them (per-channel noise floor: median subtraction in dB).
//
// Data flow (orcai_column_select):
//   clear      zero the global histograms u32[cols][256] (zero_async: a kernel node)
//   pass p=1..4  column_hist_kernel<p>   read x once; digit p of the key (bits [31:24], [23:16], [15:8], [7:0]) of every element whose higher digits
//                                        equal ITS OWN COLUMN's prefix -> LDS histogram of the workgroup's 32 columns -> non-zero bins added to global
//                column_scan_kernel<p>   one wave per column: histogram -> (digit, rank inside it); writes the column's {prefix, rank}, zeroes the
//                                        column's bins for the next pass; pass 4 writes out[c] = key2f(key)
// Four reads of x whatever the values; integer sums only, so two launches give the same bytes.  The order is f2key's (select_key.h), the one the flat
// radix select (frontend.hip) orders by: on one column the two return the same bits.
//
// The time-varying floor (orcai_segment_column_select, orcai_subtract_segment_floor, orcai_make_segment_denoised_spectrogram): the same
// select per (segment of rows, column) in ONE launch -- segment_select_kernel, histogram, scan and column state in LDS -- or, for few long segments, a loop
// of orcai_column_select calls (segment_select_fused is the rule), and the subtraction of the floor interpolated between the segment centres.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orcai_hip.h"
#include "select_key.h"
#include "zero_fill.h"

namespace {

constexpr int GROUP = 32;        // columns per workgroup: a row piece is one 128-byte run, a wave reads two rows
constexpr int BINS = 256;        // 8-bit digits
constexpr int LDS_ROW = BINS + 1;  // u32 per column in LDS: the odd stride puts equal digits of different columns into different banks
constexpr int MAX_COLS = 4096;
constexpr int MAX_BLOCKS = 1024;  // 256 compute units x the 4 workgroups of 32.1 KiB LDS each holds: the whole grid is resident at once
constexpr int UNROLL = 4;         // row tiles in flight per thread

struct ColState {
  uint32_t prefix;  // the key's digits found so far, lower bits 0
  uint32_t rank;    // 0-based rank of the wanted element among the column's elements with that prefix
};

__host__ __device__ constexpr int digit_shift(int pass) { return 32 - 8 * pass; }

// The scratch: u32[cols][256] histograms | ColState[cols] | f32[cols] spare (orcai_make_denoised_spectrogram keeps the profile there when none is asked)
inline size_t hist_bytes(int cols) { return (size_t)cols * BINS * sizeof(uint32_t); }
inline size_t state_bytes(int cols) { return (size_t)cols * sizeof(ColState); }

// lanes_log2: log2 of the lanes that share a row.  5 (a 32-column piece) whenever cols >= 32; with fewer columns the next power of two >= cols, so that
// a wave covers 64 >> lanes_log2 rows instead of idling most of its lanes.  blockIdx.y is the column group, blockIdx.x strides over the row tiles.
template <int PASS>
__global__ __launch_bounds__(256) void column_hist_kernel(const float* __restrict__ x, int64_t rows, int cols, int lanes_log2,
                                                          const ColState* __restrict__ state, uint32_t* __restrict__ hist) {
  constexpr int SH = digit_shift(PASS);
  __shared__ uint32_t h[GROUP * LDS_ROW];
  for (int i = threadIdx.x; i < GROUP * LDS_ROW; i += 256) h[i] = 0u;
  const int lc = threadIdx.x & ((1 << lanes_log2) - 1);  // column inside the group
  const int col = blockIdx.y * GROUP + lc;
  const bool col_ok = col < cols;
  uint32_t prefix = 0u;
  if (PASS > 1 && col_ok) prefix = state[col].prefix;
  __syncthreads();
  uint32_t* __restrict__ hc = h + lc * LDS_ROW;
  const int64_t tile_rows = 256 >> lanes_log2;
  const int64_t stride = (int64_t)gridDim.x * tile_rows;
  const float* __restrict__ xc = x + col;
  if (col_ok) {
    for (int64_t r = (int64_t)blockIdx.x * tile_rows + (threadIdx.x >> lanes_log2); r < rows; r += UNROLL * stride) {
      float v[UNROLL];
      bool live[UNROLL];
#pragma unroll
      for (int j = 0; j < UNROLL; ++j) {
        const int64_t rj = r + j * stride;
        live[j] = rj < rows;
        v[j] = live[j] ? xc[rj * cols] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < UNROLL; ++j) {
        const uint32_t key = f2key(v[j]);
        const bool in = live[j] && (PASS == 1 || ((key ^ prefix) >> (SH + 8)) == 0u);
        if (in) atomicAdd(&hc[(key >> SH) & 255u], 1u);
      }
    }
  }
  __syncthreads();
  uint32_t* __restrict__ g = hist + (int64_t)blockIdx.y * GROUP * BINS;
  const int group_cols = min(GROUP, cols - blockIdx.y * GROUP);
  for (int i = threadIdx.x; i < group_cols * BINS; i += 256) {
    const uint32_t c = h[(i >> 8) * LDS_ROW + (i & 255)];
    if (c) atomicAdd(&g[i], c);
  }
}

// One wave per column, 4 columns per workgroup.  Lane l holds bins 4l .. 4l + 3; an inclusive scan of the lane sums over the wave finds the one lane
// whose bins hold the rank, and that lane the bin.  Every lane zeroes the bins it read: the histogram is clear for the next pass (and the next call).
template <int PASS>
__global__ __launch_bounds__(256) void column_scan_kernel(uint32_t* __restrict__ hist, ColState* __restrict__ state, int cols, uint32_t rank0,
                                                          float* __restrict__ out) {
  constexpr int SH = digit_shift(PASS);
  const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (col >= cols) return;  // whole waves leave together
  const int lane = threadIdx.x & 63;
  uint32_t* __restrict__ hc = hist + (int64_t)col * BINS + lane * 4;
  uint32_t c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] = hc[j];
    hc[j] = 0u;
  }
  ColState s;
  if (PASS == 1) {
    s.prefix = 0u;
    s.rank = rank0;
  } else {
    s = state[col];
  }
  const uint32_t mine = c[0] + c[1] + c[2] + c[3];
  uint32_t incl = mine;  // the counts sum to at most rows < 2^32
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
    if (lane >= d) incl += up;
  }
  uint32_t before = incl - mine;
  if (s.rank >= before && s.rank < incl) {  // exactly one lane: the wanted element is among the column's elements with this prefix
    int bin = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (bin == j && s.rank >= before + c[j]) {
        before += c[j];
        bin = j + 1;
      }
    }
    const uint32_t key = s.prefix | ((uint32_t)(lane * 4 + bin) << SH);
    if (PASS == 4) {
      out[col] = key2f(key);
    } else {
      state[col].prefix = key;
      state[col].rank = s.rank - before;
    }
  }
}

// x[t][c] -= m[c] over the flat array: float4 where the address allows (from the first 16-byte boundary on), scalars before it and behind the last
// whole float4.  A thread's column advances by a constant per grid stride, so there is one 64-bit remainder per thread, not one per element.
__global__ __launch_bounds__(256) void subtract_columns_kernel(float* __restrict__ x, int64_t n, int cols, int head, const float* __restrict__ m) {
  const int64_t n4 = (n - head) >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  float4* __restrict__ x4 = reinterpret_cast<float4*>(x + head);
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int c = (int)((head + 4 * i) % cols);
  const int step = (int)((4 * stride) % cols);
  const auto wrap = [cols](int k) {
    while (k >= cols) k -= cols;
    return k;
  };
  for (; i < n4; i += stride) {
    float4 v = x4[i];
    v.x -= m[c];
    v.y -= m[wrap(c + 1)];
    v.z -= m[wrap(c + 2)];
    v.w -= m[wrap(c + 3)];
    x4[i] = v;
    c += step;
    if (c >= cols) c -= cols;
  }
  if (blockIdx.x == 0) {
    for (int64_t k = threadIdx.x; k < head; k += 256) x[k] -= m[k % cols];
    for (int64_t k = head + (n4 << 2) + threadIdx.x; k < n; k += 256) x[k] -= m[k % cols];
  }
}

// ---- the time-varying floor: one select per (segment, column), and the subtraction of the floor interpolated between segment centres ----
// Rows are cut into S = max(1, rows / seg_rows) segments of seg_rows rows; the last one takes the remainder (seg_rows .. 2 seg_rows - 1 rows, or all the
// rows when S == 1).
constexpr int SEG_UNROLL = 8;        // row tiles in flight per thread of the fused kernel: a workgroup keeps 8 KiB of loads in the air
constexpr int SEG_TILE_ROWS = 256 / GROUP;

struct Segments {
  int64_t S, W, n_last;  // segments, rows of a full one, rows of the last
};
__host__ __device__ inline Segments make_segments(int64_t rows, int64_t seg_rows) {
  const int64_t S = rows / seg_rows > 0 ? rows / seg_rows : 1;
  return Segments{S, seg_rows, rows - (S - 1) * seg_rows};
}

// One workgroup = one (segment, group of 32 adjacent columns), all four digit passes: histogram of the slab in LDS, scan in LDS, the column state
// {prefix, rank} in LDS, the slab (n_s rows x 128 bytes) read again by the next pass.  Nothing global but the loads of x and one store per column.
// Thread = (row of the tile, column of the group); with fewer than 32 columns in the group the other lanes idle (no lane packing: a segment is short).
__global__ __launch_bounds__(256) void segment_select_kernel(const float* __restrict__ x, int cols, Segments sg, uint32_t rank, uint32_t rank_last,
                                                             float* __restrict__ out) {
  __shared__ uint32_t h[GROUP * LDS_ROW];
  __shared__ ColState st[GROUP];
  const int64_t s = blockIdx.x;
  const int64_t n = s == sg.S - 1 ? sg.n_last : sg.W;
  const int lc = threadIdx.x & (GROUP - 1);
  const int col = blockIdx.y * GROUP + lc;
  const bool col_ok = col < cols;
  const int group_cols = min(GROUP, cols - blockIdx.y * GROUP);
  const float* __restrict__ xc = x + s * sg.W * cols + (col_ok ? col : 0);
  uint32_t* __restrict__ hc = h + lc * LDS_ROW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < GROUP) st[threadIdx.x] = ColState{0u, s == sg.S - 1 ? rank_last : rank};
#pragma unroll
  for (int pass = 1; pass <= 4; ++pass) {
    const int sh = digit_shift(pass);
    for (int i = threadIdx.x; i < GROUP * LDS_ROW; i += 256) h[i] = 0u;
    __syncthreads();  // the zeroes, and the state the scan of the pass before wrote
    const uint32_t prefix = st[lc].prefix;
    if (col_ok) {
      for (int64_t r = threadIdx.x >> 5; r < n; r += SEG_UNROLL * SEG_TILE_ROWS) {
        float v[SEG_UNROLL];
        bool live[SEG_UNROLL];
#pragma unroll
        for (int j = 0; j < SEG_UNROLL; ++j) {
          const int64_t rj = r + j * SEG_TILE_ROWS;
          live[j] = rj < n;
          v[j] = live[j] ? xc[rj * cols] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < SEG_UNROLL; ++j) {
          const uint32_t key = f2key(v[j]);
          const bool in = live[j] && (pass == 1 || ((key ^ prefix) >> (sh + 8)) == 0u);
          if (in) atomicAdd(&hc[(key >> sh) & 255u], 1u);
        }
      }
    }
    __syncthreads();
    // the scan of column_scan_kernel on the LDS rows: wave w takes columns w, w + 4, ...; lane l holds bins 4l .. 4l + 3
    for (int c = wave; c < group_cols; c += 4) {
      uint32_t cnt[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) cnt[j] = h[c * LDS_ROW + lane * 4 + j];
      const ColState cs = st[c];
      const uint32_t mine = cnt[0] + cnt[1] + cnt[2] + cnt[3];
      uint32_t incl = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += up;
      }
      uint32_t before = incl - mine;
      if (cs.rank >= before && cs.rank < incl) {  // exactly one lane
        int bin = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          if (bin == j && cs.rank >= before + cnt[j]) {
            before += cnt[j];
            bin = j + 1;
          }
        }
        const uint32_t key = cs.prefix | ((uint32_t)(lane * 4 + bin) << sh);
        if (pass == 4) {
          out[s * cols + blockIdx.y * GROUP + c] = key2f(key);
        } else {
          st[c] = ColState{key, cs.rank - before};  // read by every lane of this wave above, and by nobody else before the next barrier
        }
      }
    }
    __syncthreads();  // the histogram is zeroed and the state read only behind this
  }
}

// The floor of row t: F = m[s] where `lerp` is false, else fl32(m[s] + fl32(a * fl32(m[s + 1] - m[s]))).  Doubled integer coordinates: u = 2 t, the
// centre of segment s at c2_s = 2 s W + n_s - 1; held constant outside the first and the last centre.  a = float(double / double): two roundings, as
// the specification (denoise.segment_denoise_ref) has them.
struct RowFloor {
  int64_t s;
  float a;
  bool lerp;
};
__device__ __forceinline__ RowFloor row_floor(int64_t t, const Segments& sg) {
  const int64_t u = 2 * t, c2_first = sg.S > 1 ? sg.W - 1 : sg.n_last - 1, c2_last = 2 * (sg.S - 1) * sg.W + sg.n_last - 1;
  if (u <= c2_first) return RowFloor{0, 0.0f, false};
  if (u >= c2_last) return RowFloor{sg.S - 1, 0.0f, false};
  int64_t s = (u - (sg.W - 1)) / (2 * sg.W);  // S > 1 here; the centres of the full segments are 2 W apart
  if (s > sg.S - 2) s = sg.S - 2;            // behind where a full last segment's centre would be, in front of the long one's
  const int64_t c2 = 2 * s * sg.W + sg.W - 1, c2_next = s + 1 == sg.S - 1 ? c2_last : c2 + 2 * sg.W;
  return RowFloor{s, (float)((double)(u - c2) / (double)(c2_next - c2)), true};
}
// Every operation rounded on its own.  HIP's __fmul_rn / __fadd_rn are plain operators, which the compiler's default contraction still fuses: the pragma
// is what keeps the multiply and the add apart (the only f32 v_fmac left in the kernel belong to the 64-bit integer divisions).
__device__ __forceinline__ float floor_at(const RowFloor& f, const float* __restrict__ m, int cols, int c) {
#pragma clang fp contract(off)
  const float m0 = m[f.s * cols + c];
  if (!f.lerp) return m0;
  const float d = m[(f.s + 1) * cols + c] - m0;
  const float ad = f.a * d;
  return m0 + ad;
}
__device__ __forceinline__ float minus_floor(float v, const RowFloor& f, const float* __restrict__ m, int cols, int c) {
#pragma clang fp contract(off)
  const float F = floor_at(f, m, cols, c);
  return v - F;
}

// x[t][c] -= F[t][c] over the flat array, shaped as subtract_columns_kernel is: float4 from the first 16-byte boundary on, scalars in front and behind.
// A thread keeps its (row, column) and advances both by constants per grid stride; the row's {s, a} is computed in the kernel, once per float4 and again
// only where the float4 crosses into the next row -- per row piece, never per element.
__global__ __launch_bounds__(256) void subtract_segment_floor_kernel(float* __restrict__ x, int64_t n, int cols, int head, Segments sg,
                                                                     const float* __restrict__ m) {
  const int64_t n4 = (n - head) >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  float4* __restrict__ x4 = reinterpret_cast<float4*>(x + head);
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int64_t t = (head + 4 * i) / cols;
  int c = (int)((head + 4 * i) % cols);
  const int64_t step_t = (4 * stride) / cols;
  const int step_c = (int)((4 * stride) % cols);
  for (; i < n4; i += stride) {
    float4 v = x4[i];
    float* e = reinterpret_cast<float*>(&v);
    int64_t tj = t;
    int cj = c;
    RowFloor f = row_floor(tj, sg);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      e[j] = minus_floor(e[j], f, m, cols, cj);
      if (++cj == cols && j < 3) {
        cj = 0;
        f = row_floor(++tj, sg);
      }
    }
    x4[i] = v;
    t += step_t;
    c += step_c;
    if (c >= cols) {
      c -= cols;
      ++t;
    }
  }
  if (blockIdx.x == 0) {
    for (int64_t k = threadIdx.x; k < head; k += 256) x[k] = minus_floor(x[k], row_floor(k / cols, sg), m, cols, (int)(k % cols));
    for (int64_t k = head + (n4 << 2) + threadIdx.x; k < n; k += 256) x[k] = minus_floor(x[k], row_floor(k / cols, sg), m, cols, (int)(k % cols));
  }
}

// Which route a segmented select takes, decided once (as sep_route.h decides the convs'): the fused kernel launches S x ceil(cols / 32) workgroups, each
// walking its own slab four times, so it is as slow as its longest segment -- a workgroup alone gets through a row of its slab (128 bytes, four passes)
// in about 61 ns, 8.4 GB/s, whatever the rest of the chip does; a loop of orcai_column_select calls puts the whole chip on one row range after the other
// and pays 8 launches and a clear, about 45 us, per segment.  Fused while the longest segment's walk is no longer than the loop's launches; same bytes
// either way.  Both constants are measured (profiles/segment_denoise_mi355x.json): the hour at 48 kHz goes fused at 1 s, 10 s and 60 s
// segments and to the loop at 600 s, for K = 171 and 64 alike, each by a factor of 3.9 or more.
constexpr int64_t FUSED_ROW_NS = 61, SELECT_CALL_NS = 45000;
inline bool segment_select_fused(const Segments& sg, int /*cols*/) {
  const int64_t longest = sg.n_last;  // >= W, or all the rows when S == 1
  return longest * FUSED_ROW_NS <= sg.S * SELECT_CALL_NS;
}

inline bool segment_args_ok(int64_t rows, int cols, int64_t seg_rows) { return rows > 0 && rows < ((int64_t)1 << 32) && cols >= 1 && cols <= MAX_COLS && seg_rows >= 1; }
inline bool segment_ranks_ok(const Segments& sg, int64_t rank, int64_t rank_last) {
  return rank_last >= 0 && rank_last < sg.n_last && (sg.S == 1 || (rank >= 0 && rank < sg.W));  // with one segment no full one exists: rank is not read
}
inline size_t segment_spare_offset(int cols) { return hist_bytes(cols) + state_bytes(cols); }

int segment_select_fused_launch(const float* x, int cols, const Segments& sg, int64_t rank, int64_t rank_last, float* out, hipStream_t s) {
  if (sg.S > 0x7fffffff) return ORCAI_E_BADARG;
  const dim3 grid((unsigned)sg.S, (unsigned)((cols + GROUP - 1) / GROUP));
  hipLaunchKernelGGL(segment_select_kernel, grid, dim3(256), 0, s, x, cols, sg, (uint32_t)rank, (uint32_t)rank_last, out);
  return (int)hipGetLastError();
}

inline bool column_args_ok(int64_t rows, int cols) { return rows > 0 && rows < ((int64_t)1 << 32) && cols >= 1 && cols <= MAX_COLS; }

}  // namespace

extern "C" {

size_t orcai_column_select_scratch_bytes(int cols) {
  if (cols < 1 || cols > MAX_COLS) return 0;
  return hist_bytes(cols) + state_bytes(cols) + (size_t)cols * sizeof(float);
}

int orcai_column_select(const float* x, int64_t rows, int cols, int64_t rank, float* out, void* scratch, void* stream) {
  if (!x || !out || !scratch || !column_args_ok(rows, cols) || rank < 0 || rank >= rows || ((uintptr_t)x & 3) || ((uintptr_t)out & 3) ||
      ((uintptr_t)scratch & 3))
    return ORCAI_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* hist = (uint32_t*)scratch;
  ColState* state = (ColState*)((char*)scratch + hist_bytes(cols));
  const hipError_t e = orcai_zero::zero_async(hist, hist_bytes(cols), s);  // a stale or never-cleared scratch: nothing of it is read (pass 1 writes the state whole)
  if (e != hipSuccess) return (int)e;
  int lanes_log2 = 5;
  while (lanes_log2 > 0 && (1 << (lanes_log2 - 1)) >= cols) --lanes_log2;
  const int groups = (cols + GROUP - 1) / GROUP;
  const int64_t tile_rows = 256 >> lanes_log2, tiles = (rows + tile_rows - 1) / tile_rows;
  const int64_t cap = MAX_BLOCKS / groups > 0 ? MAX_BLOCKS / groups : 1;
  const dim3 grid((unsigned)(tiles < cap ? tiles : cap), (unsigned)groups), scan((unsigned)((cols + 3) / 4));
  const uint32_t r = (uint32_t)rank;
  hipLaunchKernelGGL(column_hist_kernel<1>, grid, dim3(256), 0, s, x, rows, cols, lanes_log2, (const ColState*)state, hist);
  hipLaunchKernelGGL(column_scan_kernel<1>, scan, dim3(256), 0, s, hist, state, cols, r, out);
  hipLaunchKernelGGL(column_hist_kernel<2>, grid, dim3(256), 0, s, x, rows, cols, lanes_log2, (const ColState*)state, hist);
  hipLaunchKernelGGL(column_scan_kernel<2>, scan, dim3(256), 0, s, hist, state, cols, r, out);
  hipLaunchKernelGGL(column_hist_kernel<3>, grid, dim3(256), 0, s, x, rows, cols, lanes_log2, (const ColState*)state, hist);
  hipLaunchKernelGGL(column_scan_kernel<3>, scan, dim3(256), 0, s, hist, state, cols, r, out);
  hipLaunchKernelGGL(column_hist_kernel<4>, grid, dim3(256), 0, s, x, rows, cols, lanes_log2, (const ColState*)state, hist);
  hipLaunchKernelGGL(column_scan_kernel<4>, scan, dim3(256), 0, s, hist, state, cols, r, out);
  return (int)hipGetLastError();
}

int orcai_subtract_columns(float* x, int64_t rows, int cols, const float* m, void* stream) {
  if (!x || !m || !column_args_ok(rows, cols) || ((uintptr_t)x & 3) || ((uintptr_t)m & 3)) return ORCAI_E_BADARG;
  const int64_t n = rows * (int64_t)cols;
  int64_t head = (int64_t)((16 - ((uintptr_t)x & 15)) & 15) / 4;  // floats in front of the first 16-byte boundary
  if (head > n) head = n;
  int64_t blocks = ((n - head) / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(subtract_columns_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, cols, (int)head, m);
  return (int)hipGetLastError();
}

int orcai_make_denoised_spectrogram(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k, const int* band_lo, const int* band_hi,
                                    const int* band_off, const float* weights, int n_weights, int64_t rank_col, int64_t rank_lo, int64_t rank_hi, float top_db,
                                    float* out, float* profile, void* scratch, void* workspace, void* stream) {
  const int64_t n = n_frames * (int64_t)k;
  if (!workspace || !out || !scratch || ((uintptr_t)scratch & 3) || ((uintptr_t)profile & 3) || !column_args_ok(n_frames, k) || rank_col < 0 ||
      rank_col >= n_frames || rank_lo < 0 || rank_hi < 0 || rank_lo >= n || rank_hi >= n || ((uintptr_t)out & 15))
    return ORCAI_E_BADARG;  // what the later steps would refuse, before the first one runs
  float* m = profile ? profile : (float*)((char*)scratch + hist_bytes(k) + state_bytes(k));
  int e = orcai_frontend_reset(workspace, stream);
  if (e) return e;
  e = band_lo ? orcai_stft_mel_db(pcm, n_samples, n_fft, hop, n_frames, k, band_lo, band_hi, band_off, weights, n_weights, out, workspace, stream)
              : orcai_stft_db(pcm, n_samples, n_fft, hop, n_frames, k, out, workspace, stream);
  if (e) return e;
  e = orcai_frontend_finalize(1, top_db, workspace, stream);  // ref_db and the floor; the two bounds it forms are overwritten below
  if (e) return e;
  e = orcai_db_reference(out, n, workspace, stream);
  if (e) return e;
  e = orcai_column_select(out, n_frames, k, rank_col, m, scratch, stream);
  if (e) return e;
  e = orcai_subtract_columns(out, n_frames, k, m, stream);
  if (e) return e;
  e = orcai_quantile_select_radix(out, n, rank_lo, rank_hi, workspace, stream);  // the denoised values are not dB-shaped: the level-1 map is cut for dB
  if (e) return e;
  e = orcai_frontend_finalize(0, 0.0f, workspace, stream);
  if (e) return e;
  return orcai_clip_normalize(out, n, workspace, stream);
}

size_t orcai_segment_column_select_scratch_bytes(int64_t rows, int cols, int64_t seg_rows) {
  if (!segment_args_ok(rows, cols, seg_rows)) return 0;
  return segment_spare_offset(cols) + (size_t)make_segments(rows, seg_rows).S * cols * sizeof(float);
}

int orcai_segment_column_select_route(int64_t rows, int cols, int64_t seg_rows) {
  if (!segment_args_ok(rows, cols, seg_rows)) return ORCAI_E_BADARG;
  return segment_select_fused(make_segments(rows, seg_rows), cols) ? 1 : 0;
}

static int segment_select_checked(const float* x, int64_t rows, int cols, int64_t seg_rows, int64_t rank, int64_t rank_last, float* out, void* scratch,
                                  bool need_scratch) {
  if (!x || !out || (need_scratch && !scratch) || !segment_args_ok(rows, cols, seg_rows) || ((uintptr_t)x & 3) || ((uintptr_t)out & 3) || ((uintptr_t)scratch & 3))
    return ORCAI_E_BADARG;
  return segment_ranks_ok(make_segments(rows, seg_rows), rank, rank_last) ? 0 : ORCAI_E_BADARG;
}

int orcai_segment_column_select_fused(const float* x, int64_t rows, int cols, int64_t seg_rows, int64_t rank, int64_t rank_last, float* out, void* stream) {
  const int e = segment_select_checked(x, rows, cols, seg_rows, rank, rank_last, out, nullptr, false);
  if (e) return e;
  return segment_select_fused_launch(x, cols, make_segments(rows, seg_rows), rank, rank_last, out, (hipStream_t)stream);
}

int orcai_segment_column_select(const float* x, int64_t rows, int cols, int64_t seg_rows, int64_t rank, int64_t rank_last, float* out, void* scratch,
                                void* stream) {
  int e = segment_select_checked(x, rows, cols, seg_rows, rank, rank_last, out, scratch, true);
  if (e) return e;
  const Segments sg = make_segments(rows, seg_rows);
  if (segment_select_fused(sg, cols)) return segment_select_fused_launch(x, cols, sg, rank, rank_last, out, (hipStream_t)stream);
  for (int64_t s = 0; s < sg.S && !e; ++s) {  // few, long segments: the whole chip on one row range after the other
    const bool last = s == sg.S - 1;
    e = orcai_column_select(x + s * sg.W * cols, last ? sg.n_last : sg.W, cols, last ? rank_last : rank, out + s * cols, scratch, stream);
  }
  return e;
}

int orcai_subtract_segment_floor(float* x, int64_t rows, int cols, int64_t seg_rows, const float* m, void* stream) {
  if (!x || !m || !segment_args_ok(rows, cols, seg_rows) || ((uintptr_t)x & 3) || ((uintptr_t)m & 3)) return ORCAI_E_BADARG;
  const int64_t n = rows * (int64_t)cols;
  int64_t head = (int64_t)((16 - ((uintptr_t)x & 15)) & 15) / 4;  // floats in front of the first 16-byte boundary
  if (head > n) head = n;
  int64_t blocks = ((n - head) / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(subtract_segment_floor_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, cols, (int)head,
                     make_segments(rows, seg_rows), m);
  return (int)hipGetLastError();
}

int orcai_make_segment_denoised_spectrogram(const float* pcm, int64_t n_samples, int n_fft, int hop, int64_t n_frames, int k, const int* band_lo,
                                            const int* band_hi, const int* band_off, const float* weights, int n_weights, int64_t seg_rows, int64_t rank_seg,
                                            int64_t rank_seg_last, int64_t rank_lo, int64_t rank_hi, float top_db, float* out, float* profile, void* scratch,
                                            void* workspace, void* stream) {
  const int64_t n = n_frames * (int64_t)k;
  if (!workspace || !out || !scratch || ((uintptr_t)scratch & 3) || ((uintptr_t)profile & 3) || !segment_args_ok(n_frames, k, seg_rows) ||
      !segment_ranks_ok(make_segments(n_frames, seg_rows), rank_seg, rank_seg_last) || rank_lo < 0 || rank_hi < 0 || rank_lo >= n || rank_hi >= n ||
      ((uintptr_t)out & 15))
    return ORCAI_E_BADARG;  // what the later steps would refuse, before the first one runs
  float* m = profile ? profile : (float*)((char*)scratch + segment_spare_offset(k));
  int e = orcai_frontend_reset(workspace, stream);
  if (e) return e;
  e = band_lo ? orcai_stft_mel_db(pcm, n_samples, n_fft, hop, n_frames, k, band_lo, band_hi, band_off, weights, n_weights, out, workspace, stream)
              : orcai_stft_db(pcm, n_samples, n_fft, hop, n_frames, k, out, workspace, stream);
  if (e) return e;
  e = orcai_frontend_finalize(1, top_db, workspace, stream);
  if (e) return e;
  e = orcai_db_reference(out, n, workspace, stream);
  if (e) return e;
  e = orcai_segment_column_select(out, n_frames, k, seg_rows, rank_seg, rank_seg_last, m, scratch, stream);
  if (e) return e;
  e = orcai_subtract_segment_floor(out, n_frames, k, seg_rows, m, stream);
  if (e) return e;
  e = orcai_quantile_select_radix(out, n, rank_lo, rank_hi, workspace, stream);
  if (e) return e;
  e = orcai_frontend_finalize(0, 0.0f, workspace, stream);
  if (e) return e;
  return orcai_clip_normalize(out, n, workspace, stream);
}

}  // extern "C"
