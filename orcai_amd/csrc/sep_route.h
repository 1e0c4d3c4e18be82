// sep_route.h -- which kernel a k = 3 separable-conv launch gets, decided ONCE.  Host-only, plain C++ (no HIP header): the launchers
// of model_fwd.hip and half_fwd.hip consume the plan, the entry points that zero a buffer first refuse on it before touching
// anything, and orcai_sepconv_route reports it.  This file is the one statement of the rule.
//   window  one 64-pixel window per wave, no LDS (sepconv_kernel / sepconv_h_kernel): every shape, no epilogue beyond the depthwise-output store.
//   flat    8 consecutive windows per workgroup share their rows through LDS (sepconv_ftile_kernel / sepconv_h_ftile_kernel):
//           R = 1 planes, plane or x-pooled output, at most 24 chunks of 64 pixels and 64 KiB of LDS (with the epilogue's static
//           slots), planes below 2^27 vectors per snippet.
//   strip   8 rows x 64 columns per workgroup (sepconv_tile_kernel, f32 only): as flat without its chunk and LDS limits, and two
//           output tiles (17 .. 32 channels), at most 8 input quads, a plane wide_strips() accepts, tile mode 1, not EPI 3.
#pragma once
#include <cstddef>
#include <cstdint>

namespace orcai_route {
enum Route { kWindow = 0, kStrip = 1, kFlat = 2 };
// what the launch carries beyond the convolution (sets the static-LDS surcharge and whether strips are allowed): nothing; the
// depthwise-output store; + output statistics; + BatchNorm folded on load; the input-gradient passes' epilogues EPI 2 / EPI 3
enum Extras { kNone = 0, kDwStore = 1, kDwStats = 2, kDwStatsBn = 3, kEpi2 = 4, kEpi3 = 5 };
constexpr int kFlatWaves = 8;                    // windows per workgroup of the flat-tile kernels
constexpr int kMaxChunks = 3 * kFlatWaves;       // 64-pixel chunks of the shared row range: at most three per wave
constexpr size_t kLdsLimit = 64 * 1024;          // no kernel of this family opts in beyond the default
constexpr int64_t kMaxPlaneVectors = 1ll << 27;  // 16-byte vectors of one snippet's planes: 32-bit byte offsets in the tile kernels
constexpr int64_t kMaxPlanePixels = 1ll << 29;   // pixels of one padded plane, every kernel of the family
constexpr size_t kStatsBytesF16 = 4096 + 512;    // f16 statistics epilogue: static statistics slots and the folded input BatchNorm

struct Plan {
  Route route;
  int lo, VAL, tasks;  // a window's valid output lanes [lo, 64 - lo), VAL of them; windows covering the H image rows of a plane
  int nstrip, nchunk;  // strip: strips across the width; flat: 64-pixel chunks a workgroup stages
  size_t lds_bytes;    // flat: the launch's dynamic LDS
};

// strips of VAL columns across a plane W wide: their number if there are at least two with at most 15 % of their columns wasted, else 0
inline int wide_strips(int W, int VAL) {
  const int nstrip = (W + VAL - 1) / VAL;
  return nstrip >= 2 && W * 100 >= nstrip * VAL * 85 ? nstrip : 0;
}

// the one-window kernel of any tap size; the starting point of every plan
inline Plan window_plan(int ktap, int H, int WP, int out_layout) {
  const int lo = out_layout == 2 ? ((ktap / 2 + 1) & ~1) : ktap / 2;  // x-pooled output: windows start on an even pixel
  const int VAL = 64 - 2 * lo;
  return Plan{kWindow, lo, VAL, (int)(((int64_t)H * WP + VAL - 1) / VAL), 0, 0, 0};
}

inline bool tiles_eligible(int RP, int out_layout, Extras ex, int tile_mode) {
  const bool dw_store = ex >= kDwStore && ex <= kDwStatsBn;  // the x-pooled kernels have no depthwise-output store
  return tile_mode != 0 && RP == 1 && (out_layout == 0 || (out_layout == 2 && !dw_store));
}

// p as a flat-tile launch (its windows plus a plane row above and below, in 64-pixel chunks of 32 bytes per pixel; fixed_bytes for
// the weights, static_bytes declared by the kernel itself) if it fits, else p
inline Plan flat_if_it_fits(Plan p, int WP, size_t fixed_bytes, size_t static_bytes) {
  const int nchunk = ((kFlatWaves - 1) * p.VAL + 64 + 2 * WP + 63) / 64;
  const size_t lds_bytes = (size_t)nchunk * 64 * 32 + fixed_bytes;
  if (nchunk > kMaxChunks) return p;  // planes wider than ~500 pixels
  if (lds_bytes + static_bytes > kLdsLimit) return p;
  p.route = kFlat, p.nchunk = nchunk, p.lds_bytes = lds_bytes;
  return p;
}

inline Plan plan_f32(int Cin, int Cout, int H, int W, int WP, int RP, int out_layout, Extras ex, int tile_mode) {
  Plan p = window_plan(3, H, WP, out_layout);
  const int MT = (Cout + 15) / 16, CQ = (Cin + 3) / 4, CQo = (Cout + 3) / 4;
  if (!tiles_eligible(RP, out_layout, ex, tile_mode) || (int64_t)CQo * (H + 2) * WP >= kMaxPlaneVectors || (int64_t)CQ * (H + 2) * WP >= kMaxPlaneVectors)
    return p;
  const int nstrip = tile_mode == 1 && MT == 2 && CQ <= 8 && ex != kEpi3 ? wide_strips(W, p.VAL) : 0;
  if (nstrip) {
    p.route = kStrip, p.nstrip = nstrip;
    return p;
  }
  // static floats of the epilogue: statistics slots, BatchNorm constants, folded input BatchNorm.  EPI 3 has no slots of its own;
  // it is charged those of EPI 2, as orcai_sepconv_planes_epi always has.
  const size_t stats = (size_t)kFlatWaves * 4 * 8 * MT, bn_consts = (size_t)4 * MT * 16, in_bn = 128;
  const size_t statics = ex == kDwStats ? stats : ex == kDwStatsBn ? stats + in_bn : ex >= kEpi2 ? stats + bn_consts : 0;
  return flat_if_it_fits(p, WP, (size_t)(CQ * 64 * MT + 2 * MT * 16) * sizeof(float), statics * sizeof(float));
}

// f16: flat tiles or the one-window kernel (no strips); octet planes
inline Plan plan_f16(int Cin, int Cout, int H, int /*W*/, int WP, int RP, int out_layout, Extras ex, int tile_mode) {
  const Plan p = window_plan(3, H, WP, out_layout);
  const int MT = (Cout + 15) / 16, KG = ((Cin + 7) / 8 + 3) / 4;
  if (!tiles_eligible(RP, out_layout, ex, tile_mode) || (int64_t)((Cout + 7) / 8) * (H + 2) * WP >= kMaxPlaneVectors) return p;
  return flat_if_it_fits(p, WP, (size_t)KG * MT * 64 * 16, ex == kDwStats || ex == kDwStatsBn ? kStatsBytesF16 : 0);
}
}  // namespace orcai_route
