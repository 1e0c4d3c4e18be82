// The body shared by spectrogram_bwd_kernel<NT> (MEL = false) and mel_spectrogram_bwd_kernel<NT> (MEL = true), included as TEXT inside each kernel:
// a __device__ function called from two one-line kernels made the compiler order the linear kernels' address arithmetic differently (same bits,
// 2.4 % slower on the hour at 512 / 256), and the linear kernels are to compile to the instructions they had.  The including kernel provides: the
// linear kernel's parameters under their names (k_crop = n_mels with MEL), `constexpr bool MEL`, `constexpr bool ENERGY`, `const MelBands* bands`,
// `const float* weights` (null without MEL) and `extern __shared__ float4 bwd_lds[]`.  ENERGY (orcai_stft_energy_bwd / orcai_stft_mel_energy_bwd): gout is
// the gradient w.r.t. the magnitude |X[k]| (linear) or the band power (MEL) itself -- no dB gates, no 10 / (ln 10 P); stats is null and never read, top_db
// unused.  DENOISE (orcai_denoised_spectrogram_bwd; the including kernel provides `constexpr bool DENOISE` and `const float* floor`, null without): the
// clip gates test fl32(v - floor[k]) as orcai_subtract_columns formed it, ref_db is recomputed from stats[0] = pmax as finalize_kernel computes it and
// stats[1] is never read; floor[k] is a plain global load beside g[k] (K floats, shared by every frame of every workgroup: the cache's), so the LDS
// layout and the launch plan are the plain kernels'.  Layout of bwd_lds: tw[n_fft/2] | per group: buf[n_fft] complex | per group:
// acc[run] | MEL: MelBwdLds.
  constexpr int GROUPS = 256 / NT;
  const int half = n_fft >> 1;
  float2* tw = reinterpret_cast<float2*>(bwd_lds);
  const int grp = threadIdx.x / NT, gid = threadIdx.x % NT;
  float2* buf = tw + half + grp * n_fft;
  float* acc = reinterpret_cast<float*>(tw + half + GROUPS * n_fft) + grp * run;
  MelBwdLds ml = {};
  if constexpr (MEL) {
    const int nb = (half + 4) & ~3;
    float* base = reinterpret_cast<float*>(tw + half + GROUPS * n_fft) + GROUPS * run;
    ml.dM = base + grp * k_crop;
    ml.widx_e = reinterpret_cast<uint16_t*>(base + GROUPS * k_crop);
    ml.widx_o = ml.widx_e + nb;
    ml.lo = ml.widx_o + nb;
    ml.n = ml.lo + k_crop;
    ml.off = ml.n + k_crop;
    ml.band_e = reinterpret_cast<uint8_t*>(ml.off + k_crop);
    ml.band_o = ml.band_e + nb;
    for (int k = threadIdx.x; k <= half; k += 256) {
      ml.widx_e[k] = 0xFFFFu;
      ml.widx_o[k] = 0xFFFFu;
      ml.band_e[k] = 0xFFu;
      ml.band_o[k] = 0xFFu;
    }
    __syncthreads();
    for (int m = threadIdx.x; m < k_crop; m += 256) {  // bands of one parity are disjoint: no two threads write one entry
      const int lo = bands->lo[m], nk = bands->n[m], off = bands->off[m];
      ml.lo[m] = (uint16_t)lo;
      ml.n[m] = (uint16_t)nk;
      ml.off[m] = (uint16_t)off;
      uint16_t* wi = (m & 1) ? ml.widx_o : ml.widx_e;
      uint8_t* bi = (m & 1) ? ml.band_o : ml.band_e;
      for (int j = 0; j < nk; ++j) {
        wi[lo + j] = (uint16_t)(off + j);
        bi[lo + j] = (uint8_t)(m >> 1);
      }
    }
  }
  for (int j = threadIdx.x; j < half; j += 256) {  // exp(-2 pi i j / n_fft)
    float sn, cs;
    sincospif(-2.0f * (float)j / (float)n_fft, &sn, &cs);
    tw[j] = make_float2(cs, sn);
  }
  __syncthreads();
  const float ref_db = ENERGY ? 0.0f : DENOISE ? power_to_db(stats[0]) : stats[1], p_lo = ENERGY ? 0.0f : stats[2], p_hi = ENERGY ? 0.0f : stats[3];
  const float range = p_hi - p_lo;
  auto window = [&](int n) { return 0.5f - 0.5f * (n < half ? tw[n].x : -tw[n - half].x); };  // periodic Hann: 0.5 - 0.5 cos(2 pi n / N)

  for (int64_t r = (int64_t)blockIdx.x * GROUPS + grp; r < n_runs; r += (int64_t)gridDim.x * GROUPS) {  // (NT == 256: uniform over the workgroup)
    const int64_t s0 = r * run;
    const int len = (int)(n_samples - s0 < run ? n_samples - s0 : run);
    for (int i = gid; i < len; i += NT) acc[i] = 0.0f;
    // frames with [t hop - N/2, t hop + N/2) meeting [s0, s0 + len)
    const int64_t t_lo = s0 - half < 0 ? 0 : (s0 - half) / hop + 1;
    int64_t t_hi = (s0 + len + half - 1) / hop;
    if (t_hi > n_frames - 1) t_hi = n_frames - 1;
    for (int64_t t = t_lo; t <= t_hi; ++t) {
      const int64_t base = t * hop - half;
      for (int n = gid; n < n_fft; n += NT) {
        const int64_t i = base + n;
        const float x = (i >= 0 && i < n_samples) ? pcm[i] : 0.0f;
        buf[n] = make_float2(x * window(n), 0.0f);
      }
      group_sync<NT>();
      for (int st = log2n; st >= 1; --st) {  // forward, decimation in frequency
        const int hm = 1 << (st - 1);
        for (int j = gid; j < half; j += NT) {
          const int k = j & (hm - 1);
          const int i0 = ((j >> (st - 1)) << st) + k, i1 = i0 + hm;
          const float2 w = tw[k << (log2n - st)];
          const float2 a = buf[i0], b = buf[i1];
          const float2 d = make_float2(a.x - b.x, a.y - b.y);
          buf[i0] = make_float2(a.x + b.x, a.y + b.y);
          buf[i1] = make_float2(fmaf(d.x, w.x, -d.y * w.y), fmaf(d.x, w.y, d.y * w.x));
        }
        group_sync<NT>();
      }
      const float* g = gout + t * (int64_t)k_crop;
      if constexpr (MEL && ENERGY) {  // the band power's own gradient: nothing to sum, nothing to gate
        for (int m = gid; m < k_crop; m += NT) ml.dM[m] = g[m];
        group_sync<NT>();
      } else if constexpr (MEL) {
        constexpr int SUB = NT == 64 ? 1 : 64;  // lanes per band
        const int sl = gid % SUB;
        for (int m = gid / SUB; m < k_crop; m += NT / SUB) {  // (SUB == 64: uniform over the wavefront)
          const int lo = ml.lo[m], nk = ml.n[m];
          const float* w = weights + ml.off[m];
          float M = 0.0f;
          for (int j = sl; j < nk; j += SUB) {
            const float2 z = buf[__brev((uint32_t)(lo + j)) >> (32 - log2n)];
            M = fmaf(w[j], fmaf(z.x, z.x, z.y * z.y), M);
          }
#pragma unroll
          for (int o = SUB / 2; o > 0; o >>= 1) M += __shfl_xor(M, o, 64);  // a + b == b + a: every lane holds the same bits
          float dM = 0.0f;
          if (M > AMIN_POW) {
            const float v = power_to_db(M) - ref_db;
            const float y = DENOISE ? sub_rounded_once(v, floor[m]) : v;  // the forward's Y = V - m[k], formed before it is compared
            if (v > -top_db && y > p_lo && y < p_hi) dM = (g[m] / range) * DB_GRAD / M;
          }
          if (sl == 0) ml.dM[m] = dM;
        }
        group_sync<NT>();
      }
      for (int p = gid; p < n_fft; p += NT) {  // X[k] -> G[k] where it stands
        const int k = (int)(__brev((uint32_t)p) >> (32 - log2n));
        float2 G = make_float2(0.0f, 0.0f);
        if constexpr (MEL) {
          if (k <= half) {
            const uint32_t we = ml.widx_e[k], wo = ml.widx_o[k];
            float dP = 0.0f;
            if (we != 0xFFFFu) dP = weights[we] * ml.dM[2 * ml.band_e[k]];
            if (wo != 0xFFFFu) dP = fmaf(weights[wo], ml.dM[2 * ml.band_o[k] + 1], dP);
            const float2 z = buf[p];
            G = make_float2(2.0f * z.x * dP, 2.0f * z.y * dP);
          }
        } else if (k < k_crop) {  // k_crop <= 1 + n_fft / 2
          const float2 z = buf[p];
          const float P = fmaf(z.x, z.x, z.y * z.y);
          if constexpr (ENERGY) {
            const float mag = sqrtf(P);
            if (mag > 0.0f) {  // d|X| / d(Re, Im) = (Re, Im) / |X|; exactly 0 at |X| = 0
              const float c = g[k] / mag;
              G = make_float2(z.x * c, z.y * c);
            }
          } else if (P > AMIN_POW) {
            const float v = power_to_db(P) - ref_db;
            const float y = DENOISE ? sub_rounded_once(v, floor[k]) : v;
            if (v > -top_db && y > p_lo && y < p_hi) {
              const float dP = (g[k] / range) * DB_GRAD / P;
              G = make_float2(2.0f * z.x * dP, 2.0f * z.y * dP);
            }
          }
        }
        buf[p] = G;
      }
      group_sync<NT>();
      for (int st = 1; st <= log2n; ++st) {  // inverse (unnormalised), decimation in time
        const int hm = 1 << (st - 1);
        for (int j = gid; j < half; j += NT) {
          const int k = j & (hm - 1);
          const int i0 = ((j >> (st - 1)) << st) + k, i1 = i0 + hm;
          const float2 w = tw[k << (log2n - st)];  // conjugated below
          const float2 a = buf[i0], b = buf[i1];
          const float2 tb = make_float2(fmaf(b.x, w.x, b.y * w.y), fmaf(b.y, w.x, -b.x * w.y));
          buf[i0] = make_float2(a.x + tb.x, a.y + tb.y);
          buf[i1] = make_float2(a.x - tb.x, a.y - tb.y);
        }
        group_sync<NT>();
      }
      for (int n = gid; n < n_fft; n += NT) {  // overlap-add: one thread per n, frames in order
        const int64_t q = base + n - s0;
        if (q >= 0 && q < len) acc[q] += window(n) * buf[n].x;
      }
      group_sync<NT>();
    }
    group_sync<NT>();
    for (int i = gid; i < len; i += NT) dpcm[s0 + i] = acc[i];
    group_sync<NT>();
  }
