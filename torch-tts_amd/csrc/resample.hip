// Sample-rate conversion of a padded batch (include/ttsdec.h ttsdec_resample): torchaudio's functional.resample with its defaults
// (sinc_interp_hann), the first line of the reference's AudioFrontend.encode (tacotron/data/audio.py:55-58).  With g = gcd(orig, new),
// o = orig / g, n = new / g, base = min(o, n) * rolloff, width = ceil(lpw * o / base) and taps = 2 * width + o:
//   y[blk * n + p] = sum_k K[p, k] * xp[blk * o + k]        xp = x zero-padded by width on the left; K as in ttsdec.h
//
//   resample_table_kernel  the polyphase table, evaluated in fp64 and rounded once.  |t| reaches lpw outside the taps k with
//                          |k - width - o p / n| < h = lpw o / base; there the Hann factor is cos(pi / 2)^2 ~ 4e-33 and the rounded
//                          entry an exact zero.  So every phase keeps only the run [lo(p), lo(p) + L) of its taps, L = ceil(2 h) + 3
//                          (band_lo: one tap of margin on either side), stored run-relative and phase-minor: tab[i * n + p] =
//                          K[p, lo(p) + i].  At 441 / 320 that is 20 of 459 taps.  n * L <= n * taps words, the whole workspace.
//   resample_kernel        one workgroup per tile of G * R consecutive input blocks of one utterance.  The tile's (G R - 1) o + taps
//                          samples go to LDS once, zero outside [0, len) by index.  Work item w = g * n + p (lanes on consecutive w)
//                          owns phase p of the blocks g, g + G, ..., g + (R - 1) G: R accumulators, every table word read once per R
//                          outputs, each output one fp32 fma chain over its run in tap order.
// The one mapping covers both shape regimes.  Many phases (n >= 64: 441 / 320, 320 / 441, 441 / 160): G = 1, a wave's lanes are
// consecutive phases of one block; they read consecutive table words and write consecutive outputs, and their LDS reads start at
// lo(p), o / n words apart on average (by the ds_read_b32 rule, bank = word % 32 per 32-lane half: 2-way at 441 / 320 and 441 / 160,
// none at 320 / 441).  Few phases (3 / 1, 2 / 1, 1 / 2, 3 / 2): G = ceil(256 / n), lanes lie along blocks, the phase's table words
// are a broadcast, and with n == 1 the LDS reads are o words apart: an even o is a gcd(o, 32)-way conflict there.  For n == 1 and
// 4 | o the staged samples are skewed by one word per 32 (word a at a + a / 32): 4 / 1 goes from 4-way to none, measured 0.074 ->
// 0.068 ms at 64 x 10 s.  The 2-way conflict of 2 / 1 and 6 / 1 stays: the skew was measured there too and changed nothing (0.098 /
// 0.099 and 0.093 / 0.095 ms without / with it).  3 / 1 and 1 / 2 have no conflict to begin with.  o = 320 never has lanes along
// blocks: n = 441 there.
// Deterministic: no atomics but the status word; no sum depends on the batch, on n_out or on the tile an output falls in.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "kernels.h"

using namespace ttsdec;

namespace {
constexpr int kThreads = 256;
constexpr int kMaxR = 4;              // blocks per work item
constexpr int kWindowCap = 32768;     // staged samples per workgroup (128 KiB; + 4 KiB of skew)
enum { FLAG_RANGE = 4 };              // a length beyond the row / more output than n_out (the flag of the sibling calls)

inline HandleBase* base(ttsdec_handle* h) { return reinterpret_cast<HandleBase*>(h); }

struct Plan {
  int o, n, lpw, width, taps, L, G, R, window, skew;
  double base, h;  // min(o, n) * rolloff; lpw * o / base
};

int gcd_int(int a, int b) {
  while (b) { const int t = a % b; a = b; b = t; }
  return a;
}

// TTSDEC_OK and the plan, or the refusal of the sizes
int make_plan(int orig_freq, int new_freq, int lpw, float rolloff, Plan* pl) {
  if (orig_freq <= 0 || new_freq <= 0 || orig_freq == new_freq || lpw < 1 || !(rolloff > 0.f) || !(rolloff <= 1.f)) return TTSDEC_ERR_INVALID_ARG;
  const int g = gcd_int(orig_freq, new_freq);
  Plan p;
  p.o = orig_freq / g; p.n = new_freq / g; p.lpw = lpw;
  if (p.o > 1024 || p.n > 1024) return TTSDEC_ERR_DIMS;
  // rolloff travels as a float, the reference's is a double: the table takes the shortest decimal of 7 digits that gives this float
  // (0.99f is read as 0.99, not as 0.9900000095), so its fp64 values are the ones torch rounds
  char dec[32];
  snprintf(dec, sizeof dec, "%.7g", (double)rolloff);
  p.base = (double)(p.o < p.n ? p.o : p.n) * strtod(dec, nullptr);
  p.h = (double)lpw * p.o / p.base;
  const double taps = 2.0 * ceil(p.h) + p.o;
  if (taps > 16384.0) return TTSDEC_ERR_DIMS;
  p.width = (int)ceil(p.h);
  p.taps = 2 * p.width + p.o;
  p.L = (int)ceil(2.0 * p.h) + 3;
  if (p.L > p.taps) p.L = p.taps;
  // the tile: about kThreads work items, kMaxR blocks each, cut down until its samples fit (G R = 1: taps <= 16384 words)
  p.G = p.n >= kThreads ? 1 : (kThreads + p.n - 1) / p.n;
  p.R = kMaxR;
  while ((long long)(p.G * p.R - 1) * p.o + p.taps > kWindowCap) {
    if (p.R > 1) p.R >>= 1;
    else p.G = (p.G + 1) / 2;
  }
  p.window = (p.G * p.R - 1) * p.o + p.taps;
  p.skew = p.n == 1 && p.o % 4 == 0;
  *pl = p;
  return TTSDEC_OK;
}

// the workspace is the table alone: n * taps words (the runs fill n * L of them)
float* carve_resample(Carver& cv, const Plan& p) { return cv.take((size_t)p.n * p.taps); }
size_t table_bytes(const Plan& p) {
  Carver cv{nullptr};
  carve_resample(cv, p);
  return cv.bytes();
}

// first tap of phase p's run: one below the first k with |k - width - o p / n| < h (the same expression in both kernels)
__device__ inline int band_lo(int p, int o, int n, int width, double h) {
  const int lo = (int)floor((double)width + (double)o * (double)p / (double)n - h) - 1;
  return lo > 0 ? lo : 0;
}

// grid ceil(L * n / kThreads): tab[i * n + p] = K[p, lo(p) + i], zero past the last tap
__global__ __launch_bounds__(kThreads) void resample_table_kernel(float* __restrict__ tab, int o, int n, int lpw, int width, int taps, int L,
                                                                  double base, double h) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= L * n) return;
  const int i = idx / n, p = idx - i * n;
  const int k = band_lo(p, o, n, width, h) + i;
  float v = 0.f;
  if (k < taps) {  // the operation order of torchaudio's _get_sinc_resample_kernel, in fp64
    const double pi = 3.14159265358979323846;
    double t = (-(double)p / (double)n + (double)(k - width) / (double)o) * base;
    t = t < -(double)lpw ? -(double)lpw : (t > (double)lpw ? (double)lpw : t);
    const double c = cos(t * pi / (double)lpw / 2.0);
    const double win = c * c;
    t *= pi;
    const double s = t == 0.0 ? 1.0 : sin(t) / t;
    v = (float)(s * (win * (base / (double)o)));
  }
  tab[idx] = v;
}

struct RsArgs {
  const float* wav;    // [B, Nsamp]
  const int* lengths;  // [B] or nullptr
  const float* tab;    // [L, n]
  float* out;          // [B, n_out]
  int* lengths_out;    // [B] or nullptr
  int* status;         // or nullptr
  int Nsamp, n_out, o, n, width, taps, L, G, window, skew;
  double h;
};

// grid (ceil(ceil(n_out / n) / (G R)), B); dynamic LDS: window (+ window / 32) floats.  R is a template argument so that the
// tap loop is straight-line code: four table words requested together, then per tap R LDS words and R fmas.
template <int R>
__global__ __launch_bounds__(kThreads) void resample_kernel(const RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const int b = blockIdx.y, tid = threadIdx.x, o = a.o, n = a.n, G = a.G;
  const int skew = a.skew ? -1 : 0;
  // ---- the utterance: its samples, its outputs, its flag ----
  int len = a.lengths ? a.lengths[b] : a.Nsamp, flags = 0;
  if (len > a.Nsamp) { flags |= FLAG_RANGE; len = a.Nsamp; }
  if (len < 0) len = 0;
  long long m = ((long long)n * len + o - 1) / o;
  if (m > a.n_out) { flags |= FLAG_RANGE; m = a.n_out; }
  const long long mb = m;
  if (blockIdx.x == 0 && tid == 0) {
    if (flags && a.status) atomicOr(a.status, flags);
    if (a.lengths_out) a.lengths_out[b] = (int)mb;
  }
  const long long blk0 = (long long)blockIdx.x * (G * R), j0 = blk0 * n;  // first block and first output of the tile
  float* ob = a.out + (size_t)b * a.n_out;
  if (j0 >= mb) {  // (workgroup-uniform) nothing of this tile is a sample of the utterance
    const long long left = (long long)a.n_out - j0, all = (long long)G * R * n;
    const int nj = (int)(left < all ? left : all);
    for (int idx = tid; idx < nj; idx += kThreads) ob[j0 + idx] = 0.f;
    return;
  }
  // ---- the tile's samples, zero outside [0, len) whatever the row holds there ----
  const long long s0 = blk0 * o - a.width;
  const float* wb = a.wav + (size_t)b * a.Nsamp;
  for (int q = tid; q < a.window; q += kThreads) {
    const long long s = s0 + q;
    xs[q + ((q >> 5) & skew)] = s >= 0 && s < len ? wb[s] : 0.f;
  }
  __syncthreads();
  // ---- one fma chain per output, in tap order ----
  const int items = n * G, stride = G * o;
  for (int w = tid; w < items; w += kThreads) {
    const int g = w / n, p = w - g * n;
    const int lo = band_lo(p, o, n, a.width, a.h);
    const int cnt = a.L < a.taps - lo ? a.L : a.taps - lo;
    const float* __restrict__ tp = a.tab + p;
    const int x0 = g * o + lo;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    int i = 0;
    for (; i + 4 <= cnt; i += 4) {  // four table words in flight, then their 4 R fmas (still tap order)
      float kv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) kv[u] = tp[(size_t)(i + u) * n];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int q = x0 + r * stride + i + u;
          acc[r] = fmaf(kv[u], xs[q + ((q >> 5) & skew)], acc[r]);
        }
      }
    }
    for (; i < cnt; ++i) {
      const float kv = tp[(size_t)i * n];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int q = x0 + r * stride + i;
        acc[r] = fmaf(kv, xs[q + ((q >> 5) & skew)], acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long j = (blk0 + g + (long long)r * G) * n + p;
      if (j < a.n_out) ob[j] = j < mb ? acc[r] : 0.f;
    }
  }
}

}  // namespace

extern "C" {

size_t ttsdec_resample_workspace_bytes(const ttsdec_handle* h, int orig_freq, int new_freq, int lowpass_filter_width, float rolloff) {
  Plan p;
  if (!h || make_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, &p) != TTSDEC_OK) return 0;
  return table_bytes(p);
}

int ttsdec_resample(ttsdec_handle* h, const float* wave, const int32_t* lengths, int B, int n_samples, int orig_freq, int new_freq,
                    int lowpass_filter_width, float rolloff, float* out, int n_out, int32_t* lengths_out, int32_t* status, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (!h || B <= 0 || n_samples <= 0 || n_out <= 0) return TTSDEC_ERR_INVALID_ARG;
  Plan p;
  const int rc = make_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, &p);
  if (rc != TTSDEC_OK) return rc;
  if (B > 65535 || n_samples > (1 << 30) || n_out > (1 << 30)) return TTSDEC_ERR_DIMS;
  if (!wave || !out) return TTSDEC_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < table_bytes(p) || (reinterpret_cast<uintptr_t>(workspace) & 255)) return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (status) {
    const hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return hip_fail(base(h), e, "resample");
  }
  Carver cv{static_cast<float*>(workspace)};
  float* tab = carve_resample(cv, p);
  hipLaunchKernelGGL(resample_table_kernel, dim3((unsigned)((p.L * p.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, tab, p.o, p.n, p.lpw,
                     p.width, p.taps, p.L, p.base, p.h);
  RsArgs a;
  a.wav = wave; a.lengths = lengths; a.tab = tab; a.out = out; a.lengths_out = lengths_out; a.status = status;
  a.Nsamp = n_samples; a.n_out = n_out; a.o = p.o; a.n = p.n; a.width = p.width; a.taps = p.taps; a.L = p.L; a.G = p.G;
  a.window = p.window; a.skew = p.skew; a.h = p.h;
  const size_t lds = sizeof(float) * (size_t)(p.window + (p.skew ? p.window / 32 + 1 : 0));
  const int blocks = (n_out + p.n - 1) / p.n, tile = p.G * p.R;
  const dim3 grid((unsigned)((blocks + tile - 1) / tile), (unsigned)B);
  void (*kern)(const RsArgs) = p.R == 4 ? resample_kernel<4> : p.R == 2 ? resample_kernel<2> : resample_kernel<1>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return record_hip_error(base(h), "hipFuncSetAttribute(resample_kernel)");
  hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, st, a);
  return record_hip_error(base(h), "resample");
}

}  // extern "C"
