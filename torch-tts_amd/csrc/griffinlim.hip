// Mel -> waveform for the Tacotron path (include/ttsdec.h ttsdec_mel_to_magnitude / ttsdec_griffinlim): the reference's
// tacotron/inference.py:13-22 synth_audio with AudioFrontend.mel_inv / .decode (tacotron/data/audio.py:69-76) - torchaudio's
// InverseMelScale, amplitude_to_DB, DB_to_amplitude and GriffinLim (fast Griffin-Lim, Perraudin et al. 2013) - on a padded batch
// with per-utterance frame counts.
//
//   mel_to_mag_kernel  m_rev -> db_to_amplitude -> P M -> relu -> amplitude_to_db -> db_to_amplitude -> sqrt in one pass.  P =
//                      fb (fb^T fb)^-1 [bins, n_mels] is the minimum-norm solution operator of fb^T D = M (what lstsq(driver="gels")
//                      returns for the full-row-rank fb^T), made once on the host in fp64.  Vector ALU: 64 frames x 4 bins per
//                      thread quartet, the mel tile in LDS as [mel][64 + 1], P rows through wave-uniform loads; K = n_mels = 80 and
//                      3 GFLOP at 64 x 600 frames leave nothing for the matrix pipe to win.
//   transpose_kernel   [B, bins, T] <-> [B, T, bins] (fp32 or complex): the iteration works frame-major, where a frame's spectrum is
//                      one contiguous row; the caller's tensors keep torch's [B, bins, T].  Writes zeros at frames >= frames[b].
//   istft_kernel       one workgroup per run of F frames (F * n_fft = kTile): phase factors (given; or, from the second iteration
//                      on, (R_k - mom R_k-1) / (|R_k - mom R_k-1| + 1e-16) of the last two rebuilt spectra - `angles` and `tprev` of
//                      the reference are never stored) -> mag * phase -> inverse real FFT of n_fft points as one complex FFT of
//                      M = n_fft / 2 points (Z[k] = E[k] + i O[k], E = (X[k] + conj X[M-k]) / 2, O = (X[k] - conj X[M-k]) / 2 *
//                      conj W^k; ifft = conj fft conj / M; fft_lds.h) -> times the window -> frames [B, T, n_fft].
//   stft_kernel        the same run of frames forward (torch.stft(center=True, pad_mode="reflect")): its (F - 1) hop + n_fft
//                      samples are gathered from the inverse frames - each sample the sum, in frame order, of the <= n_fft / hop
//                      frames that cover it, divided by the same sum of the squared window (torch.istft's overlap-add, with no
//                      atomics and no waveform in memory) - reflected at the utterance's own two ends, windowed, transformed and
//                      split to X[k], k <= M -> rebuilt [B, T, bins].
//   ola_kernel         that gather once more for the waveform itself, after the last inverse; peak_kernel: w / max |w| per utterance.
// LDS: the samples and the window are read as 8-byte pairs (lanes on consecutive pairs: every bank once per 32-lane group; the
// 4-byte reads at stride 2 of spec.hip's first pass are 2-way), spectra are read and written in bin order through swz().
// Nothing depends on the batch or on where a frame falls in its run: a ragged batch gives each utterance what it gets alone.
#include <math.h>
#include <stdint.h>

#include "fft_lds.h"
#include "kernels.h"

using namespace ttsdec;

namespace {
constexpr int kThreads = kFftThreads;
constexpr int kTile = 4096;       // floats of one LDS image of a run: F frames x n_fft / 2 complex points
constexpr int kMaxMels = 256;
constexpr int kMelFrames = 64;    // frames per workgroup of mel_to_mag_kernel (one per lane)
constexpr int kMelBins = 4;       // bins per thread and step
constexpr int kMaxFrames = 1 << 22;
enum { FLAG_SHORT = 1, FLAG_RANGE = 4 };  // status word: fewer than 2 frames (the row is zeros); frames[b] beyond T (clamped)
enum { PH_ONES = 0, PH_GIVEN = 1, PH_UPDATE = 2 };

inline HandleBase* base(ttsdec_handle* h) { return reinterpret_cast<HandleBase*>(h); }

// frames of utterance b that take part (0: refused), and its flags
__device__ inline int frames_of(const int* __restrict__ frames, int b, int T, int* flags) {
  int tb = frames ? frames[b] : T, fl = 0;
  if (tb > T) { fl |= FLAG_RANGE; tb = T; }
  if (tb < 2) { fl |= FLAG_SHORT; tb = 0; }
  *flags = fl;
  return tb;
}

// ---------------------------------------------------------------------------------------------------------------------------
// mel -> magnitude.  grid (ceil(T / 64), B); dynamic LDS n_mels * 65 floats
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void mel_to_mag_kernel(const float* __restrict__ y, const float* __restrict__ P, const int* __restrict__ frames,
                                                              int T, int n_mels, int bins, float* __restrict__ mag, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int ms = kMelFrames + 1;
  const int b = blockIdx.y, t0 = blockIdx.x * kMelFrames, tid = threadIdx.x;
  int flags;
  const int tb = frames_of(frames, b, T, &flags);
  if (flags && status && blockIdx.x == 0 && tid == 0) atomicOr(status, flags);
  const float* yb = y + (size_t)b * T * n_mels;
  if (t0 < tb) {  // (workgroup-uniform)
    for (int idx = tid; idx < kMelFrames * n_mels; idx += kThreads) {
      const int f = idx / n_mels, m = idx - f * n_mels, t = t0 + f;
      // m_rev (dataset.py:183-184), then db_to_amplitude(ref 1, power 1)
      lds[m * ms + f] = t < tb ? powf(10.f, 0.1f * (yb[(size_t)t * n_mels + m] * 100.f - 100.f)) : 0.f;
    }
  }
  __syncthreads();
  const int f = tid & (kMelFrames - 1), t = t0 + f;
  const int kg = __builtin_amdgcn_readfirstlane(tid / kMelFrames);  // one wave, one group of bins: P is read wave-uniformly
  float* mb = mag + (size_t)b * bins * T;
  for (int k0 = kg * kMelBins; k0 < bins; k0 += (kThreads / kMelFrames) * kMelBins) {
    float acc[kMelBins];
    const float* row[kMelBins];
#pragma unroll
    for (int i = 0; i < kMelBins; ++i) {
      acc[i] = 0.f;
      row[i] = P + (size_t)(k0 + i < bins ? k0 + i : bins - 1) * n_mels;
    }
    if (t0 < tb) {
      for (int m = 0; m < n_mels; ++m) {
        const float v = lds[m * ms + f];
#pragma unroll
        for (int i = 0; i < kMelBins; ++i) acc[i] = fmaf(row[i][m], v, acc[i]);
      }
    }
    if (t >= T) continue;
#pragma unroll
    for (int i = 0; i < kMelBins; ++i) {
      if (k0 + i >= bins) break;
      float out = 0.f;
      if (t < tb) {
        const float d = fmaxf(acc[i], 0.f);                     // InverseMelScale's relu
        const float db = 10.f * log10f(fmaxf(d, 1e-12f));       // amplitude_to_db(10, 1e-12, 0)
        out = sqrtf(powf(10.f, 0.1f * db));                     // db_to_amplitude(1, 1), then the power spectrogram's root
      }
      mb[(size_t)(k0 + i) * T + t] = out;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// src [B, R, C] -> dst [B, C, R]; the frame axis is the columns of src (frame_is_col) or its rows.  grid (ceil(C/32), ceil(R/32), B)
// ---------------------------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(kThreads) void transpose_kernel(const E* __restrict__ src, E* __restrict__ dst, const int* __restrict__ frames, int T, int R,
                                                             int C, int frame_is_col) {
  __shared__ E tile[32][33];
  const int b = blockIdx.z, r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  int flags;
  const int tb = frames_of(frames, b, T, &flags);
  const E* sb = src + (size_t)b * R * C;
  E* db = dst + (size_t)b * R * C;
  for (int i = ty; i < 32; i += kThreads / 32) {
    const int r = r0 + i, c = c0 + tx;
    E v = {};
    if (r < R && c < C && (frame_is_col ? c : r) < tb) v = sb[(size_t)r * C + c];
    tile[i][tx] = v;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += kThreads / 32) {
    const int c = c0 + i, r = r0 + tx;
    if (r < R && c < C) db[(size_t)c * R + r] = tile[tx][i];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the iteration
// ---------------------------------------------------------------------------------------------------------------------------
struct GlArgs {
  const float* mag;      // [B, T, bins]
  const cf* cur;         // [B, T, bins]: PH_GIVEN the phase factors, PH_UPDATE the last rebuilt spectrum
  const cf* prev;        // PH_UPDATE: the rebuilt spectrum before that (the reference's tprev)
  cf* ang_out;           // nullptr, or where the phase factors go (may be `prev`: every element is read, then written, by one thread)
  cf* reb;               // stft_kernel: [B, T, bins]
  float* fr;             // [B, T, n_fft] windowed inverse frames
  float* wave;           // ola_kernel: [B, hop * (T - 1)]
  const int* frames;     // [B] or nullptr
  const float* window;   // [n_fft]
  const cf* tw;          // [n_fft]
  int* status;           // or nullptr
  float mom;             // momentum / (1 + momentum)
  int mode, T, n_fft, lgM, hop, F, scount;
};

__device__ inline cf phase_at(const GlArgs& a, size_t o) {
  cf ph = {1.f, 0.f};
  if (a.mode == PH_GIVEN) {
    ph = a.cur[o];
  } else if (a.mode == PH_UPDATE) {
    const cf c = a.cur[o], p = a.prev[o];
    const cf d = {c.x - p.x * a.mom, c.y - p.y * a.mom};
    const float r = hypotf(d.x, d.y) + 1e-16f;
    ph = {d.x / r, d.y / r};
  }
  if (a.ang_out) a.ang_out[o] = ph;
  return ph;
}

// Sample j (0 <= j < hop (tb - 1)) of torch.istft's result from the windowed frames fr [tb, N] of one utterance
__device__ inline float ola_sample(const float* __restrict__ fr, const float* win, int tb, int N, int hop, int j) {
  const int p = j + N / 2;
  const int lo = p < N ? 0 : (p - N) / hop + 1;
  int hi = p / hop;
  hi = hi < tb - 1 ? hi : tb - 1;
  float acc = 0.f, env = 0.f;
  for (int t = lo; t <= hi; ++t) {
    const int n = p - t * hop;
    acc += fr[(size_t)t * N + n];
    env += win[n] * win[n];
  }
  return acc / env;
}

// grid (ceil(T / F), B); dynamic LDS 3 n_fft + 2 kTile floats
__global__ __launch_bounds__(kThreads) void istft_kernel(const GlArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = a.n_fft, M = N >> 1, bins = M + 1, F = a.F, T = a.T, lgM = a.lgM;
  cf* tw = reinterpret_cast<cf*>(lds);            // [N]
  float* win = lds + 2 * N;                       // [N]
  cf* bufA = reinterpret_cast<cf*>(lds + 3 * N);  // [F * M]
  cf* bufB = bufA + kTile / 2;
  const int b = blockIdx.y, t0 = blockIdx.x * F, tid = threadIdx.x;
  int flags;
  const int tb = frames_of(a.frames, b, T, &flags);
  if (flags && a.status && blockIdx.x == 0 && tid == 0) atomicOr(a.status, flags);
  if (t0 >= tb) return;  // (workgroup-uniform)
  for (int i = tid; i < N; i += kThreads) {
    tw[i] = a.tw[i];
    win[i] = a.window[i];
  }
  __syncthreads();
  // ---- mag * phase -> conj Z, bins k and M - k by one thread ----
  const int half = M / 2 + 1;
  for (int idx = tid; idx < F * half; idx += kThreads) {
    const int f = idx / half, k = idx - f * half, t = t0 + f;
    cf* z = bufA + (f << lgM);
    if (t >= tb) {  // a frame past the utterance's end: not stored below
      z[swz(k)] = {0.f, 0.f};
      if (k) z[swz(M - k)] = {0.f, 0.f};
      continue;
    }
    const size_t o = ((size_t)b * T + t) * bins;
    const int m = M - k;
    const cf pk = phase_at(a, o + k);
    const cf pm = m == k ? pk : phase_at(a, o + m);
    const float gk = a.mag[o + k], gm = a.mag[o + m];
    const cf xk = {gk * pk.x, gk * pk.y}, xm = {gm * pm.x, gm * pm.y};
    if (k == 0) {  // X[0] and X[M] count with their real parts (a real signal's are real)
      z[0] = {0.5f * (xk.x + xm.x), -(0.5f * (xk.x - xm.x))};
      continue;
    }
    const cf e = {0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y)};
    const cf d = {0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y)};
    const cf w = tw[k];
    const cf o2 = cmul(d, cf{w.x, -w.y});
    z[swz(k)] = {e.x - o2.y, -(e.y + o2.x)};  // conj (E + i O)
    z[swz(m)] = {e.x + o2.y, -(o2.x - e.y)};  // conj (conj E + i conj O)
  }
  __syncthreads();
  fft_pass<8, false>(bufA, bufB, tw, nullptr, nullptr, 0, M, lgM, 1, F);
  __syncthreads();
  const cf* Z = fft_rest(bufB, bufA, tw, M, lgM, F);
  // ---- x[2n] + i x[2n + 1] = conj Z[n] / M, times the window ----
  const float sc = 1.f / (float)M;
  const float2* win2 = reinterpret_cast<const float2*>(win);
  for (int idx = tid; idx < (F << lgM); idx += kThreads) {
    const int f = idx >> lgM, n = idx & (M - 1), t = t0 + f;
    if (t >= tb) continue;
    const cf v = Z[(f << lgM) + swz(n)];
    const float2 w = win2[n];
    reinterpret_cast<float2*>(a.fr + ((size_t)b * T + t) * N)[n] = make_float2(v.x * sc * w.x, -v.y * sc * w.y);
  }
}

// grid (ceil(T / F), B); dynamic LDS 3 n_fft + 2 kTile + scount floats
__global__ __launch_bounds__(kThreads) void stft_kernel(const GlArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = a.n_fft, M = N >> 1, bins = M + 1, F = a.F, T = a.T, lgM = a.lgM, hop = a.hop;
  cf* tw = reinterpret_cast<cf*>(lds);
  float* win = lds + 2 * N;
  cf* bufA = reinterpret_cast<cf*>(lds + 3 * N);
  cf* bufB = bufA + kTile / 2;
  float* samp = lds + 3 * N + 2 * kTile;  // [scount]
  const int b = blockIdx.y, t0 = blockIdx.x * F, tid = threadIdx.x;
  int flags;
  const int tb = frames_of(a.frames, b, T, &flags);
  if (t0 >= tb) return;  // (workgroup-uniform)
  for (int i = tid; i < N; i += kThreads) {
    tw[i] = a.tw[i];
    win[i] = a.window[i];
  }
  __syncthreads();
  // ---- the run's samples: overlap-add of the inverse frames, reflected at the utterance's own ends ----
  const float* frb = a.fr + (size_t)b * T * N;
  const int L = hop * (tb - 1), period = 2 * (L - 1);
  const int nf = tb - t0 < F ? tb - t0 : F;  // frames of the run that exist
  const int need = (nf - 1) * hop + N;
  for (int s = tid; s < a.scount; s += kThreads) {
    float v = 0.f;
    if (s < need) {
      int j = t0 * hop + s - N / 2;
      if (period == 0) {
        j = 0;
      } else {  // (an utterance no longer than n_fft / 2 samples is reflected more than once; torch refuses it)
        j %= period;
        if (j < 0) j += period;
        if (j >= L) j = period - j;
      }
      v = ola_sample(frb, win, tb, N, hop, j);
    }
    samp[s] = v;
  }
  __syncthreads();
  // ---- first radix-8 pass on the window-weighted samples, read as pairs ----
  if (hop & 1) {
    fft_pass<8, true>(nullptr, bufA, tw, samp, win, hop, M, lgM, 1, F);
  } else {
    const float2* s2 = reinterpret_cast<const float2*>(samp);
    const float2* w2 = reinterpret_cast<const float2*>(win);
    const int lgPer = lgM - 3, per = 1 << lgPer, fs2 = hop >> 1;
    for (int w = tid; w < (F << lgPer); w += kThreads) {
      const int f = w >> lgPer, j = w & (per - 1);
      cf v[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int i = j + (r << lgPer);
        const float2 s = s2[f * fs2 + i], ww = w2[i];
        v[r] = {s.x * ww.x, s.y * ww.y};
      }
      dft<8>(v);
#pragma unroll
      for (int r = 0; r < 8; ++r) bufA[(f << lgM) + swz((j << 3) + r)] = v[r];
    }
  }
  __syncthreads();
  const cf* Z = fft_rest(bufA, bufB, tw, M, lgM, F);
  // ---- split step: X[k] = E[k] + W^k O[k], k <= M ----
  for (int idx = tid; idx < bins * F; idx += kThreads) {
    const int f = idx / bins, k = idx - f * bins, t = t0 + f;
    if (t >= tb) continue;
    const cf zk = Z[(f << lgM) + swz(k & (M - 1))], zm = Z[(f << lgM) + swz((M - k) & (M - 1))];
    const cf xe = {0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)};
    const cf xo = {0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x)};
    a.reb[((size_t)b * T + t) * bins + k] = cadd(xe, cmul(tw[k], xo));
  }
}

// grid (ceil(hop (T - 1) / 256), B)
__global__ __launch_bounds__(kThreads) void ola_kernel(const GlArgs a) {
  const int b = blockIdx.y, j = blockIdx.x * kThreads + threadIdx.x, Lfull = a.hop * (a.T - 1);
  if (j >= Lfull) return;
  int flags;
  const int tb = frames_of(a.frames, b, a.T, &flags);
  float v = 0.f;
  if (tb && j < a.hop * (tb - 1)) v = ola_sample(a.fr + (size_t)b * a.T * a.n_fft, a.window, tb, a.n_fft, a.hop, j);
  a.wave[(size_t)b * Lfull + j] = v;
}

// w / max |w| over each utterance's own samples (inference.py:21).  grid B
__global__ __launch_bounds__(kThreads) void peak_kernel(float* __restrict__ wave, const int* __restrict__ frames, int T, int hop) {
  __shared__ float red[kThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  int flags;
  const int tb = frames_of(frames, b, T, &flags);
  if (!tb) return;
  const int L = hop * (tb - 1);
  float* w = wave + (size_t)b * hop * (T - 1);
  float m = 0.f;
  for (int j = tid; j < L; j += kThreads) m = fmaxf(m, fabsf(w[j]));
  red[tid] = m;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  m = red[0];
  for (int j = tid; j < L; j += kThreads) w[j] = w[j] / m;
}

// the twiddles (fft_lds.h) for k < n_fft.  grid n_fft / 256
__global__ __launch_bounds__(kThreads) void twiddle_kernel(cf* __restrict__ tw, int n_fft) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  tw[k] = twiddle(k, n_fft);
}


struct WsLayout { size_t tw, mag, ra, rb, fr, total; };
WsLayout ws_layout(int B, int T, int n_fft) {
  const size_t bt = (size_t)B * T, bins = n_fft / 2 + 1;
  WsLayout l;
  l.tw = 0;
  l.mag = l.tw + up((size_t)n_fft * sizeof(cf), 256);
  l.ra = l.mag + up(bt * bins * sizeof(float), 256);
  l.rb = l.ra + up(bt * bins * sizeof(cf), 256);
  l.fr = l.rb + up(bt * bins * sizeof(cf), 256);
  l.total = l.fr + up(bt * n_fft * sizeof(float), 256);
  return l;
}

int check_sizes(const ttsdec_handle* h, int B, int T, int n_fft, int hop) {
  if (!h || B <= 0 || T <= 0 || hop <= 0) return TTSDEC_ERR_INVALID_ARG;
  // (hop <= n_fft / 2: the overlap-added squared Hann window then has no zero inside the waveform)
  if (!fft_ok(n_fft) || hop > n_fft / 2 || T < 2 || T > kMaxFrames || B > 65535) return TTSDEC_ERR_DIMS;
  return TTSDEC_OK;
}

template <typename E>
void transpose(const E* src, E* dst, const int32_t* frames, int B, int T, int R, int C, int frame_is_col, hipStream_t st) {
  hipLaunchKernelGGL(transpose_kernel<E>, dim3((unsigned)((C + 31) / 32), (unsigned)((R + 31) / 32), (unsigned)B), dim3(kThreads), 0, st, src, dst,
                     frames, T, R, C, frame_is_col);
}

}  // namespace

extern "C" {

size_t ttsdec_griffinlim_workspace_bytes(const ttsdec_handle* h, int B, int T, int n_fft) {
  if (!h || B <= 0 || B > 65535 || T < 2 || T > kMaxFrames || !fft_ok(n_fft)) return 0;
  return ws_layout(B, T, n_fft).total;
}

int ttsdec_mel_to_magnitude(ttsdec_handle* h, const float* y, const float* P, const int32_t* frames, int B, int T, int n_mels, int n_fft, float* mag,
                            int32_t* status, void* stream) {
  if (!h || B <= 0 || T <= 0 || n_mels <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (!fft_ok(n_fft) || n_mels > kMaxMels || T < 2 || T > kMaxFrames || B > 65535) return TTSDEC_ERR_DIMS;
  if (!y || !P || !mag) return TTSDEC_ERR_INVALID_ARG;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (status) {
    const hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return hip_fail(base(h), e, "mel_to_magnitude");
  }
  const size_t lds = sizeof(float) * (size_t)n_mels * (kMelFrames + 1);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(mel_to_mag_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return record_hip_error(base(h), "hipFuncSetAttribute(mel_to_mag_kernel)");
  hipLaunchKernelGGL(mel_to_mag_kernel, dim3((unsigned)((T + kMelFrames - 1) / kMelFrames), (unsigned)B), dim3(kThreads), lds, st, y, P, frames, T, n_mels,
                     n_fft / 2 + 1, mag, status);
  return record_hip_error(base(h), "mel_to_magnitude");
}

int ttsdec_griffinlim(ttsdec_handle* h, const float* mag, const int32_t* frames, int B, int T, const float* window, int n_fft, int hop_length,
                      const float* angles, const float* tprev, int n_iter, float momentum, int normalize, float* wave, float* rebuilt_out,
                      float* angles_out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_sizes(h, B, T, n_fft, hop_length);
  if (rc != TTSDEC_OK) return rc;
  if (n_iter < 0 || !(momentum >= 0.f && momentum < 1.f)) return TTSDEC_ERR_INVALID_ARG;
  if (!mag || !window || !wave || ((rebuilt_out || angles_out) && n_iter == 0)) return TTSDEC_ERR_INVALID_ARG;
  const WsLayout l = ws_layout(B, T, n_fft);
  if (!workspace || workspace_bytes < l.total || (reinterpret_cast<uintptr_t>(workspace) & 255)) return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  const int bins = n_fft / 2 + 1;
  cf* tw = reinterpret_cast<cf*>(ws + l.tw);
  float* magT = reinterpret_cast<float*>(ws + l.mag);
  cf* cur = reinterpret_cast<cf*>(ws + l.ra);
  cf* prev = reinterpret_cast<cf*>(ws + l.rb);
  hipError_t e = hipSuccess;
  if (status) e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
  if (e == hipSuccess && n_iter > 0 && !tprev) e = hipMemsetAsync(prev, 0, (size_t)B * T * bins * sizeof(cf), st);
  if (e != hipSuccess) return hip_fail(base(h), e, "griffinlim");
  hipLaunchKernelGGL(twiddle_kernel, dim3((unsigned)(n_fft / kThreads)), dim3(kThreads), 0, st, tw, n_fft);
  transpose<float>(mag, magT, frames, B, T, bins, T, 1, st);
  if (angles) transpose<cf>(reinterpret_cast<const cf*>(angles), cur, frames, B, T, bins, T, 1, st);
  if (tprev && n_iter > 0) transpose<cf>(reinterpret_cast<const cf*>(tprev), prev, frames, B, T, bins, T, 1, st);

  GlArgs a;
  a.mag = magT; a.ang_out = nullptr; a.fr = reinterpret_cast<float*>(ws + l.fr); a.wave = wave; a.frames = frames; a.window = window; a.tw = tw;
  a.status = status; a.mom = momentum / (1.f + momentum); a.T = T; a.n_fft = n_fft; a.lgM = lg2(n_fft / 2); a.hop = hop_length;
  a.F = kTile / n_fft; a.scount = (a.F - 1) * hop_length + n_fft;
  const size_t lds_i = sizeof(float) * ((size_t)3 * n_fft + 2 * kTile), lds_f = lds_i + sizeof(float) * (size_t)a.scount;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(istft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_i) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(stft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_f) != hipSuccess)
    return record_hip_error(base(h), "hipFuncSetAttribute(griffinlim kernels)");
  const dim3 grid((unsigned)((T + a.F - 1) / a.F), (unsigned)B);
  // Iteration 0 reads the given phase factors from `cur` and leaves its rebuilt spectrum there; iteration k >= 1 reads the last two
  // rebuilt spectra and overwrites the older one, which the inverse of the same iteration was the last to need.
  for (int it = 0; it <= n_iter; ++it) {
    a.mode = it ? PH_UPDATE : (angles ? PH_GIVEN : PH_ONES);
    a.cur = cur;
    a.prev = prev;
    a.ang_out = (it == n_iter && angles_out) ? prev : nullptr;
    hipLaunchKernelGGL(istft_kernel, grid, dim3(kThreads), lds_i, st, a);
    if (it == n_iter) break;
    a.reb = it ? prev : cur;
    hipLaunchKernelGGL(stft_kernel, grid, dim3(kThreads), lds_f, st, a);
    if (it) { cf* t = cur; cur = prev; prev = t; }
  }
  const int Lfull = hop_length * (T - 1);
  hipLaunchKernelGGL(ola_kernel, dim3((unsigned)((Lfull + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads), 0, st, a);
  if (normalize) hipLaunchKernelGGL(peak_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, wave, frames, T, hop_length);
  if (rebuilt_out) transpose<cf>(cur, reinterpret_cast<cf*>(rebuilt_out), frames, B, T, T, bins, 0, st);
  if (angles_out) transpose<cf>(prev, reinterpret_cast<cf*>(angles_out), frames, B, T, T, bins, 0, st);
  return record_hip_error(base(h), "griffinlim");
}

}  // extern "C"
