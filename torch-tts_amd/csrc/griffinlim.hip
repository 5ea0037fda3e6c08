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
//   istft_kernel       one workgroup per run of F frames (F * n_fft = kTile; the RunLds of stft_run.h without samples): phase
//                      factors (given; or, from the second iteration on, (R_k - mom R_k-1) / (|R_k - mom R_k-1| + 1e-16) of the
//                      last two rebuilt spectra - `angles` and `tprev` of the reference are never stored) -> mag * phase -> inverse
//                      real FFT of n_fft points as one complex FFT of M = n_fft / 2 points (Z[k] = E[k] + i O[k], E = (X[k] +
//                      conj X[M-k]) / 2, O = (X[k] - conj X[M-k]) / 2 * conj W^k; ifft = conj fft conj / M; fft_lds.h) -> times
//                      the window -> frames [B, T, n_fft].
//   stft_kernel        the same run of frames forward (torch.stft(center=True, pad_mode="reflect")): its (F - 1) hop + n_fft
//                      samples are gathered from the inverse frames - each sample the sum, in frame order, of the <= n_fft / hop
//                      frames that cover it, divided by the same sum of the squared window (torch.istft's overlap-add, with no
//                      atomics and no waveform in memory) - reflected at the utterance's own two ends; then stft_run.h's
//                      forward_run, whose emit stores X[k], k <= M -> rebuilt [B, T, bins].
//   ola_kernel         that gather once more for the waveform itself, after the last inverse; peak_kernel: w / max |w| per utterance.
// The twiddles come from stft_run.h's launch_stft_tables.  LDS: with an even hop the samples and the window are read as 8-byte pairs
// (fft_lds.h fft_pass8_first_paired), spectra are read and written in bin order through swz().
// Nothing depends on the batch or on where a frame falls in its run: a ragged batch gives each utterance what it gets alone.
#include <math.h>
#include <stdint.h>

#include "kernels.h"
#include "stft_run.h"

using namespace ttsdec;

namespace {
constexpr int kThreads = kFftThreads;
constexpr int kMelFrames = 64;    // frames per workgroup of mel_to_mag_kernel (one per lane)
constexpr int kMelBins = 4;       // bins per thread and step
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

// grid (ceil(T / F), B); dynamic LDS run_lds_floats(n_fft, 0)
__global__ __launch_bounds__(kThreads) void istft_kernel(const GlArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = a.n_fft, M = N >> 1, bins = M + 1, F = a.F, T = a.T, lgM = a.lgM;
  const RunLds l = run_lds(lds, N);
  cf *tw = l.tw, *bufA = l.bufA, *bufB = l.bufB;
  const int b = blockIdx.y, t0 = blockIdx.x * F, tid = threadIdx.x;
  int flags;
  const int tb = frames_of(a.frames, b, T, &flags);
  if (flags && a.status && blockIdx.x == 0 && tid == 0) atomicOr(a.status, flags);
  if (t0 >= tb) return;  // (workgroup-uniform)
  load_tables(l, N, a.tw, a.window, N);
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
  const float2* win2 = reinterpret_cast<const float2*>(l.win);
  for (int idx = tid; idx < (F << lgM); idx += kThreads) {
    const int f = idx >> lgM, n = idx & (M - 1), t = t0 + f;
    if (t >= tb) continue;
    const cf v = Z[(f << lgM) + swz(n)];
    const float2 w = win2[n];
    reinterpret_cast<float2*>(a.fr + ((size_t)b * T + t) * N)[n] = make_float2(v.x * sc * w.x, -v.y * sc * w.y);
  }
}

// grid (ceil(T / F), B); dynamic LDS run_lds_floats(n_fft, scount)
__global__ __launch_bounds__(kThreads) void stft_kernel(const GlArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = a.n_fft, M = N >> 1, bins = M + 1, F = a.F, T = a.T, hop = a.hop;
  const RunLds l = run_lds(lds, N);
  const int b = blockIdx.y, t0 = blockIdx.x * F, tid = threadIdx.x;
  int flags;
  const int tb = frames_of(a.frames, b, T, &flags);
  if (t0 >= tb) return;  // (workgroup-uniform)
  load_tables(l, N, a.tw, a.window, N);
  __syncthreads();  // (ola_sample reads the window from LDS)
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
      v = ola_sample(frb, l.win, tb, N, hop, j);
    }
    l.samp[s] = v;
  }
  __syncthreads();
  // ---- transform and split step: X[k], k <= M, of the frames that exist ----
  cf* reb = a.reb + ((size_t)b * T + t0) * bins;
  forward_run(l, hop, !(hop & 1), M, a.lgM, F, [=](int f, int k, cf x, float*) {
    if (t0 + f >= tb) return;
    reb[(size_t)f * bins + k] = x;
  });
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

// [n_fft] twiddles; [B, T, bins] the magnitudes frame-major; two rebuilt spectra [B, T, bins]; [B, T, n_fft] windowed inverse frames
struct GlWs { cf* tw; float* mag; cf *ra, *rb; float* fr; };
GlWs carve_griffinlim(Carver& cv, size_t B, size_t T, size_t n_fft) {
  const size_t bt = B * T, bins = n_fft / 2 + 1;
  GlWs w;
  w.tw = reinterpret_cast<cf*>(cv.take(2 * n_fft));
  w.mag = cv.take(bt * bins);
  w.ra = reinterpret_cast<cf*>(cv.take(2 * bt * bins));
  w.rb = reinterpret_cast<cf*>(cv.take(2 * bt * bins));
  w.fr = cv.take(bt * n_fft);
  return w;
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
  Carver cv{nullptr};
  carve_griffinlim(cv, B, T, n_fft);
  return cv.bytes();
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
  Carver cv{static_cast<float*>(workspace)};
  const GlWs ws = carve_griffinlim(cv, B, T, n_fft);
  if (!workspace || workspace_bytes < cv.bytes() || (reinterpret_cast<uintptr_t>(workspace) & 255)) return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int bins = n_fft / 2 + 1;
  cf *cur = ws.ra, *prev = ws.rb;
  hipError_t e = hipSuccess;
  if (status) e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
  if (e == hipSuccess && n_iter > 0 && !tprev) e = hipMemsetAsync(prev, 0, (size_t)B * T * bins * sizeof(cf), st);
  if (e != hipSuccess) return hip_fail(base(h), e, "griffinlim");
  launch_stft_tables(ws.tw, n_fft, nullptr, nullptr, nullptr, 0, 0, bins, 0, nullptr, st);
  transpose<float>(mag, ws.mag, frames, B, T, bins, T, 1, st);
  if (angles) transpose<cf>(reinterpret_cast<const cf*>(angles), cur, frames, B, T, bins, T, 1, st);
  if (tprev && n_iter > 0) transpose<cf>(reinterpret_cast<const cf*>(tprev), prev, frames, B, T, bins, T, 1, st);

  GlArgs a;
  a.mag = ws.mag; a.ang_out = nullptr; a.fr = ws.fr; a.wave = wave; a.frames = frames; a.window = window; a.tw = ws.tw;
  a.status = status; a.mom = momentum / (1.f + momentum); a.T = T; a.n_fft = n_fft; a.lgM = lg2(n_fft / 2); a.hop = hop_length;
  a.F = run_frames(n_fft); a.scount = run_samples(n_fft, hop_length);
  const size_t lds_i = sizeof(float) * run_lds_floats(n_fft, 0), lds_f = sizeof(float) * run_lds_floats(n_fft, a.scount);
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
