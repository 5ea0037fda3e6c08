// VITS2 spectrogram front-end (include/ttsdec.h ttsvits_spectrogram / ttsvits_spec_to_mel / ttsvits_mel_spectrogram): the reference's
// vits2/mel_processing.py:58-187 - reflect pad by (n_fft - hop) / 2 at each utterance's own ends, Hann-windowed STFT (center=False),
// sqrt(re^2 + im^2 + 1e-6), and for the mel forms log(clamp(mel_basis @ spec, 1e-5)).
//
//   spec_prep_kernel   the per-call tables in the workspace: exp(-2 pi i k / n_fft), k < n_fft, evaluated in fp64 and rounded once; and
//                      per mel row the run [lo, hi) of bins outside which the basis row is exactly zero (a triangular filterbank
//                      has ~2 * bins non-zeros in n_mels * bins entries; a dense basis just gets [0, bins)).
//   stft_kernel<MEL>   one workgroup per run of F consecutive frames of one utterance, F * n_fft = kTile.  The samples the run
//                      covers are loaded once ((F - 1) * hop + n_fft of them, reflected by index), each frame is the real FFT of
//                      n_fft points as a complex FFT of M = n_fft / 2 points z[n] = x[2n] + i x[2n + 1] plus the split step
//                      X[k] = (Z[k] + conj Z[M - k]) / 2 - i W^k (Z[k] - conj Z[M - k]) / 2.  The complex FFT is the Stockham
//                      autosort of fft_lds.h (shared with griffinlim.hip); the first pass reads the window-weighted samples.
//                      The magnitudes go to LDS as [bin][F + 1] and leave as [B, bins, T] with the run's frames contiguous,
//                      or - MEL - through the basis to [B, n_mels, T] without reaching memory.
//   mel_kernel         the same epilogue on a spec tile read from memory (ttsvits_spec_to_mel).
// Frames at or past an utterance's count are exact zeros.  No sum depends on the batch or on the position of a frame in its run.
#include <math.h>
#include <stdint.h>

#include "fft_lds.h"
#include "kernels.h"

using namespace ttsdec;

namespace {
constexpr int kThreads = kFftThreads;
constexpr int kTile = 4096;      // floats of one LDS image of a run: F frames x n_fft / 2 complex points
constexpr int kMelFrames = 16;   // frames per workgroup of mel_kernel (bins <= 513), half of it above
constexpr int kMaxMels = 256;
enum { FLAG_REFLECT = 1, FLAG_EMPTY = 2, FLAG_RANGE = 4 };  // status word: len <= pad; no frame; a length beyond the row / frames beyond T

inline HandleBase* base(ttsvits_handle* h) { return reinterpret_cast<HandleBase*>(h); }

// log(max(basis @ S, 1e-5)) of the tile S [bins][ss] (frames t0 .. t0 + F - 1 of utterance b) -> mel [n_mels, T] of that utterance
__device__ inline void mel_epilogue(const float* __restrict__ S, int ss, int bins, int F, int lgF, const float* __restrict__ basis,
                                    const int2* __restrict__ band, int n_mels, float* __restrict__ melb, int T, int t0, int tb) {
  for (int idx = threadIdx.x; idx < (n_mels << lgF); idx += kThreads) {
    const int m = idx >> lgF, f = idx & (F - 1), t = t0 + f;
    if (t >= T) continue;
    float val = 0.f;
    if (t < tb) {
      const int2 r = band[m];
      const float* row = basis + (size_t)m * bins;
      float acc = 0.f;
      for (int k = r.x; k < r.y; ++k) acc += row[k] * S[k * ss + f];
      val = logf(fmaxf(acc, 1e-5f));
    }
    melb[(size_t)m * T + t] = val;
  }
}

// frames of an utterance of len samples (0: refused), and its flags
__device__ inline int frames_of(int len, int Nsamp, int n_fft, int hop, int pad, int T, int* flags) {
  int fl = 0;
  if (len > Nsamp) { fl |= FLAG_RANGE; len = Nsamp; }
  int tb = 0;
  if (len <= pad) fl |= FLAG_REFLECT;
  else if (len + 2 * pad < n_fft) fl |= FLAG_EMPTY;
  else tb = 1 + (len + 2 * pad - n_fft) / hop;
  if (tb > T) { fl |= FLAG_RANGE; tb = T; }
  *flags = fl;
  return tb;
}

struct StftArgs {
  const float* wav;      // [B, Nsamp]
  const int* lengths;    // [B] or nullptr
  const float* window;   // [win]
  const cf* tw;          // [n_fft]
  const float* basis;    // [n_mels, bins] (MEL)
  const int2* band;      // [n_mels] (MEL)
  float* out;            // [B, bins, T], or [B, n_mels, T] (MEL)
  int* status;           // or nullptr
  int Nsamp, n_fft, lgM, hop, win, n_mels, T, F, lgF, scount;
};

template <bool MEL>
__global__ __launch_bounds__(kThreads) void stft_kernel(const StftArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = a.n_fft, M = N >> 1, bins = M + 1, F = a.F, T = a.T;
  cf* tw = reinterpret_cast<cf*>(lds);              // [N]
  float* win = lds + 2 * N;                         // [N]
  cf* bufA = reinterpret_cast<cf*>(lds + 3 * N);    // [F * M]
  cf* bufB = bufA + kTile / 2;                      // [F * M]
  float* samp = lds + 3 * N + 2 * kTile;            // [scount]
  const int b = blockIdx.y, t0 = blockIdx.x * F, tid = threadIdx.x;
  const int pad = (N - a.hop) / 2;
  int flags;
  const int len0 = a.lengths ? a.lengths[b] : a.Nsamp;
  const int tb = frames_of(len0, a.Nsamp, N, a.hop, pad, T, &flags);
  const int len = len0 < a.Nsamp ? len0 : a.Nsamp;
  if (flags && a.status && blockIdx.x == 0 && tid == 0) atomicOr(a.status, flags);
  const int rows = MEL ? a.n_mels : bins;
  float* outb = a.out + (size_t)b * rows * T;
  if (t0 >= tb) {  // (workgroup-uniform) nothing of this run is a frame of the utterance
    for (int idx = tid; idx < (rows << a.lgF); idx += kThreads) {
      const int t = t0 + (idx & (F - 1));
      if (t < T) outb[(size_t)(idx >> a.lgF) * T + t] = 0.f;
    }
    return;
  }
  // ---- tables and the run's samples ----
  for (int i = tid; i < N; i += kThreads) {
    tw[i] = a.tw[i];
    const int wl = (N - a.win) / 2, j = i - wl;
    win[i] = (j >= 0 && j < a.win) ? a.window[j] : 0.f;
  }
  const float* wb = a.wav + (size_t)b * a.Nsamp;
  const bool overlap = a.hop <= N;
  const int fs = overlap ? a.hop : N;
  const long long plen = (long long)len + 2 * pad;  // samples of the padded utterance
  for (int s = tid; s < a.scount; s += kThreads) {
    long long p;
    if (overlap) p = (long long)t0 * a.hop + s;
    else p = (long long)(t0 + s / N) * a.hop + s % N;
    float v = 0.f;
    if (p < plen) {
      long long j = p - pad;
      if (j < 0) j = -j;
      if (j >= len) j = 2 * ((long long)len - 1) - j;
      v = wb[j];
    }
    samp[s] = v;
  }
  __syncthreads();
  // ---- complex FFT of M points per frame ----
  const int lgM = a.lgM;
  fft_pass<8, true>(nullptr, bufA, tw, samp, win, fs, M, lgM, 1, F);
  __syncthreads();
  const cf* Z = fft_rest(bufA, bufB, tw, M, lgM, F);
  float* S = reinterpret_cast<float*>(Z == bufA ? bufB : bufA);
  // ---- split step and magnitude: S[k][f], k <= M ----
  const int ss = F + 1;
  for (int idx = tid; idx < bins * F; idx += kThreads) {
    const int f = idx / bins, k = idx - f * bins;
    const cf zk = Z[(f << lgM) + swz(k & (M - 1))], zm = Z[(f << lgM) + swz((M - k) & (M - 1))];
    const cf xe = {0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)};
    const cf xo = {0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x)};
    const cf x = cadd(xe, cmul(tw[k], xo));
    S[k * ss + f] = sqrtf((x.x * x.x + x.y * x.y) + 1e-6f);
  }
  __syncthreads();
  if (MEL) {
    mel_epilogue(S, ss, bins, F, a.lgF, a.basis, a.band, a.n_mels, outb, T, t0, tb);
  } else {
    for (int idx = tid; idx < (bins << a.lgF); idx += kThreads) {
      const int k = idx >> a.lgF, f = idx & (F - 1), t = t0 + f;
      if (t < T) outb[(size_t)k * T + t] = t < tb ? S[k * ss + f] : 0.f;
    }
  }
}

// grid (ceil(T / F), B); dynamic LDS bins * (F + 1) floats
__global__ __launch_bounds__(kThreads) void mel_kernel(const float* __restrict__ spec, const int* __restrict__ frames, int bins, int T, int F, int lgF,
                                                       const float* __restrict__ basis, const int2* __restrict__ band, int n_mels,
                                                       float* __restrict__ mel) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.y, t0 = blockIdx.x * F, ss = F + 1;
  int tb = frames ? frames[b] : T;
  tb = tb < 0 ? 0 : (tb > T ? T : tb);
  const float* sb = spec + (size_t)b * bins * T;
  if (t0 < tb) {  // (workgroup-uniform)
    for (int idx = threadIdx.x; idx < (bins << lgF); idx += kThreads) {
      const int k = idx >> lgF, f = idx & (F - 1), t = t0 + f;
      lds[k * ss + f] = t < T ? sb[(size_t)k * T + t] : 0.f;
    }
  }
  __syncthreads();
  mel_epilogue(lds, ss, bins, F, lgF, basis, band, n_mels, mel + (size_t)b * n_mels * T, T, t0, tb);
}

// blocks [0, n_fft / 256): the twiddles; then one block per mel row: its band
__global__ __launch_bounds__(kThreads) void spec_prep_kernel(cf* __restrict__ tw, int n_fft, const float* __restrict__ basis, int bins, int n_mels,
                                                             int2* __restrict__ band) {
  const int nb = n_fft / kThreads;
  if ((int)blockIdx.x < nb) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    tw[k] = twiddle(k, n_fft);
    return;
  }
  __shared__ int lo, hi;
  const int m = blockIdx.x - nb;
  if (threadIdx.x == 0) { lo = bins; hi = 0; }
  __syncthreads();
  int l = bins, h = 0;
  for (int k = threadIdx.x; k < bins; k += kThreads)
    if (basis[(size_t)m * bins + k] != 0.f) { l = l < k ? l : k; h = k + 1; }
  if (h) { atomicMin(&lo, l); atomicMax(&hi, h); }
  __syncthreads();
  if (threadIdx.x == 0) band[m] = hi > lo ? make_int2(lo, hi) : make_int2(0, 0);
}

size_t tw_bytes(int n_fft) { return up((size_t)n_fft * sizeof(cf), 256); }
size_t ws_bytes_of(int n_fft, int n_mels) { return tw_bytes(n_fft) + up((size_t)n_mels * sizeof(int2), 256); }

int check_wave(const ttsvits_handle* h, int B, int N, int n_fft, int hop, int win, int T) {
  if (!h || B <= 0 || N <= 0 || hop <= 0 || win <= 0 || T <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (!fft_ok(n_fft) || win > n_fft || B > 65535 || N > (1 << 30) || hop > (1 << 30)) return TTSDEC_ERR_DIMS;
  return TTSDEC_OK;
}

int check_ws(const void* ws, size_t bytes, int n_fft, int n_mels) {
  return (!ws || bytes < ws_bytes_of(n_fft, n_mels) || (reinterpret_cast<uintptr_t>(ws) & 255)) ? TTSDEC_ERR_WORKSPACE : TTSDEC_OK;
}

int run_stft(ttsvits_handle* h, const float* wav, const int32_t* lengths, int B, int N, const float* window, int n_fft, int hop, int win,
             const float* basis, int n_mels, float* out, int T, int32_t* status, void* ws, hipStream_t st, const char* what) {
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  const int bins = n_fft / 2 + 1;
  cf* tw = static_cast<cf*>(ws);
  int2* band = reinterpret_cast<int2*>(static_cast<char*>(ws) + tw_bytes(n_fft));
  if (status) {
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return hip_fail(base(h), e, what);
  }
  hipLaunchKernelGGL(spec_prep_kernel, dim3((unsigned)(n_fft / kThreads + n_mels)), dim3(kThreads), 0, st, tw, n_fft, basis, bins, n_mels, band);
  StftArgs a;
  a.wav = wav; a.lengths = lengths; a.window = window; a.tw = tw; a.basis = basis; a.band = band; a.out = out; a.status = status;
  a.Nsamp = N; a.n_fft = n_fft; a.lgM = lg2(n_fft / 2); a.hop = hop; a.win = win; a.n_mels = n_mels; a.T = T;
  a.F = kTile / n_fft; a.lgF = lg2(a.F);
  a.scount = hop <= n_fft ? (a.F - 1) * hop + n_fft : a.F * n_fft;
  const size_t lds = sizeof(float) * ((size_t)3 * n_fft + 2 * kTile + a.scount);
  const dim3 grid((unsigned)((T + a.F - 1) / a.F), (unsigned)B);
  auto kfn = n_mels ? stft_kernel<true> : stft_kernel<false>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return record_hip_error(base(h), "hipFuncSetAttribute(stft kernel)");
  hipLaunchKernelGGL(kfn, grid, dim3(kThreads), lds, st, a);
  return record_hip_error(base(h), what);
}

}  // namespace

extern "C" {

size_t ttsvits_spec_workspace_bytes(const ttsvits_handle* h, int n_fft, int n_mels) {
  if (!h || !fft_ok(n_fft) || n_mels < 0 || n_mels > kMaxMels) return 0;
  return ws_bytes_of(n_fft, n_mels);
}

int ttsvits_spectrogram(ttsvits_handle* h, const float* wav, const int32_t* lengths, int B, int N, const float* window, int n_fft, int hop_size,
                        int win_size, float* spec, int T, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_wave(h, B, N, n_fft, hop_size, win_size, T);
  if (rc != TTSDEC_OK) return rc;
  if (!wav || !window || !spec) return TTSDEC_ERR_INVALID_ARG;
  if ((rc = check_ws(workspace, workspace_bytes, n_fft, 0)) != TTSDEC_OK) return rc;
  return run_stft(h, wav, lengths, B, N, window, n_fft, hop_size, win_size, nullptr, 0, spec, T, status, workspace,
                  static_cast<hipStream_t>(stream), "spectrogram");
}

int ttsvits_mel_spectrogram(ttsvits_handle* h, const float* wav, const int32_t* lengths, int B, int N, const float* window, int n_fft, int hop_size,
                            int win_size, const float* mel_basis, int n_mels, float* mel, int T, int32_t* status, void* workspace,
                            size_t workspace_bytes, void* stream) {
  int rc = check_wave(h, B, N, n_fft, hop_size, win_size, T);
  if (rc != TTSDEC_OK) return rc;
  if (n_mels <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (n_mels > kMaxMels) return TTSDEC_ERR_DIMS;
  if (!wav || !window || !mel_basis || !mel) return TTSDEC_ERR_INVALID_ARG;
  if ((rc = check_ws(workspace, workspace_bytes, n_fft, n_mels)) != TTSDEC_OK) return rc;
  return run_stft(h, wav, lengths, B, N, window, n_fft, hop_size, win_size, mel_basis, n_mels, mel, T, status, workspace,
                  static_cast<hipStream_t>(stream), "mel_spectrogram");
}

int ttsvits_spec_to_mel(ttsvits_handle* h, const float* spec, const int32_t* frames, int B, int n_fft, int T, const float* mel_basis, int n_mels,
                        float* mel, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || B <= 0 || T <= 0 || n_mels <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (!fft_ok(n_fft) || n_mels > kMaxMels || B > 65535) return TTSDEC_ERR_DIMS;
  if (!spec || !mel_basis || !mel) return TTSDEC_ERR_INVALID_ARG;
  const int rc = check_ws(workspace, workspace_bytes, n_fft, n_mels);
  if (rc != TTSDEC_OK) return rc;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int bins = n_fft / 2 + 1;
  int2* band = reinterpret_cast<int2*>(static_cast<char*>(workspace) + tw_bytes(n_fft));
  hipLaunchKernelGGL(spec_prep_kernel, dim3((unsigned)n_mels), dim3(kThreads), 0, st, nullptr, 0, mel_basis, bins, n_mels, band);
  const int F = bins <= 513 ? kMelFrames : kMelFrames / 2;
  const size_t lds = sizeof(float) * (size_t)bins * (F + 1);
  hipLaunchKernelGGL(mel_kernel, dim3((unsigned)((T + F - 1) / F), (unsigned)B), dim3(kThreads), lds, st, spec, frames, bins, T, F, lg2(F), mel_basis,
                     band, n_mels, mel);
  return record_hip_error(base(h), "spec_to_mel");
}

}  // extern "C"
