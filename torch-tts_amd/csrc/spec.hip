// VITS2 spectrogram front-end (include/ttsdec.h ttsvits_spectrogram / ttsvits_spec_to_mel / ttsvits_mel_spectrogram): the reference's
// vits2/mel_processing.py:58-187 - reflect pad by (n_fft - hop) / 2 at each utterance's own ends, Hann-windowed STFT (center=False),
// sqrt(re^2 + im^2 + 1e-6), and for the mel forms log(clamp(mel_basis @ spec, 1e-5)).
//
//   (tables)           twiddles and, per mel row, the band of its non-zero bins, in the workspace: stft_run.h launch_stft_tables.
//   stft_kernel<MEL>   one workgroup per run of F consecutive frames of one utterance, F * n_fft = kTile: the frame run of
//                      stft_run.h - the samples the run covers loaded once ((F - 1) * hop + n_fft of them, reflected by index; frame
//                      by frame when hop > n_fft), the window centred, forward_run - with sqrt(|X|^2 + 1e-6) as its emit.
//                      The magnitudes go to LDS as [bin][F + 1] and leave as [B, bins, T] with the run's frames contiguous,
//                      or - MEL - through the basis to [B, n_mels, T] without reaching memory.
//   mel_kernel         the same epilogue on a spec tile read from memory (ttsvits_spec_to_mel).
// Frames at or past an utterance's count are exact zeros.  No sum depends on the batch or on the position of a frame in its run.
#include <math.h>
#include <stdint.h>

#include "kernels.h"
#include "stft_run.h"

using namespace ttsdec;

namespace {
constexpr int kThreads = kFftThreads;
constexpr int kMelFrames = 16;   // frames per workgroup of mel_kernel (bins <= 513), half of it above
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
      val = logf(fmaxf(band_dot(basis + (size_t)m * bins, 1, band[m], S, ss, f), 1e-5f));
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
  const RunLds l = run_lds(lds, N);
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
  load_tables(l, N, a.tw, a.window, a.win);
  const bool overlap = a.hop <= N;
  load_reflected(l.samp, a.scount, a.wav + (size_t)b * a.Nsamp, len, pad, t0, a.hop, N, overlap, [](float v) { return v; });
  __syncthreads();
  // ---- transform, split step and magnitude: S[k][f], k <= M ----
  const int ss = F + 1;
  const float* S = forward_run(l, overlap ? a.hop : N, false, M, a.lgM, F,
                               [ss](int f, int k, cf x, float* S) { S[k * ss + f] = sqrtf((x.x * x.x + x.y * x.y) + 1e-6f); });
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

struct SpecWs { cf* tw; int2* band; };  // [n_fft] twiddles; [n_mels] bands
SpecWs carve_spec(Carver& cv, int n_fft, int n_mels) {
  SpecWs w;
  w.tw = reinterpret_cast<cf*>(cv.take((size_t)2 * n_fft));
  w.band = reinterpret_cast<int2*>(cv.take((size_t)2 * n_mels));
  return w;
}

int check_wave(const ttsvits_handle* h, int B, int N, int n_fft, int hop, int win, int T) {
  if (!h || B <= 0 || N <= 0 || hop <= 0 || win <= 0 || T <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (!fft_ok(n_fft) || win > n_fft || B > 65535 || N > (1 << 30) || hop > (1 << 30)) return TTSDEC_ERR_DIMS;
  return TTSDEC_OK;
}

// the caller's workspace carved into w, or refused
int check_ws(void* ws, size_t bytes, int n_fft, int n_mels, SpecWs* w) {
  Carver cv{static_cast<float*>(ws)};
  *w = carve_spec(cv, n_fft, n_mels);
  return (!ws || bytes < cv.bytes() || (reinterpret_cast<uintptr_t>(ws) & 255)) ? TTSDEC_ERR_WORKSPACE : TTSDEC_OK;
}

int run_stft(ttsvits_handle* h, const float* wav, const int32_t* lengths, int B, int N, const float* window, int n_fft, int hop, int win,
             const float* basis, int n_mels, float* out, int T, int32_t* status, const SpecWs& w, hipStream_t st, const char* what) {
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  const int bins = n_fft / 2 + 1;
  if (status) {
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return hip_fail(base(h), e, what);
  }
  launch_stft_tables(w.tw, n_fft, nullptr, nullptr, basis, bins, 1, bins, n_mels, w.band, st);
  StftArgs a;
  a.wav = wav; a.lengths = lengths; a.window = window; a.tw = w.tw; a.basis = basis; a.band = w.band; a.out = out; a.status = status;
  a.Nsamp = N; a.n_fft = n_fft; a.lgM = lg2(n_fft / 2); a.hop = hop; a.win = win; a.n_mels = n_mels; a.T = T;
  a.F = run_frames(n_fft); a.lgF = lg2(a.F); a.scount = run_samples(n_fft, hop);
  const size_t lds = sizeof(float) * run_lds_floats(n_fft, a.scount);
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
  Carver cv{nullptr};
  carve_spec(cv, n_fft, n_mels);
  return cv.bytes();
}

int ttsvits_spectrogram(ttsvits_handle* h, const float* wav, const int32_t* lengths, int B, int N, const float* window, int n_fft, int hop_size,
                        int win_size, float* spec, int T, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_wave(h, B, N, n_fft, hop_size, win_size, T);
  if (rc != TTSDEC_OK) return rc;
  if (!wav || !window || !spec) return TTSDEC_ERR_INVALID_ARG;
  SpecWs w;
  if ((rc = check_ws(workspace, workspace_bytes, n_fft, 0, &w)) != TTSDEC_OK) return rc;
  return run_stft(h, wav, lengths, B, N, window, n_fft, hop_size, win_size, nullptr, 0, spec, T, status, w,
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
  SpecWs w;
  if ((rc = check_ws(workspace, workspace_bytes, n_fft, n_mels, &w)) != TTSDEC_OK) return rc;
  return run_stft(h, wav, lengths, B, N, window, n_fft, hop_size, win_size, mel_basis, n_mels, mel, T, status, w,
                  static_cast<hipStream_t>(stream), "mel_spectrogram");
}

int ttsvits_spec_to_mel(ttsvits_handle* h, const float* spec, const int32_t* frames, int B, int n_fft, int T, const float* mel_basis, int n_mels,
                        float* mel, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || B <= 0 || T <= 0 || n_mels <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (!fft_ok(n_fft) || n_mels > kMaxMels || B > 65535) return TTSDEC_ERR_DIMS;
  if (!spec || !mel_basis || !mel) return TTSDEC_ERR_INVALID_ARG;
  SpecWs w;
  const int rc = check_ws(workspace, workspace_bytes, n_fft, n_mels, &w);
  if (rc != TTSDEC_OK) return rc;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int bins = n_fft / 2 + 1;
  launch_stft_tables(nullptr, 0, nullptr, nullptr, mel_basis, bins, 1, bins, n_mels, w.band, st);
  const int F = bins <= 513 ? kMelFrames : kMelFrames / 2;
  const size_t lds = sizeof(float) * (size_t)bins * (F + 1);
  hipLaunchKernelGGL(mel_kernel, dim3((unsigned)((T + F - 1) / F), (unsigned)B), dim3(kThreads), lds, st, spec, frames, bins, T, F, lg2(F), mel_basis,
                     w.band, n_mels, mel);
  return record_hip_error(base(h), "spec_to_mel");
}

}  // extern "C"
