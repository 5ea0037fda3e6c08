// Waveform -> dB spectrogram and dB mel for the Tacotron path (include/ttsdec.h ttsdec_mel_analysis): the reference's
// AudioFrontend.encode (tacotron/data/audio.py:55-67) after its resampling - wave / max |wave|, torchaudio's
// Spectrogram(power=2, normalized=True, center=True), MelScale and amplitude_to_DB(10, 1e-12, 0) - on a padded batch with
// per-utterance sample counts.
//
//   peak_kernel        max |x| of every utterance over its own samples: a grid over (chunks, B) whose workgroups combine with an
//                      integer atomicMax on the bit pattern of |x| (non-negative floats order as their bits), so the result is exact
//                      and does not depend on the order.  The words live in the workspace and are zeroed on the stream.
//   (tables)           twiddles, per mel the band of its filterbank column's non-zero bins, and 1 / sum w^2, in the workspace:
//                      stft_run.h launch_stft_tables.
//   analysis_kernel    one workgroup per run of F consecutive frames of one utterance, F * n_fft = kTile: the frame run of stft_run.h
//                      - the run's (F - 1) hop + n_fft samples loaded once, reflected by index about the utterance's own ends
//                      (center=True: pad n_fft / 2) and divided by the peak, forward_run - with |X|^2 / sum w^2 to LDS as
//                      [bin][F + 1] as its emit.  Two epilogues read that tile:
//                      10 log10(max(D, 1e-12)) -> spec_db [B, T, bins] (skipped for a null pointer), and the mel through each
//                      filter's band -> mel_db [B, T, n_mels].  The power spectrogram never reaches memory.
// Frames at or past an utterance's count are exact zeros.  No sum depends on the batch or on the position of a frame in its run.
#include <math.h>
#include <stdint.h>

#include "kernels.h"
#include "stft_run.h"

using namespace ttsdec;

namespace {
constexpr int kThreads = kFftThreads;
constexpr int kPeakChunk = 8192;   // samples per workgroup of peak_kernel
// status word: len <= n_fft / 2 (the reflection is undefined); a peak of 0; a length beyond the row / frames beyond T
enum { FLAG_REFLECT = 1, FLAG_ZERO = 2, FLAG_RANGE = 4 };

inline HandleBase* base(ttsdec_handle* h) { return reinterpret_cast<HandleBase*>(h); }

// grid (ceil(Nsamp / kPeakChunk), B)
__global__ __launch_bounds__(kThreads) void peak_kernel(const float* __restrict__ wav, const int* __restrict__ lengths, int Nsamp,
                                                        unsigned int* __restrict__ peak) {
  __shared__ unsigned int red;
  const int b = blockIdx.y, s0 = blockIdx.x * kPeakChunk;
  int len = lengths ? lengths[b] : Nsamp;
  len = len < Nsamp ? len : Nsamp;
  if (s0 >= len) return;  // (workgroup-uniform)
  if (threadIdx.x == 0) red = 0u;
  __syncthreads();
  const int s1 = s0 + kPeakChunk < len ? s0 + kPeakChunk : len;
  const float* wb = wav + (size_t)b * Nsamp;
  unsigned int m = 0u;
  for (int s = s0 + threadIdx.x; s < s1; s += kThreads) {
    const unsigned int v = __float_as_uint(fabsf(wb[s]));
    m = m > v ? m : v;
  }
  atomicMax(&red, m);
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(peak + b, red);
}

struct AnArgs {
  const float* wav;          // [B, Nsamp]
  const int* lengths;        // [B] or nullptr
  const float* window;       // [n_fft]
  const cf* tw;              // [n_fft]
  const float* inv_wss;      // [1]
  const unsigned int* peak;  // [B] bits of max |x|
  const float* fb;           // [bins, n_mels]
  const int2* band;          // [n_mels]
  float* spec_db;            // [B, T, bins] or nullptr
  float* mel_db;             // [B, T, n_mels]
  int* frames_out;           // [B] or nullptr
  int* status;               // or nullptr
  int Nsamp, n_fft, lgM, hop, n_mels, T, F, scount;
};

__device__ inline float to_db(float v) { return 10.f * log10f(fmaxf(v, 1e-12f)); }  // amplitude_to_DB(10, 1e-12, 0)

// grid (ceil(T / F), B); dynamic LDS run_lds_floats(n_fft, scount)
__global__ __launch_bounds__(kThreads) void analysis_kernel(const AnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = a.n_fft, M = N >> 1, bins = M + 1, F = a.F, T = a.T, hop = a.hop, n_mels = a.n_mels;
  const RunLds l = run_lds(lds, N);
  const int b = blockIdx.y, t0 = blockIdx.x * F, tid = threadIdx.x;
  // ---- the utterance: its samples, its frames, its flags ----
  int len = a.lengths ? a.lengths[b] : a.Nsamp, flags = 0;
  if (len > a.Nsamp) { flags |= FLAG_RANGE; len = a.Nsamp; }
  const float peak = __uint_as_float(a.peak[b]);
  int tb = 0;
  if (len <= M) flags |= FLAG_REFLECT;
  else if (peak == 0.f) flags |= FLAG_ZERO;
  else tb = 1 + len / hop;
  if (tb > T) { flags |= FLAG_RANGE; tb = T; }
  if (blockIdx.x == 0 && tid == 0) {
    if (flags && a.status) atomicOr(a.status, flags);
    if (a.frames_out) a.frames_out[b] = tb;
  }
  float* specb = a.spec_db ? a.spec_db + (size_t)b * T * bins : nullptr;
  float* melb = a.mel_db + (size_t)b * T * n_mels;
  const int nf = T - t0 < F ? T - t0 : F;  // frames of the run inside the tensors
  if (t0 >= tb) {  // (workgroup-uniform) nothing of this run is a frame of the utterance
    if (specb)
      for (int idx = tid; idx < nf * bins; idx += kThreads) specb[(size_t)t0 * bins + idx] = 0.f;
    for (int idx = tid; idx < nf * n_mels; idx += kThreads) melb[(size_t)t0 * n_mels + idx] = 0.f;
    return;
  }
  // ---- tables and the run's samples (len > M: one reflection reaches every padded sample) ----
  load_tables(l, N, a.tw, a.window, N);
  load_reflected(l.samp, a.scount, a.wav + (size_t)b * a.Nsamp, len, M, t0, hop, N, true, [peak](float v) { return v / peak; });
  __syncthreads();
  // ---- transform, split step and normalised power: S[k][f], k <= M ----
  const int ss = F + 1;
  const float sc = *a.inv_wss;
  const float* S = forward_run(l, hop, false, M, a.lgM, F,
                               [ss, sc](int f, int k, cf x, float* S) { S[k * ss + f] = (x.x * x.x + x.y * x.y) * sc; });
  __syncthreads();
  // ---- dB spectrogram: a frame's bins are contiguous ----
  if (specb) {
    for (int idx = tid; idx < nf * bins; idx += kThreads) {
      const int f = idx / bins, k = idx - f * bins;
      specb[(size_t)t0 * bins + idx] = t0 + f < tb ? to_db(S[k * ss + f]) : 0.f;
    }
  }
  // ---- dB mel: fp32 sums over each filter's band, in bin order (lanes on consecutive mels: the filterbank rows are read whole) ----
  for (int idx = tid; idx < nf * n_mels; idx += kThreads) {
    const int f = idx / n_mels, m = idx - f * n_mels;
    float val = 0.f;
    if (t0 + f < tb) val = to_db(band_dot(a.fb + m, n_mels, a.band[m], S, ss, f));
    melb[(size_t)t0 * n_mels + idx] = val;
  }
}

struct AnWs { cf* tw; int2* band; float* inv_wss; unsigned int* peak; };  // [n_fft]; [n_mels]; [1]; [B] bits of max |x|
AnWs carve_analysis(Carver& cv, int B, int n_fft, int n_mels) {
  AnWs w;
  w.tw = reinterpret_cast<cf*>(cv.take((size_t)2 * n_fft));
  w.band = reinterpret_cast<int2*>(cv.take((size_t)2 * n_mels));
  w.inv_wss = cv.take(1);
  w.peak = reinterpret_cast<unsigned int*>(cv.take((size_t)B));
  return w;
}

bool sizes_ok(int B, int n_fft, int n_mels) { return B <= 65535 && fft_ok(n_fft) && n_mels <= kMaxMels; }

}  // namespace

extern "C" {

size_t ttsdec_mel_analysis_workspace_bytes(const ttsdec_handle* h, int B, int n_fft, int n_mels) {
  if (!h || B <= 0 || n_mels <= 0 || !sizes_ok(B, n_fft, n_mels)) return 0;
  Carver cv{nullptr};
  carve_analysis(cv, B, n_fft, n_mels);
  return cv.bytes();
}

int ttsdec_mel_analysis(ttsdec_handle* h, const float* wave, const int32_t* lengths, int B, int n_samples, const float* window, const float* fb,
                        int n_mels, int n_fft, int hop_length, int T, float* spec_db, float* mel_db, int32_t* frames_out, int32_t* status,
                        void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || B <= 0 || n_samples <= 0 || n_mels <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (!sizes_ok(B, n_fft, n_mels) || hop_length < 1 || hop_length > n_fft / 2 || T < 1 || T > kMaxFrames || n_samples > (1 << 30))
    return TTSDEC_ERR_DIMS;
  if (!wave || !window || !fb || !mel_db) return TTSDEC_ERR_INVALID_ARG;
  Carver cv{static_cast<float*>(workspace)};
  const AnWs l = carve_analysis(cv, B, n_fft, n_mels);
  if (!workspace || workspace_bytes < cv.bytes() || (reinterpret_cast<uintptr_t>(workspace) & 255)) return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int bins = n_fft / 2 + 1;
  hipError_t e = hipMemsetAsync(l.peak, 0, (size_t)B * sizeof(unsigned int), st);
  if (e == hipSuccess && status) e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
  if (e != hipSuccess) return hip_fail(base(h), e, "mel_analysis");
  hipLaunchKernelGGL(peak_kernel, dim3((unsigned)((n_samples + kPeakChunk - 1) / kPeakChunk), (unsigned)B), dim3(kThreads), 0, st, wave, lengths,
                     n_samples, l.peak);
  launch_stft_tables(l.tw, n_fft, window, l.inv_wss, fb, 1, n_mels, bins, n_mels, l.band, st);
  AnArgs a;
  a.wav = wave; a.lengths = lengths; a.window = window; a.tw = l.tw; a.inv_wss = l.inv_wss; a.peak = l.peak; a.fb = fb; a.band = l.band;
  a.spec_db = spec_db; a.mel_db = mel_db; a.frames_out = frames_out; a.status = status;
  a.Nsamp = n_samples; a.n_fft = n_fft; a.lgM = lg2(n_fft / 2); a.hop = hop_length; a.n_mels = n_mels; a.T = T;
  a.F = run_frames(n_fft); a.scount = run_samples(n_fft, hop_length);
  const size_t lds = sizeof(float) * run_lds_floats(n_fft, a.scount);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(analysis_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return record_hip_error(base(h), "hipFuncSetAttribute(analysis_kernel)");
  hipLaunchKernelGGL(analysis_kernel, dim3((unsigned)((T + a.F - 1) / a.F), (unsigned)B), dim3(kThreads), lds, st, a);
  return record_hip_error(base(h), "mel_analysis");
}

}  // extern "C"
