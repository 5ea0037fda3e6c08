// Waveform -> dB spectrogram and dB mel for the Tacotron path (include/ttsdec.h ttsdec_mel_analysis): the reference's
// AudioFrontend.encode (tacotron/data/audio.py:55-67) after its resampling - wave / max |wave|, torchaudio's
// Spectrogram(power=2, normalized=True, center=True), MelScale and amplitude_to_DB(10, 1e-12, 0) - on a padded batch with
// per-utterance sample counts.
//
//   peak_kernel        max |x| of every utterance over its own samples: a grid over (chunks, B) whose workgroups combine with an
//                      integer atomicMax on the bit pattern of |x| (non-negative floats order as their bits), so the result is exact
//                      and does not depend on the order.  The words live in the workspace and are zeroed on the stream.
//   prep_kernel        the per-call tables in the workspace: the twiddles (fft_lds.h); per mel the run [lo, hi) of bins outside which
//                      its filterbank column is exactly zero; and 1 / sum w^2, summed in fp64 in a fixed order and rounded once.
//   analysis_kernel    one workgroup per run of F consecutive frames of one utterance, F * n_fft = kTile (spec.hip's stft_kernel): the
//                      run's (F - 1) hop + n_fft samples are loaded once, reflected by index about the utterance's own ends
//                      (center=True: pad n_fft / 2) and divided by the peak; first radix-8 pass on the window-weighted samples,
//                      fft_rest, the split step, |X|^2 / sum w^2 to LDS as [bin][F + 1].  Two epilogues read that tile:
//                      10 log10(max(D, 1e-12)) -> spec_db [B, T, bins] (skipped for a null pointer), and the mel through each
//                      filter's band -> mel_db [B, T, n_mels].  The power spectrogram never reaches memory.
// Frames at or past an utterance's count are exact zeros.  No sum depends on the batch or on the position of a frame in its run.
#include <math.h>
#include <stdint.h>

#include "fft_lds.h"
#include "kernels.h"

using namespace ttsdec;

namespace {
constexpr int kThreads = kFftThreads;
constexpr int kTile = 4096;        // floats of one LDS image of a run: F frames x n_fft / 2 complex points
constexpr int kMaxMels = 256;
constexpr int kMaxFrames = 1 << 22;
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

// blocks [0, n_fft / 256): the twiddles; block n_fft / 256: 1 / sum w^2; then one block per mel: its band
__global__ __launch_bounds__(kThreads) void prep_kernel(cf* __restrict__ tw, int n_fft, const float* __restrict__ window, float* __restrict__ inv_wss,
                                                        const float* __restrict__ fb, int bins, int n_mels, int2* __restrict__ band) {
  const int nb = n_fft / kThreads, tid = threadIdx.x;
  if ((int)blockIdx.x < nb) {
    const int k = blockIdx.x * kThreads + tid;
    tw[k] = twiddle(k, n_fft);
    return;
  }
  if ((int)blockIdx.x == nb) {  // every thread its strided terms in order, then a tree: one fixed order
    __shared__ double part[kThreads];
    double acc = 0.0;
    for (int i = tid; i < n_fft; i += kThreads) acc += (double)window[i] * (double)window[i];
    part[tid] = acc;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if (tid < s) part[tid] += part[tid + s];
      __syncthreads();
    }
    if (tid == 0) *inv_wss = (float)(1.0 / part[0]);
    return;
  }
  __shared__ int lo, hi;
  const int m = blockIdx.x - nb - 1;
  if (tid == 0) { lo = bins; hi = 0; }
  __syncthreads();
  int l = bins, h = 0;
  for (int k = tid; k < bins; k += kThreads)
    if (fb[(size_t)k * n_mels + m] != 0.f) { l = l < k ? l : k; h = k + 1; }
  if (h) { atomicMin(&lo, l); atomicMax(&hi, h); }
  __syncthreads();
  if (tid == 0) band[m] = hi > lo ? make_int2(lo, hi) : make_int2(0, 0);
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

// grid (ceil(T / F), B); dynamic LDS 3 n_fft + 2 kTile + scount floats
__global__ __launch_bounds__(kThreads) void analysis_kernel(const AnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = a.n_fft, M = N >> 1, bins = M + 1, F = a.F, T = a.T, hop = a.hop, n_mels = a.n_mels;
  cf* tw = reinterpret_cast<cf*>(lds);              // [N]
  float* win = lds + 2 * N;                         // [N]
  cf* bufA = reinterpret_cast<cf*>(lds + 3 * N);    // [F * M]
  cf* bufB = bufA + kTile / 2;                      // [F * M]
  float* samp = lds + 3 * N + 2 * kTile;            // [scount]
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
  // ---- tables and the run's samples ----
  for (int i = tid; i < N; i += kThreads) {
    tw[i] = a.tw[i];
    win[i] = a.window[i];
  }
  const float* wb = a.wav + (size_t)b * a.Nsamp;
  const long long plen = (long long)len + N;  // samples of the padded utterance
  for (int s = tid; s < a.scount; s += kThreads) {
    const long long p = (long long)t0 * hop + s;
    float v = 0.f;
    if (p < plen) {  // (len > M: one reflection reaches every padded sample)
      long long j = p - M;
      if (j < 0) j = -j;
      if (j >= len) j = 2 * ((long long)len - 1) - j;
      v = wb[j] / peak;
    }
    samp[s] = v;
  }
  __syncthreads();
  // ---- complex FFT of M points per frame ----
  const int lgM = a.lgM;
  fft_pass<8, true>(nullptr, bufA, tw, samp, win, hop, M, lgM, 1, F);
  __syncthreads();
  const cf* Z = fft_rest(bufA, bufB, tw, M, lgM, F);
  float* S = reinterpret_cast<float*>(Z == bufA ? bufB : bufA);
  // ---- split step and normalised power: S[k][f], k <= M ----
  const int ss = F + 1;
  const float sc = *a.inv_wss;
  for (int idx = tid; idx < bins * F; idx += kThreads) {
    const int f = idx / bins, k = idx - f * bins;
    const cf zk = Z[(f << lgM) + swz(k & (M - 1))], zm = Z[(f << lgM) + swz((M - k) & (M - 1))];
    const cf xe = {0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)};
    const cf xo = {0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x)};
    const cf x = cadd(xe, cmul(tw[k], xo));
    S[k * ss + f] = (x.x * x.x + x.y * x.y) * sc;
  }
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
    if (t0 + f < tb) {
      const int2 r = a.band[m];
      float acc = 0.f;
      for (int k = r.x; k < r.y; ++k) acc += a.fb[(size_t)k * n_mels + m] * S[k * ss + f];
      val = to_db(acc);
    }
    melb[(size_t)t0 * n_mels + idx] = val;
  }
}

struct WsLayout { cf* tw; int2* band; float* inv_wss; unsigned int* peak; size_t bytes; };
WsLayout ws_layout(void* ws, int B, int n_fft, int n_mels) {
  Carver c{static_cast<float*>(ws)};
  WsLayout l;
  l.tw = reinterpret_cast<cf*>(c.take((size_t)2 * n_fft));
  l.band = reinterpret_cast<int2*>(c.take((size_t)2 * n_mels));
  l.inv_wss = c.take(1);
  l.peak = reinterpret_cast<unsigned int*>(c.take((size_t)B));
  l.bytes = c.bytes();
  return l;
}

bool sizes_ok(int B, int n_fft, int n_mels) { return B <= 65535 && fft_ok(n_fft) && n_mels <= kMaxMels; }

}  // namespace

extern "C" {

size_t ttsdec_mel_analysis_workspace_bytes(const ttsdec_handle* h, int B, int n_fft, int n_mels) {
  if (!h || B <= 0 || n_mels <= 0 || !sizes_ok(B, n_fft, n_mels)) return 0;
  return ws_layout(nullptr, B, n_fft, n_mels).bytes;
}

int ttsdec_mel_analysis(ttsdec_handle* h, const float* wave, const int32_t* lengths, int B, int n_samples, const float* window, const float* fb,
                        int n_mels, int n_fft, int hop_length, int T, float* spec_db, float* mel_db, int32_t* frames_out, int32_t* status,
                        void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || B <= 0 || n_samples <= 0 || n_mels <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (!sizes_ok(B, n_fft, n_mels) || hop_length < 1 || hop_length > n_fft / 2 || T < 1 || T > kMaxFrames || n_samples > (1 << 30))
    return TTSDEC_ERR_DIMS;
  if (!wave || !window || !fb || !mel_db) return TTSDEC_ERR_INVALID_ARG;
  const WsLayout l = ws_layout(workspace, B, n_fft, n_mels);
  if (!workspace || workspace_bytes < l.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255)) return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int bins = n_fft / 2 + 1;
  hipError_t e = hipMemsetAsync(l.peak, 0, (size_t)B * sizeof(unsigned int), st);
  if (e == hipSuccess && status) e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
  if (e != hipSuccess) return hip_fail(base(h), e, "mel_analysis");
  hipLaunchKernelGGL(peak_kernel, dim3((unsigned)((n_samples + kPeakChunk - 1) / kPeakChunk), (unsigned)B), dim3(kThreads), 0, st, wave, lengths,
                     n_samples, l.peak);
  hipLaunchKernelGGL(prep_kernel, dim3((unsigned)(n_fft / kThreads + 1 + n_mels)), dim3(kThreads), 0, st, l.tw, n_fft, window, l.inv_wss, fb, bins,
                     n_mels, l.band);
  AnArgs a;
  a.wav = wave; a.lengths = lengths; a.window = window; a.tw = l.tw; a.inv_wss = l.inv_wss; a.peak = l.peak; a.fb = fb; a.band = l.band;
  a.spec_db = spec_db; a.mel_db = mel_db; a.frames_out = frames_out; a.status = status;
  a.Nsamp = n_samples; a.n_fft = n_fft; a.lgM = lg2(n_fft / 2); a.hop = hop_length; a.n_mels = n_mels; a.T = T;
  a.F = kTile / n_fft; a.scount = (a.F - 1) * hop_length + n_fft;
  const size_t lds = sizeof(float) * ((size_t)3 * n_fft + 2 * kTile + a.scount);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(analysis_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return record_hip_error(base(h), "hipFuncSetAttribute(analysis_kernel)");
  hipLaunchKernelGGL(analysis_kernel, dim3((unsigned)((T + a.F - 1) / a.F), (unsigned)B), dim3(kThreads), lds, st, a);
  return record_hip_error(base(h), "mel_analysis");
}

}  // extern "C"
