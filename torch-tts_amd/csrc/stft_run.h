// The frame run every short-time Fourier kernel works on (spec.hip stft_kernel<MEL>, analysis.hip analysis_kernel, griffinlim.hip
// stft_kernel and istft_kernel): one workgroup of kFftThreads threads takes F = kTile / n_fft consecutive frames of one utterance.
//   RunLds           its dynamic LDS: twiddles, window, two images of F * n_fft / 2 complex points, the run's samples.
//   load_tables      twiddles and window into LDS; a window shorter than n_fft is centred in zeros.
//   load_reflected   the samples the run covers, once, reflected by index about the utterance's own two ends.
//   forward_run      first radix-8 pass on the window-weighted samples, fft_rest (fft_lds.h), and the split step of the real FFT:
//                    n_fft real points as M = n_fft / 2 complex ones z[n] = x[2n] + i x[2n + 1], X[k] = E[k] + W^k O[k] with
//                    E = (Z[k] + conj Z[M - k]) / 2, O = -i (Z[k] - conj Z[M - k]) / 2.  What becomes of X[k] is the caller's emit.
//   band_dot         a mel filter over its band [lo, hi) of bins: the in-order fp32 sum both mel epilogues take.
//   launch_stft_tables  the per-call tables in a workspace (stft_tables.hip): twiddles, bands, 1 / sum w^2.
#pragma once
#include "fft_lds.h"

namespace ttsdec {

constexpr int kTile = 4096;  // floats of one LDS image of a run: F frames x n_fft / 2 complex points
constexpr int kMaxMels = 256;
constexpr int kMaxFrames = 1 << 22;

inline int run_frames(int n_fft) { return kTile / n_fft; }
// samples a run covers: overlapping frames share them; hop > n_fft (spec.hip) loads each frame's n_fft on their own
inline int run_samples(int n_fft, int hop) { return hop <= n_fft ? (run_frames(n_fft) - 1) * hop + n_fft : run_frames(n_fft) * n_fft; }
// floats of RunLds (scount = 0: istft_kernel, which gathers nothing).  This sets the occupancy: 51 KiB at 1024 / 256
constexpr size_t run_lds_floats(int n_fft, int scount) { return (size_t)3 * n_fft + 2 * kTile + scount; }

// A plain aggregate, made by run_lds and passed by value: the compiler then sees in fft_rest (a real call) that tw is the base of the
// dynamic LDS, as it did when every kernel carved these pointers itself, and keeps its twiddle reads 8-byte LDS reads.  Through a
// constructor and a reference it does not (flat address arithmetic and 4-byte read pairs instead).
struct RunLds {
  cf* tw;       // [n_fft]
  float* win;   // [n_fft]
  cf *bufA, *bufB;  // [F * n_fft / 2] each
  float* samp;  // [scount]
};
__device__ inline RunLds run_lds(float* lds, int N) {  // lds: the kernel's dynamic LDS, run_lds_floats long
  cf* a = reinterpret_cast<cf*>(lds + 3 * N);
  return {reinterpret_cast<cf*>(lds), lds + 2 * N, a, a + kTile / 2, lds + 3 * N + 2 * kTile};
}

// window [wlen] lands at (N - wlen) / 2 of win [N]; wlen = N is a plain copy.  No barrier.
__device__ inline void load_tables(const RunLds l, int N, const cf* __restrict__ tw, const float* __restrict__ window, int wlen) {
  for (int i = threadIdx.x; i < N; i += kFftThreads) {
    l.tw[i] = tw[i];
    const int wl = (N - wlen) / 2, j = i - wl;
    l.win[i] = (j >= 0 && j < wlen) ? window[j] : 0.f;
  }
}

// samp[s], s < scount: sample p - pad of the utterance wb [len] padded by `pad` at both ends (one reflection reaches every padded
// sample; past the padded end: 0), p = t0 * hop + s for overlapping frames, else frame t0 + s / N's sample s % N; through fn.
template <typename Fn>
__device__ inline void load_reflected(float* samp, int scount, const float* __restrict__ wb, int len, int pad, int t0, int hop, int N, bool overlap,
                                      Fn fn) {
  const long long plen = (long long)len + 2 * pad;  // samples of the padded utterance
  for (int s = threadIdx.x; s < scount; s += kFftThreads) {
    long long p;
    if (overlap) p = (long long)t0 * hop + s;
    else p = (long long)(t0 + s / N) * hop + s % N;
    float v = 0.f;
    if (p < plen) {
      long long j = p - pad;
      if (j < 0) j = -j;
      if (j >= len) j = 2 * ((long long)len - 1) - j;
      v = fn(wb[j]);
    }
    samp[s] = v;
  }
}

// The run in l.samp (frame stride fs; behind a barrier) -> emit(f, k, X[k], S) for every frame f < F and bin k <= M.  `paired`: the
// first pass of fft_lds.h that reads pairs (even fs).  S, also returned, is the image the spectra are NOT in: an emit may fill it.
template <typename Emit>
__device__ inline float* forward_run(const RunLds l, int fs, bool paired, int M, int lgM, int F, Emit emit) {
  if (paired) fft_pass8_first_paired(l.bufA, l.samp, l.win, fs, M, lgM, F);
  else fft_pass<8, true>(nullptr, l.bufA, l.tw, l.samp, l.win, fs, M, lgM, 1, F);
  __syncthreads();
  const cf* Z = fft_rest(l.bufA, l.bufB, l.tw, M, lgM, F);
  float* S = reinterpret_cast<float*>(Z == l.bufA ? l.bufB : l.bufA);
  const int bins = M + 1;
  for (int idx = threadIdx.x; idx < bins * F; idx += kFftThreads) {
    const int f = idx / bins, k = idx - f * bins;
    const cf zk = Z[(f << lgM) + swz(k & (M - 1))], zm = Z[(f << lgM) + swz((M - k) & (M - 1))];
    const cf xe = {0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)};
    const cf xo = {0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x)};
    emit(f, k, cadd(xe, cmul(l.tw[k], xo)), S);
  }
  return S;
}

// sum over k in [r.x, r.y) of fb[k * stride] * S[k * ss + f], in bin order
__device__ inline float band_dot(const float* __restrict__ fb, size_t stride, int2 r, const float* __restrict__ S, int ss, int f) {
  float acc = 0.f;
  for (int k = r.x; k < r.y; ++k) acc += fb[(size_t)k * stride] * S[k * ss + f];
  return acc;
}

// On st: tw [n_fft] = exp(-2 pi i k / n_fft) (n_fft = 0: none); band[m], m < n_mels = the run [lo, hi) of bins outside which filter m
// is exactly zero, filter m's bin k at fb[m * mel_stride + k * bin_stride]; *inv_wss = 1 / sum window[i]^2, i < n_fft (nullptr: none)
void launch_stft_tables(cf* tw, int n_fft, const float* window, float* inv_wss, const float* fb, size_t mel_stride, size_t bin_stride, int bins,
                        int n_mels, int2* band, hipStream_t st);

}  // namespace ttsdec
