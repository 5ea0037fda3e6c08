// The per-call tables of the short-time Fourier kernels (stft_run.h launch_stft_tables), one launch: the twiddles
// exp(-2 pi i k / n_fft), k < n_fft, evaluated in fp64 and rounded once (fft_lds.h); per mel filter the run [lo, hi) of bins outside
// which it is exactly zero (a triangular filterbank has ~2 * bins non-zeros in n_mels * bins entries; a dense one just gets [0, bins));
// and 1 / sum w^2, summed in fp64 in a fixed order and rounded once.
#include "stft_run.h"

namespace ttsdec {

// blocks [0, n_fft / 256): the twiddles; one block if inv_wss: 1 / sum w^2; then one block per mel: its band
__global__ __launch_bounds__(kFftThreads) void stft_tables_kernel(cf* __restrict__ tw, int n_fft, const float* __restrict__ window,
                                                                   float* __restrict__ inv_wss, const float* __restrict__ fb, size_t mel_stride,
                                                                   size_t bin_stride, int bins, int2* __restrict__ band) {
  const int nb = n_fft / kFftThreads, tid = threadIdx.x;
  if ((int)blockIdx.x < nb) {
    const int k = blockIdx.x * kFftThreads + tid;
    tw[k] = twiddle(k, n_fft);
    return;
  }
  if (inv_wss && (int)blockIdx.x == nb) {  // every thread its strided terms in order, then a tree: one fixed order
    __shared__ double part[kFftThreads];
    double acc = 0.0;
    for (int i = tid; i < n_fft; i += kFftThreads) acc += (double)window[i] * (double)window[i];
    part[tid] = acc;
    __syncthreads();
    for (int s = kFftThreads / 2; s > 0; s >>= 1) {
      if (tid < s) part[tid] += part[tid + s];
      __syncthreads();
    }
    if (tid == 0) *inv_wss = (float)(1.0 / part[0]);
    return;
  }
  __shared__ int lo, hi;
  const int m = blockIdx.x - nb - (inv_wss ? 1 : 0);
  if (tid == 0) { lo = bins; hi = 0; }
  __syncthreads();
  int l = bins, h = 0;
  for (int k = tid; k < bins; k += kFftThreads)
    if (fb[m * mel_stride + k * bin_stride] != 0.f) { l = l < k ? l : k; h = k + 1; }
  if (h) { atomicMin(&lo, l); atomicMax(&hi, h); }
  __syncthreads();
  if (tid == 0) band[m] = hi > lo ? make_int2(lo, hi) : make_int2(0, 0);
}

void launch_stft_tables(cf* tw, int n_fft, const float* window, float* inv_wss, const float* fb, size_t mel_stride, size_t bin_stride, int bins,
                        int n_mels, int2* band, hipStream_t st) {
  const unsigned blocks = n_fft / kFftThreads + (inv_wss ? 1 : 0) + n_mels;
  hipLaunchKernelGGL(stft_tables_kernel, dim3(blocks), dim3(kFftThreads), 0, st, tw, n_fft, window, inv_wss, fb, mel_stride, bin_stride, bins, band);
}

}  // namespace ttsdec
