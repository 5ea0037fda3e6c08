// The in-LDS complex FFT under every frame run (stft_run.h; spec.hip, griffinlim.hip, analysis.hip): a Stockham autosort of
// radix-8 / radix-4 passes over the F frames of a workgroup's run (M = 128: 8 4 4, 256: 8 8 4, 512: 8 8 8, 1024: 8 8 4 4),
// ping-ponging between two LDS images of F * M complex points.  Complex element i of a frame sits at swz(i): a pass's reads (lanes
// on consecutive i) and the stride-8 writes of the first pass then touch every LDS bank once per lane group; the stride-64 writes
// of the second pass are 2-way.  Workgroups of kFftThreads threads.
#pragma once
#include <hip/hip_runtime.h>

namespace ttsdec {

constexpr int kFftThreads = 256;

inline int lg2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
inline bool fft_ok(int n_fft) { return n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048; }  // the sizes the passes below cover

struct cf { float x, y; };
__device__ inline cf cadd(cf a, cf b) { return {a.x + b.x, a.y + b.y}; }
__device__ inline cf csub(cf a, cf b) { return {a.x - b.x, a.y - b.y}; }
__device__ inline cf cmul(cf a, cf b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ inline cf mul_mi(cf a) { return {a.y, -a.x}; }  // a * -i
__device__ inline int swz(int i) { return i ^ (((i >> 3) ^ (i >> 6)) & 7); }
// exp(-2 pi i k / n_fft), evaluated in fp64 and rounded once
__device__ inline cf twiddle(int k, int n_fft) {
  double s, c;
  sincospi(-2.0 * (double)k / (double)n_fft, &s, &c);
  return {(float)c, (float)s};
}

// natural-order DFTs of 4 and 8 points in registers
__device__ inline void dft4(cf& v0, cf& v1, cf& v2, cf& v3) {
  const cf a = cadd(v0, v2), b = csub(v0, v2), c = cadd(v1, v3), d = mul_mi(csub(v1, v3));
  v0 = cadd(a, c);
  v1 = cadd(b, d);
  v2 = csub(a, c);
  v3 = csub(b, d);
}
template <int R> __device__ inline void dft(cf* v);
template <> __device__ inline void dft<4>(cf* v) { dft4(v[0], v[1], v[2], v[3]); }
template <> __device__ inline void dft<8>(cf* v) {
  constexpr float h = 0.70710678118654752440f;
  cf e0 = cadd(v[0], v[4]), e1 = cadd(v[1], v[5]), e2 = cadd(v[2], v[6]), e3 = cadd(v[3], v[7]);
  cf o0 = csub(v[0], v[4]), o1 = csub(v[1], v[5]), o2 = csub(v[2], v[6]), o3 = csub(v[3], v[7]);
  o1 = {(o1.x + o1.y) * h, (o1.y - o1.x) * h};   // * (1 - i) / sqrt 2
  o2 = mul_mi(o2);
  o3 = {(o3.y - o3.x) * h, -(o3.x + o3.y) * h};  // * (-1 - i) / sqrt 2
  dft4(e0, e1, e2, e3);
  dft4(o0, o1, o2, o3);
  v[0] = e0; v[2] = e1; v[4] = e2; v[6] = e3;
  v[1] = o0; v[3] = o1; v[5] = o2; v[7] = o3;
}

// One Stockham pass of radix R over the F frames of the run: butterfly j of a frame reads elements j + r M / R, multiplies by
// W_M^(r (j mod Ns) M / (Ns R)) = tw[r (j mod Ns) n_fft / (Ns R)], and writes the DFT to (j / Ns) Ns R + j mod Ns + r Ns.
// FIRST: the elements are the window-weighted samples (samp: frame stride fs; win: the n_fft-point window).
template <int R, bool FIRST>
__device__ inline void fft_pass(const cf* __restrict__ src, cf* __restrict__ dst, const cf* __restrict__ tw, const float* __restrict__ samp,
                                const float* __restrict__ win, int fs, int M, int lgM, int Ns, int F) {
  constexpr int lgR = R == 8 ? 3 : 2;
  const int lgPer = lgM - lgR, per = 1 << lgPer;
  const int twq = (2 * M) / (Ns * R);
  for (int w = threadIdx.x; w < (F << lgPer); w += kFftThreads) {
    const int f = w >> lgPer, j = w & (per - 1);
    cf v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = j + (r << lgPer);
      if (FIRST) {
        const float* s = samp + f * fs + 2 * i;
        v[r] = {s[0] * win[2 * i], s[1] * win[2 * i + 1]};
      } else {
        v[r] = src[(f << lgM) + swz(i)];
      }
    }
    const int jl = j & (Ns - 1);
    if (!FIRST) {
      const int q = jl * twq;
#pragma unroll
      for (int r = 1; r < R; ++r) v[r] = cmul(v[r], tw[q * r]);
    }
    dft<R>(v);
    const int o = ((j - jl) << lgR) + jl;
#pragma unroll
    for (int r = 0; r < R; ++r) dst[(f << lgM) + swz(o + r * Ns)] = v[r];
  }
}

// fft_pass<8, true> with the samples and the window read as 8-byte pairs: lanes on consecutive pairs touch every bank once per
// 32-lane group, where the 4-byte reads at stride 2 above are 2-way.  Needs an even frame stride fs.  The same products, the same DFT.
__device__ inline void fft_pass8_first_paired(cf* __restrict__ dst, const float* __restrict__ samp, const float* __restrict__ win, int fs, int M,
                                              int lgM, int F) {
  const float2* s2 = reinterpret_cast<const float2*>(samp);
  const float2* w2 = reinterpret_cast<const float2*>(win);
  const int lgPer = lgM - 3, per = 1 << lgPer, fs2 = fs >> 1;
  for (int w = threadIdx.x; w < (F << lgPer); w += kFftThreads) {
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
    for (int r = 0; r < 8; ++r) dst[(f << lgM) + swz((j << 3) + r)] = v[r];
  }
}

// Every pass after the first radix-8 one, whose result is in a: returns the image that holds the M-point DFTs (element k of frame f
// at (f << lgM) + swz(k)); the other image is free.  Ends behind a barrier.
__device__ inline cf* fft_rest(cf* a, cf* b, const cf* tw, int M, int lgM, int F) {
  if (M == 128) {
    fft_pass<4, false>(a, b, tw, nullptr, nullptr, 0, M, lgM, 8, F);
    __syncthreads();
    fft_pass<4, false>(b, a, tw, nullptr, nullptr, 0, M, lgM, 32, F);
  } else {
    fft_pass<8, false>(a, b, tw, nullptr, nullptr, 0, M, lgM, 8, F);
    __syncthreads();
    if (M == 512) fft_pass<8, false>(b, a, tw, nullptr, nullptr, 0, M, lgM, 64, F);
    else fft_pass<4, false>(b, a, tw, nullptr, nullptr, 0, M, lgM, 64, F);
  }
  __syncthreads();
  if (M != 1024) return a;
  fft_pass<4, false>(a, b, tw, nullptr, nullptr, 0, M, lgM, 256, F);
  __syncthreads();
  return b;
}

}  // namespace ttsdec
