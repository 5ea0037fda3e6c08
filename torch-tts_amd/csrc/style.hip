// C ABI of the style encoder (tacotron/modules/style.py, modules/attention.py:129-186): ReferenceEncoder and what VAE / GST /
// GST_VAE put behind it, eval mode, exact fp32.  A second handle of the ttsenc_ family (include/ttsdec.h ttsenc_style_*):
//   stage 0 (Cin = 1): direct 3x3 stride-2 conv + bias + BN + ReLU, 4 channels per thread
//   -> stages 1 .. K-1: implicit-GEMM convs on gemm_tile.h with a stride-2 2-D address generator of their own
//   -> one GEMM for the LSTM's input projection over all T' steps (the last conv's channels-last output is its A operand as it lies)
//   -> T' sequential steps of the LSTM kernel in packed-sequence mode (a row stops at its own clipped step count)
//   -> one tail kernel, a workgroup per utterance: the small linears, z, kl, fc_out, the token attention.
// Activations are channels-last, [B, T_l, F_l, C_l]; sizes L -> (L - 1) / 2 + 1 per stage on both axes.
#include <string.h>

#include <new>

#include "step_bodies.h"

using namespace ttsdec;

namespace {
constexpr int kMaxConvs = TTSENC_STYLE_MAX_CONVS;
constexpr int kMaxFeat = 1024;   // d_enc, d_emb: the tail kernel's LDS rows
constexpr int kMaxVae = 256;
constexpr int kMaxTokens = 64;
constexpr int kMaxHeads = 16;
constexpr int kTailThreads = 256;

struct StyleBlob {  // offsets in floats
  size_t conv_w[kMaxConvs], bias[kMaxConvs], alpha[kMaxConvs], beta[kMaxConvs];
  size_t w_ih, w_hh, bsum, mean_w, mean_b, logvar_w, logvar_b, fc_out, wq, kproj, vproj, total;
};
struct StyleWs {
  float *act[2], *gx, *h, *c;
  int* steps;
  size_t total;  // bytes, or 0: refused (layout.h within_dma_reach)
};
struct StageDims {  // per conv stage: output sizes
  int T[kMaxConvs], F[kMaxConvs];
};
inline int half_up(int L) { return (L - 1) / 2 + 1; }
}  // namespace

struct ttsenc_style_handle : HandleBase {
  ttsenc_style_dims d;
  StyleBlob bl;
  int f_last;  // frequency bins after the last stage
};

namespace {
bool has_vae(int kind) { return kind == TTSENC_STYLE_VAE || kind == TTSENC_STYLE_GST_VAE; }
bool has_gst(int kind) { return kind == TTSENC_STYLE_GST || kind == TTSENC_STYLE_GST_VAE; }

StageDims stage_dims(const ttsenc_style_dims& d, int T) {
  StageDims s;
  int t = T, f = d.n_mels;
  for (int i = 0; i < d.n_convs; ++i) {
    t = half_up(t);
    f = half_up(f);
    s.T[i] = t;
    s.F[i] = f;
  }
  return s;
}

StyleBlob make_layout(const ttsenc_style_dims& d, int f_last) {
  StyleBlob L;
  memset(&L, 0, sizeof(L));
  Carver cv{nullptr};
  for (int i = 0; i < d.n_convs; ++i) {
    const size_t ci = i == 0 ? 1 : d.filters[i - 1], co = d.filters[i];
    L.conv_w[i] = cv.take_off(co * 9 * ci);  // stage 0: [tap][C_0]; later stages: [C_out][ky][kx][C_in]
    L.bias[i] = cv.take_off(co);
    L.alpha[i] = cv.take_off(co);
    L.beta[i] = cv.take_off(co);
  }
  const size_t H = d.d_enc, feat = (size_t)d.filters[d.n_convs - 1] * f_last;
  L.w_ih = cv.take_off(4 * H * feat);  // columns in channels-last order f * C + c
  L.w_hh = cv.take_off(4 * H * H);
  L.bsum = cv.take_off(4 * H);
  if (has_vae(d.kind)) {
    const size_t din = d.kind == TTSENC_STYLE_VAE ? d.d_enc : d.d_emb;
    L.mean_w = cv.take_off(d.d_vae * din);
    L.mean_b = cv.take_off(d.d_vae);
    L.logvar_w = cv.take_off(d.d_vae * din);
    L.logvar_b = cv.take_off(d.d_vae);
    L.fc_out = cv.take_off((size_t)d.d_emb * d.d_vae);
  }
  if (has_gst(d.kind)) {
    L.wq = cv.take_off((size_t)d.d_emb * d.d_enc);
    L.kproj = cv.take_off((size_t)d.n_tokens * d.d_emb);  // tanh(embed) . W_key^T
    L.vproj = cv.take_off((size_t)d.n_tokens * d.d_emb);  // tanh(embed) . W_value^T
  }
  L.total = cv.off;
  return L;
}

StyleWs carve(const ttsenc_style_dims& d, int B, int T, float* base) {
  StyleWs W;
  Carver cv{base};
  const StageDims s = stage_dims(d, T);
  size_t n[2] = {0, 0};  // stage i writes act[i & 1]
  for (int i = 0; i < d.n_convs; ++i) {
    const size_t e = (size_t)B * s.T[i] * s.F[i] * d.filters[i];
    if (e > n[i & 1]) n[i & 1] = e;
  }
  W.act[0] = cv.take(n[0]);
  W.act[1] = cv.take(n[1] ? n[1] : 1);
  const int Tp = s.T[d.n_convs - 1];
  W.gx = cv.take((size_t)B * Tp * 4 * d.d_enc);
  W.h = cv.take((size_t)B * d.d_enc);
  W.c = cv.take((size_t)B * d.d_enc);
  W.steps = reinterpret_cast<int*>(cv.take(B));
  W.total = within_dma_reach(cv.bytes());
  return W;
}

// ===========================================================================
// kernels
// ===========================================================================
// a row's LSTM step count: clip(trunc(len / 2^K), min = 1) (style.py:63-64), never beyond the T' steps there are
__global__ void style_steps_kernel(const int32_t* lengths, int* steps, int B, int n_convs, int Tp) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int s = Tp;
  if (lengths != nullptr) {
    const int len = lengths[b];
    s = len > 0 ? len >> n_convs : 0;
    s = s < 1 ? 1 : s;
    s = s > Tp ? Tp : s;
  }
  steps[b] = s;
}

// stage 0: out[b, t, f, c] = relu(bn(bias[c] + sum_{ky, kx} x[b, 2t + ky - 1, 2f + kx - 1] * w[ky*3 + kx][c])).
// A thread owns 4 channels (one 16-byte store) and keeps their 36 taps and 12 epilogue values in registers while it walks
// positions; the C0 / 4 threads of a position read the same 9 inputs.
struct Conv0Args {
  const float* x;
  int ldx;
  const float *w, *bias, *alpha, *beta;  // w [9][C0]
  float* out;
  int T, F, To, Fo, C0;
  long n_pos;  // B * To * Fo
};
__global__ __launch_bounds__(256) void style_conv0_kernel(Conv0Args g) {
  const int C4 = g.C0 >> 2;
  const int ppb = 256 / C4;  // positions per workgroup and pass
  const int c4 = threadIdx.x % C4, pin = threadIdx.x / C4;
  if (pin >= ppb) return;
  f32x4 w[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = *reinterpret_cast<const f32x4*>(g.w + (size_t)k * g.C0 + c4 * 4);
  const f32x4 bias = *reinterpret_cast<const f32x4*>(g.bias + c4 * 4);
  const f32x4 alpha = *reinterpret_cast<const f32x4*>(g.alpha + c4 * 4);
  const f32x4 beta = *reinterpret_cast<const f32x4*>(g.beta + c4 * 4);
  for (long pos = (long)blockIdx.x * ppb + pin; pos < g.n_pos; pos += (long)gridDim.x * ppb) {
    const int f = (int)(pos % g.Fo);
    const long bt = pos / g.Fo;
    const int t = (int)(bt % g.To);
    const long b = bt / g.To;
    float in[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int ty = 2 * t + ky - 1;
      const bool tok = ty >= 0 && ty < g.T;
      const float* row = g.x + ((size_t)b * g.T + (tok ? ty : 0)) * g.ldx;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int fx = 2 * f + kx - 1;
        const bool ok = tok && fx >= 0 && fx < g.F;
        in[ky * 3 + kx] = ok ? row[ok ? fx : 0] : 0.f;
      }
    }
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 9; ++k) acc = fmaf(in[k], w[k][j], acc);  // taps in order: the k-order of an output is fixed
      acc = add_rn(acc, bias[j]);
      acc = add_rn(mul_rn(acc, alpha[j]), beta[j]);
      v[j] = acc > 0.f ? acc : 0.f;
    }
    *reinterpret_cast<f32x4*>(g.out + (size_t)pos * g.C0 + c4 * 4) = v;
  }
}

// Stages 1 .. K-1 as an implicit GEMM: M = B * To * Fo rows, N = Co, K = 9 * Ci with k = (ky*3 + kx) * Ci + c.  In channels-last
// storage the three kx taps of one ky are ONE contiguous run of 3 * Ci floats starting at act[b, 2t + ky - 1, 2f - 1, 0], so the
// K axis is gemm_tile's three K segments (one per ky).  Out of the picture: a whole segment when its frame 2t + ky - 1 is (the
// lane's offset is beyond the descriptor's range: the DMA writes zeros), the first Ci of every segment when f = 0, the last Ci
// when 2f + 1 = Fi (the per-row k window, the same for the three segments).  Ci % 4 == 0 keeps every 16-byte column in one tap.
struct LoaderConv2d {
  const void* x;
  int m0, M, Ti, Fi, Ci, To, Fo;
  static constexpr bool kRange = true;
  __device__ __forceinline__ int nseg() const { return 3; }
  __device__ __forceinline__ int seglen(int) const { return 3 * Ci; }
  __device__ __forceinline__ bool row_ok(int r) const { return m0 + r < M; }
  // element index of k = 0 of segment ky in row m (may lie in front of x: only lanes inside the picture are dereferenced)
  __device__ __forceinline__ long elem(int m, int ky) const {
    const int f = m % Fo, bt = m / Fo;
    const int t = bt % To, b = bt / To;
    return (((long)b * Ti + 2 * t + ky - 1) * Fi + 2 * f - 1) * Ci;
  }
  __device__ __forceinline__ gbyte* row_ptr(int r, int ky, int) const { return as_global(x) + elem(m0 + r, ky) * 4; }
  __device__ __forceinline__ int k_lo(int r) const { return (m0 + r) % Fo == 0 ? Ci : 0; }
  __device__ __forceinline__ int k_hi(int r) const { return 2 * ((m0 + r) % Fo) + 1 < Fi ? 3 * Ci : 2 * Ci; }
  __device__ __forceinline__ long col_off(int c16) const { return (long)c16 * 16; }
  __device__ __forceinline__ long tile_inc(int rowb) const { return rowb; }
  // buffer-descriptor form: based at the segment start of THIS workgroup's first row; rows ascend in memory with m (a step of t
  // is 2 * Fi * Ci floats, the f of a row spans less), so every offset is non-negative and a tile's rows stay within a few MB
  __device__ __forceinline__ const void* seg_base(int ky, int) const { return static_cast<const char*>(x) + elem(m0, ky) * 4; }
  __device__ __forceinline__ unsigned row_off(int r, int ky) const {
    const int m = m0 + r;
    const int ty = 2 * ((m / Fo) % To) + ky - 1;
    if (ty < 0 || ty >= Ti) return kBufRange;
    return (unsigned)((elem(m, ky) - elem(m0, ky)) * 4);
  }
};

// rows n0.. of the repacked conv weight [Co][3 segments of 3 * Ci]
struct LoaderConvW {
  const float* w;
  int n0, N, Ci;
  static constexpr bool kRange = false;
  __device__ __forceinline__ int nseg() const { return 3; }
  __device__ __forceinline__ int seglen(int) const { return 3 * Ci; }
  __device__ __forceinline__ bool row_ok(int r) const { return n0 + r < N; }
  __device__ __forceinline__ gbyte* row_ptr(int r, int s, int) const { return as_global(w) + ((long)(n0 + r) * 9 + 3 * s) * Ci * 4; }
  __device__ __forceinline__ long col_off(int c16) const { return (long)c16 * 16; }
  __device__ __forceinline__ long tile_inc(int rowb) const { return rowb; }
  __device__ __forceinline__ const void* seg_base(int s, int) const { return w + ((size_t)n0 * 9 + 3 * s) * Ci; }
  __device__ __forceinline__ unsigned row_off(int r, int) const { return (unsigned)r * 9u * (unsigned)Ci * 4u; }
};

struct ConvArgs {
  const float* in;  // [B, Ti, Fi, Ci]
  const float *w, *bias, *alpha, *beta;
  float* out;  // [M, Co]
  int M, Ti, Fi, Ci, To, Fo, Co;
};
template <class Cfg>
__global__ __launch_bounds__(kGemmThreads, Cfg::kWavesPerSimd) void style_conv_kernel(ConvArgs g) {
  __shared__ __attribute__((aligned(16))) float smem[Cfg::kLdsFloats];
  constexpr int BM = Cfg::BM, BN = Cfg::BN, LDO = Cfg::LDO;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const LoaderConv2d la{g.in, m0, g.M, g.Ti, g.Fi, g.Ci, g.To, g.Fo};
  const LoaderConvW lb{g.w, n0, g.Co, g.Ci};
  gemm_tile<Cfg, LoaderConv2d, LoaderConvW, NoGate, DmaDesc::PerSegment>(la, lb, smem);
  // style.py:54-56: relu(bn(conv + bias)), BN in eval mode as v * alpha + beta; four columns per thread, one 16-byte store
  constexpr int Q = BN / 4;
  for (int e = threadIdx.x; e < BM * Q; e += kGemmThreads) {
    const int row = e / Q, col = (e % Q) * 4;
    const int m = m0 + row, n = n0 + col;
    if (m >= g.M || n >= g.Co) continue;  // (Co % 4 == 0: a group of four is inside or outside as a whole)
    const f32x4 bias = *reinterpret_cast<const f32x4*>(g.bias + n);
    const f32x4 alpha = *reinterpret_cast<const f32x4*>(g.alpha + n);
    const f32x4 beta = *reinterpret_cast<const f32x4*>(g.beta + n);
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = add_rn(smem[row * LDO + col + j], bias[j]);
      a = add_rn(mul_rn(a, alpha[j]), beta[j]);
      v[j] = a > 0.f ? a : 0.f;
    }
    *reinterpret_cast<f32x4*>(g.out + (size_t)m * g.Co + n) = v;
  }
}

// The tile comes from the stage's channel counts alone, never from M: an output's k-order then does not depend on the batch or on
// T, so an utterance gives the same bits alone and inside a batch.  Ci >= 64 (K >= 576; the stages whose M is a few thousand rows
// at the most): 32 x 32 tiles with the four MFMA waves splitting K.  Ci < 64: the K-sequential tiles, 128 x 32 for Co <= 32
// (64 x 64 would leave half its columns empty), 64 x 64 above.
template <class Cfg>
void launch_conv_cfg(const ConvArgs& a, hipStream_t st) {
  dim3 grid((a.Co + Cfg::BN - 1) / Cfg::BN, (a.M + Cfg::BM - 1) / Cfg::BM);
  hipLaunchKernelGGL((style_conv_kernel<Cfg>), grid, dim3(kGemmThreads), 0, st, a);
}
void launch_conv(const ConvArgs& a, hipStream_t st) {
  if (a.Ci >= 64) launch_conv_cfg<TileCfg<1, 1, 4, 4>>(a, st);
  else if (a.Co <= 32) launch_conv_cfg<TileCfg<4, 1, 1, 4>>(a, st);
  else launch_conv_cfg<TileCfg<2, 2, 1, 4>>(a, st);
}

// out[n] = b[n] + sum_k W[n][k] * in[k], k ascending (one thread per output: a fixed order)
__device__ __forceinline__ float dot_row(const float* W, const float* in, int K) {
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(W[k], in[k], acc);
  return acc;
}

// Everything behind enc_out, one workgroup per utterance (style.py:96-109, 134-151, 166-177; attention.py:152-186).
struct TailArgs {
  const float* enc;  // [B, d_enc]
  const float* eps;  // [B, d_vae]
  const float *mean_w, *mean_b, *logvar_w, *logvar_b, *fc_out, *wq, *kproj, *vproj;
  float *x_out, *kl_out;
  int kind, d_enc, d_emb, d_vae, n_tokens, n_heads;
};
__global__ __launch_bounds__(kTailThreads) void style_tail_kernel(TailArgs g) {
  __shared__ float s_in[kMaxFeat], s_q[kMaxFeat], s_style[kMaxFeat], s_z[kMaxVae], s_p[kMaxHeads * kMaxTokens];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < g.d_enc; i += kTailThreads) s_in[i] = g.enc[(size_t)b * g.d_enc + i];
  __syncthreads();
  const float* vin = s_in;  // what mean_linear / logvar_linear read
  int din = g.d_enc;
  if (g.kind == TTSENC_STYLE_GST || g.kind == TTSENC_STYLE_GST_VAE) {
    const int dk = g.d_emb / g.n_heads;
    for (int n = tid; n < g.d_emb; n += kTailThreads) s_q[n] = dot_row(g.wq + (size_t)n * g.d_enc, s_in, g.d_enc);
    __syncthreads();
    // scores[h][t] = d_gain * q_h . k_h[t], d_gain = 1 / sqrt(key_dim) with key_dim = d_emb / n_heads (style.py:89)
    const float gain = div_rn(1.0f, sqrt_rn((float)dk));
    for (int e = tid; e < g.n_heads * g.n_tokens; e += kTailThreads) {
      const int hd = e / g.n_tokens, t = e % g.n_tokens;
      s_p[hd * kMaxTokens + t] = mul_rn(gain, dot_row(g.kproj + (size_t)t * g.d_emb + hd * dk, s_q + hd * dk, dk));
    }
    __syncthreads();
    if (tid < g.n_heads) {  // softmax over the tokens of head tid
      float* p = s_p + tid * kMaxTokens;
      float mx = p[0];
      for (int t = 1; t < g.n_tokens; ++t) mx = fmaxf(mx, p[t]);
      float sum = 0.f;
      for (int t = 0; t < g.n_tokens; ++t) {
        p[t] = expf(sub_rn(p[t], mx));
        sum = add_rn(sum, p[t]);
      }
      for (int t = 0; t < g.n_tokens; ++t) p[t] = div_rn(p[t], sum);
    }
    __syncthreads();
    for (int n = tid; n < g.d_emb; n += kTailThreads) {  // heads concatenated: column n belongs to head n / dk
      const float* p = s_p + (n / dk) * kMaxTokens;
      float acc = 0.f;
      for (int t = 0; t < g.n_tokens; ++t) acc = fmaf(p[t], g.vproj[(size_t)t * g.d_emb + n], acc);
      s_style[n] = acc;
      if (g.kind == TTSENC_STYLE_GST) g.x_out[(size_t)b * g.d_emb + n] = acc;
    }
    __syncthreads();
    vin = s_style;
    din = g.d_emb;
  }
  if (g.kind == TTSENC_STYLE_VAE || g.kind == TTSENC_STYLE_GST_VAE) {
    for (int n = tid; n < g.d_vae; n += kTailThreads) {
      const float mean = add_rn(dot_row(g.mean_w + (size_t)n * din, vin, din), g.mean_b[n]);
      const float logvar = add_rn(dot_row(g.logvar_w + (size_t)n * din, vin, din), g.logvar_b[n]);
      // z = eps * exp(0.5 * logvar) + mean;  kl = -(1 + logvar - mean^2 - exp(logvar)) / 2
      s_z[n] = add_rn(mul_rn(g.eps[(size_t)b * g.d_vae + n], expf(mul_rn(0.5f, logvar))), mean);
      const float inner = sub_rn(sub_rn(add_rn(1.0f, logvar), mul_rn(mean, mean)), expf(logvar));
      g.kl_out[(size_t)b * g.d_vae + n] = div_rn(-inner, 2.0f);
    }
    __syncthreads();
    for (int n = tid; n < g.d_emb; n += kTailThreads) {
      const float v = dot_row(g.fc_out + (size_t)n * g.d_vae, s_z, g.d_vae);
      g.x_out[(size_t)b * g.d_emb + n] = g.kind == TTSENC_STYLE_VAE ? tanhf(v) : v;
    }
  }
}

// ---- packing ----
__global__ void style_conv0_pack_kernel(const float* w /*[C0][9]*/, float* out /*[9][C0]*/, int C0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 9 * C0) return;
  out[i] = w[(i % C0) * 9 + i / C0];
}
// out[t][n] = sum_j tanh(embed[t][j]) * W[n][j]  (style.py:103-105 keys, attention.py:154-155)
__global__ void style_token_proj_kernel(const float* embed, const float* W, float* out, int n_tokens, int d_emb, int dk) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_tokens * d_emb) return;
  const int t = i / d_emb, n = i % d_emb;
  float acc = 0.f;
  for (int j = 0; j < dk; ++j) acc = fmaf(tanhf(embed[t * dk + j]), W[(size_t)n * dk + j], acc);
  out[i] = acc;
}
}  // namespace

extern "C" {

int ttsenc_style_create(const ttsenc_style_dims* dims, ttsenc_style_handle** out) {
  if (!dims || !out) return TTSDEC_ERR_INVALID_ARG;
  *out = nullptr;
  const ttsenc_style_dims& d = *dims;
  if (d.n_mels <= 0 || d.n_convs < 1 || d.n_convs > kMaxConvs) return TTSDEC_ERR_DIMS;
  for (int i = 0; i < d.n_convs; ++i)
    if (d.filters[i] <= 0 || (d.filters[i] & 3) || d.filters[i] > 1024) return TTSDEC_ERR_DIMS;
  if (d.d_enc <= 0 || (d.d_enc & 3) || d.d_enc > kMaxFeat) return TTSDEC_ERR_DIMS;
  if (d.kind < TTSENC_STYLE_ENCODER || d.kind > TTSENC_STYLE_GST_VAE) return TTSDEC_ERR_DIMS;
  if (d.kind != TTSENC_STYLE_ENCODER && (d.d_emb <= 0 || d.d_emb > kMaxFeat)) return TTSDEC_ERR_DIMS;
  if (has_vae(d.kind) && (d.d_vae <= 0 || d.d_vae > kMaxVae)) return TTSDEC_ERR_DIMS;
  if (has_gst(d.kind)) {
    if (d.n_tokens <= 0 || d.n_tokens > kMaxTokens || d.n_heads <= 0 || d.n_heads > kMaxHeads) return TTSDEC_ERR_DIMS;
    if (d.d_emb % d.n_heads) return TTSDEC_ERR_DIMS;
  }
  ttsenc_style_handle* h = new (std::nothrow) ttsenc_style_handle();
  if (!h) return TTSDEC_ERR_INVALID_ARG;
  h->d = d;
  int f = d.n_mels;
  for (int i = 0; i < d.n_convs; ++i) f = half_up(f);
  h->f_last = f;
  h->bl = make_layout(d, f);
  if (!within_dma_reach(h->bl.total * sizeof(float))) {
    delete h;
    return TTSDEC_ERR_DIMS;
  }
  h->device = current_device_or_minus1();
  *out = h;
  return TTSDEC_OK;
}

int ttsenc_style_destroy(ttsenc_style_handle* h) {
  delete h;
  return TTSDEC_OK;
}

const char* ttsenc_style_last_hip_error(const ttsenc_style_handle* h) { return last_hip_error(h); }
int ttsenc_style_num_weight_tensors(const ttsenc_style_handle* h) {
  return h ? TTSENC_STYLE_W_STAGES + TTSENC_STYLE_W_PER_STAGE * h->d.n_convs : TTSDEC_ERR_INVALID_ARG;
}
size_t ttsenc_style_packed_bytes(const ttsenc_style_handle* h) { return h ? h->bl.total * sizeof(float) : 0; }
size_t ttsenc_style_workspace_bytes(const ttsenc_style_handle* h, int B, int T) {
  if (!h || B <= 0 || T <= 0) return 0;
  return carve(h->d, B, T, nullptr).total;
}

int ttsenc_style_pack_weights(ttsenc_style_handle* h, const float* const* src, int n_src, void* blob, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!h) return TTSDEC_ERR_INVALID_ARG;
  const ttsenc_style_dims& d = h->d;
  const int n_expected = ttsenc_style_num_weight_tensors(h);
  if (src && n_src == n_expected) {  // the tensors this handle's kind has must be there; the others are ignored
    for (int i = 0; i < n_src; ++i) {
      const bool need = i <= TTSENC_STYLE_W_LSTM_BHH || i >= TTSENC_STYLE_W_STAGES ||
                        (i <= TTSENC_STYLE_W_FC_OUT ? has_vae(d.kind) : has_gst(d.kind));
      if (need && !src[i]) return TTSDEC_ERR_INVALID_ARG;
    }
  }
  const int rc = pack_begin(h, src, n_src, n_expected, true, blob, ttsenc_style_packed_bytes(h), st);
  if (rc != TTSDEC_OK) return rc;
  const StyleBlob& L = h->bl;
  float* b = static_cast<float*>(blob);
  for (int i = 0; i < d.n_convs; ++i) {
    const float* const* s = src + TTSENC_STYLE_W_STAGES + TTSENC_STYLE_W_PER_STAGE * i;
    const int ci = i == 0 ? 1 : d.filters[i - 1], co = d.filters[i];
    if (i == 0) hipLaunchKernelGGL(style_conv0_pack_kernel, grid1(9 * (size_t)co), dim3(256), 0, st, s[TTSENC_STYLE_W_CONV_W], b + L.conv_w[0], co);
    else launch_conv_transpose(s[TTSENC_STYLE_W_CONV_W], b + L.conv_w[i], co, ci, 9, st);  // [Co][Ci][3][3] -> [Co][ky][kx][Ci]
    launch_copy(s[TTSENC_STYLE_W_CONV_B], b + L.bias[i], co, st);
    launch_bn_fold(s[TTSENC_STYLE_W_BN_W], s[TTSENC_STYLE_W_BN_B], s[TTSENC_STYLE_W_BN_MEAN], s[TTSENC_STYLE_W_BN_VAR], d.bn_eps,
                   b + L.alpha[i], b + L.beta[i], co, st);
  }
  const int H = d.d_enc, C = d.filters[d.n_convs - 1], Fl = h->f_last;
  // W_ih [4H][c * F' + f] -> [4H][f * C + c]: the same move as a conv weight's [Co][Ci][k] -> [Co][k][Ci]
  launch_conv_transpose(src[TTSENC_STYLE_W_LSTM_IH], b + L.w_ih, 4 * H, C, Fl, st);
  launch_copy(src[TTSENC_STYLE_W_LSTM_HH], b + L.w_hh, (size_t)4 * H * H, st);
  launch_add_vec(src[TTSENC_STYLE_W_LSTM_BIH], src[TTSENC_STYLE_W_LSTM_BHH], b + L.bsum, 4 * H, st);
  if (has_vae(d.kind)) {
    const size_t din = d.kind == TTSENC_STYLE_VAE ? d.d_enc : d.d_emb;
    launch_copy(src[TTSENC_STYLE_W_MEAN_W], b + L.mean_w, d.d_vae * din, st);
    launch_copy(src[TTSENC_STYLE_W_MEAN_B], b + L.mean_b, d.d_vae, st);
    launch_copy(src[TTSENC_STYLE_W_LOGVAR_W], b + L.logvar_w, d.d_vae * din, st);
    launch_copy(src[TTSENC_STYLE_W_LOGVAR_B], b + L.logvar_b, d.d_vae, st);
    launch_copy(src[TTSENC_STYLE_W_FC_OUT], b + L.fc_out, (size_t)d.d_emb * d.d_vae, st);
  }
  if (has_gst(d.kind)) {
    const int dk = d.d_emb / d.n_heads;
    const size_t n = (size_t)d.n_tokens * d.d_emb;
    launch_copy(src[TTSENC_STYLE_W_QUERY], b + L.wq, (size_t)d.d_emb * d.d_enc, st);
    hipLaunchKernelGGL(style_token_proj_kernel, grid1(n), dim3(256), 0, st, src[TTSENC_STYLE_W_EMBED], src[TTSENC_STYLE_W_KEY], b + L.kproj,
                       d.n_tokens, d.d_emb, dk);
    hipLaunchKernelGGL(style_token_proj_kernel, grid1(n), dim3(256), 0, st, src[TTSENC_STYLE_W_EMBED], src[TTSENC_STYLE_W_VALUE], b + L.vproj,
                       d.n_tokens, d.d_emb, dk);
  }
  return pack_end(h, b);
}

int ttsenc_style_bind_weights(ttsenc_style_handle* h, const void* blob) { return bind_blob(h, blob); }

int ttsenc_style_forward(ttsenc_style_handle* h, const float* x, int ldx, const int32_t* lengths, const float* eps, int B, int T,
                         float* enc_out, float* x_out, float* kl_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !x || !enc_out || !workspace || B <= 0 || T <= 0 || ldx < h->d.n_mels) return TTSDEC_ERR_INVALID_ARG;
  const ttsenc_style_dims& d = h->d;
  if (has_vae(d.kind) && (!eps || !kl_out)) return TTSDEC_ERR_INVALID_ARG;
  if (d.kind != TTSENC_STYLE_ENCODER && !x_out) return TTSDEC_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(enc_out) & 15)) return TTSDEC_ERR_INVALID_ARG;  // (an LSTM state buffer: read by 16-byte DMA)
  if (!h->blob) return TTSDEC_ERR_NOT_BOUND;
  if (!device_is_current(h->device)) return TTSDEC_ERR_DEVICE;
  const StageDims s = stage_dims(d, T);
  // (32-bit row indices in the conv loaders and the GEMMs)
  if ((size_t)B * s.T[0] * s.F[0] > 0x7fffffffu / 2) return TTSDEC_ERR_INVALID_ARG;
  const size_t need = carve(d, B, T, nullptr).total;
  if (!need || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255)) return TTSDEC_ERR_WORKSPACE;
  const StyleWs W = carve(d, B, T, static_cast<float*>(workspace));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const StyleBlob& bl = h->bl;
  const float* blob = h->blob;
  const int K = d.n_convs, H = d.d_enc, Tp = s.T[K - 1], Fp = s.F[K - 1], C = d.filters[K - 1];

  hipLaunchKernelGGL(style_steps_kernel, grid1(B), dim3(256), 0, st, lengths, W.steps, B, K, Tp);
  {  // stage 0
    Conv0Args a;
    a.x = x; a.ldx = ldx;
    a.w = blob + bl.conv_w[0]; a.bias = blob + bl.bias[0]; a.alpha = blob + bl.alpha[0]; a.beta = blob + bl.beta[0];
    a.out = W.act[0];
    a.T = T; a.F = d.n_mels; a.To = s.T[0]; a.Fo = s.F[0]; a.C0 = d.filters[0];
    a.n_pos = (long)B * s.T[0] * s.F[0];
    const int ppb = 256 / (a.C0 / 4);
    long blocks = (a.n_pos + ppb - 1) / ppb;
    if (blocks > 256 * 8) blocks = 256 * 8;  // a few passes per thread: its 48 weight registers are loaded once
    hipLaunchKernelGGL(style_conv0_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
  }
  for (int i = 1; i < K; ++i) {
    ConvArgs a;
    a.in = W.act[(i - 1) & 1];
    a.w = blob + bl.conv_w[i]; a.bias = blob + bl.bias[i]; a.alpha = blob + bl.alpha[i]; a.beta = blob + bl.beta[i];
    a.out = W.act[i & 1];
    a.Ti = s.T[i - 1]; a.Fi = s.F[i - 1]; a.Ci = d.filters[i - 1];
    a.To = s.T[i]; a.Fo = s.F[i]; a.Co = d.filters[i];
    a.M = B * a.To * a.Fo;
    launch_conv(a, st);
  }
  {  // gx [B * T', 4H] = feat [B * T', F' * C] . W_ih^T
    const int feat = Fp * C;
    GemmArgs g = gemm_args(planes_f32(W.act[(K - 1) & 1]), feat, planes_f32(blob + bl.w_ih), PREC_F32, B * Tp, 4 * H, feat);
    g.out = W.gx;
    launch_gemm<A_PLAIN, EPI_PLAIN>(g, st);
  }
  // The recurrence from a zero state (style.py:70).  Step t reads state buffer t & 1 and writes the other; a row past its own
  // step count carries its state over, so after T' steps buffer T' & 1 holds every row's last hidden state: that one is enc_out.
  float* hbuf[2];
  hbuf[Tp & 1] = enc_out;
  hbuf[1 - (Tp & 1)] = W.h;
  if (hipMemsetAsync(hbuf[0], 0, (size_t)B * H * sizeof(float), st) != hipSuccess) return record_hip_error(h, "memset");
  if (hipMemsetAsync(W.c, 0, (size_t)B * H * sizeof(float), st) != hipSuccess) return record_hip_error(h, "memset");
  for (int t = 0; t < Tp; ++t) {
    const int p = t & 1;
    LstmArgs a;
    memset(&a, 0, sizeof(a));
    a.a = make_seg1(hbuf[p], H, H); a.a_lo = a.a;
    a.w = make_seg1(blob + bl.w_hh, H, H); a.w_lo = a.w;
    a.bsum = blob + bl.bsum; a.h_prev = hbuf[p]; a.c = W.c; a.h_out = hbuf[1 - p];
    a.M = B; a.H = H; a.K = H; a.pz = 0.f; a.mode = 2;
    a.seq_lens = W.steps; a.seq_t = t; a.seq_L = Tp; a.seq_Lout = Tp; a.seq_reverse = 0;
    a.gx = W.gx; a.gx_ld = 4 * H; a.gx_off = 0;
    launch_lstm(a, st);
  }
  if (d.kind != TTSENC_STYLE_ENCODER) {
    TailArgs a;
    memset(&a, 0, sizeof(a));
    a.enc = enc_out; a.eps = eps;
    a.mean_w = blob + bl.mean_w; a.mean_b = blob + bl.mean_b; a.logvar_w = blob + bl.logvar_w; a.logvar_b = blob + bl.logvar_b;
    a.fc_out = blob + bl.fc_out; a.wq = blob + bl.wq; a.kproj = blob + bl.kproj; a.vproj = blob + bl.vproj;
    a.x_out = x_out; a.kl_out = kl_out;
    a.kind = d.kind; a.d_enc = H; a.d_emb = d.d_emb; a.d_vae = d.d_vae; a.n_tokens = d.n_tokens; a.n_heads = d.n_heads;
    hipLaunchKernelGGL(style_tail_kernel, dim3(B), dim3(kTailThreads), 0, st, a);
  }
  return record_hip_error(h, "style forward");
}

}  // extern "C"
