// C ABI of the VITS2 duration predictors and the length regulator (include/ttsdec.h ttsdur_*): the `self.dp(...)` and the prior
// expansion of SynthesizerTrn.infer, vits2/models.py:1288-1320.
//
// Exact fp32 on the vector ALU.  The predictors are ~1 MFLOP per token: the path is latency, not FLOPs, so every stage is one
// launch over tiles of kRows frames (256 threads, one column per lane, the tile's activations in LDS, weights from L2):
//   pw_conv_kernel   a 1- or 3-tap conv (K-major weight), optional ReLU + LayerNorm + a folded 1-column projection
//                    (DurationPredictor: two launches; the SDP's pre (+ cond(g)): one)
//   dds_layer_kernel one DDSConv layer (modules.py:84-127): depthwise dilated conv of x * mask, LN, GELU, 1x1 conv, LN, GELU,
//                    x + y; a ConvFlow's pre (1 -> C) and `+ g` in the load of its first layer; the conditioning path's proj or a
//                    ConvFlow's proj (C -> 29), inverse spline, Flip bookkeeping and the closing ElementwiseAffine in the
//                    epilogue of the last
//   lengths_kernel   w = exp(logw) * mask * length_scale, ceil, running sums, y_len, one workgroup
//   expand_kernel    the frame-rate prior (m_p, logs_p, z_p channel-last; attn) from the running sums, no dense matmul
// SDP reverse at n_flows = 4: 1 (cond(g)) + 1 (pre) + 3 (DDSConv) + 3 x 3 (ConvFlows) = 14 launches (13 without g).
// The SDP's forward direction, the duration likelihood (include/ttsdec.h ttsvits_durnll_*, models.py:87-125), runs on the same
// kernels: dds_layer_kernel<true> adds post_pre in the load, `+ x` on the posterior conditioning's proj, the spline's forward
// branch with its log-determinant, and the elementwise steps between the flows (ElementwiseAffine, the sigmoid split, Log) in
// the epilogues; nll_reduce_kernel sums each utterance's tokens.  dds_layer_kernel<false> is the reverse path's kernel as it was.
// At n_flows = 4: 1 (cond(g)) + 1 (pre) + 3 + 3 (post_convs) + 4 x 3 (post_flows) + 4 x 3 (flows) + 1 (sums) = 33 launches.
// Every weight has one record (KConv: a K-major conv weight with its bias; Vec, layout.h: a tensor copied as given), made by one
// walk at *_create; *_pack_weights and the forward calls read offsets, shapes and source indices from the records.  The two
// handle types are one struct, and the SDP has one record set (Sdp: pre, the main Trunk, flow[k] = flows.{2k+1}; post_pre, the
// posterior Trunk, pflow[k] = post_flows.{2k+1}) that Walk::sdp walks for both: all of it for ttsvits_durnll_* (full), without
// flow[0] and the posterior half for ttsdur_* kind 0, whose reverse pass runs flow[n_flows-1] .. flow[1].  Both directions open
// with run_trunk (cond(g), pre, proj(convs)) and carve one workspace shape (carve_sdp; the log-det sums only when full).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>

#include "kernels.h"

using namespace ttsdec;

namespace {
constexpr int kRows = 16;      // frames per workgroup tile
constexpr int kThreads = 256;
constexpr int kMaxC = 256;     // LDS: 3 x kRows x C floats (DDSConv), kRows x (3 C_in + N) floats (pw_conv) <= 64 KiB
constexpr int kBins = 10;      // ConvFlow num_bins
constexpr int kProj = 3 * kBins - 1;
constexpr float kTail = 5.f;   // ConvFlow tail_bound

struct KConv {  // a Conv1d weight [N, Cin, taps] packed K-major [taps * Cin][N] (pack_kmajor_kernel) and its bias [N]; float offsets
  size_t w, b;
  int N, Cin, taps;
  int src;  // its first source tensor: the weight, then the bias
  size_t n() const { return (size_t)N * Cin * taps; }
};
struct Pair { Vec w, b; };  // a weight and its bias, or a LayerNorm's gamma and beta, both copied as given
struct DdsLayer {           // one DDSConv layer: convs_sep [C, 1, 3] -> [3][C] tap-major, convs_1x1 [C][C], norms_1, norms_2
  KConv dw, pw;
  Pair n1, n2;
};
typedef DdsLayer DdsW[3];   // one DDSConv
struct Flow {               // one ConvFlow: pre [C, 1, 1], [C]; its DDSConv; proj [C][29]
  Pair pre;
  DdsW convs;
  KConv proj;
};
struct Trunk {              // a conditioning path behind its pre: the DDSConv, proj [C][C], then the ElementwiseAffine its flows open with
  DdsW convs;
  KConv proj;
  Vec m, logs;              // [2], [2]
};
struct Sdp {                // the StochasticDurationPredictor's records, the same struct in both handles
  KConv pre;                // [C][C]
  Trunk main;               // convs, proj, flows.0
  Flow flow[8];             // flow[k] is flows.{2k+1}; flow[0] (flows.1) the likelihood handle only
  Pair post_pre;            // [C, 1, 1], [C]: from here on the likelihood handle only
  Trunk post;               // post_convs, post_proj, post_flows.0
  Flow pflow[4];            // post_flows.{1, 3, 5, 7}
};
struct DurBlob {
  Sdp sdp;                   // kind 0, and ttsvits_durnll_*
  KConv c1, c2;              // kind 1: [3C][F], [3F][F]
  Pair n1, n2, p;            // [F], [F]; proj: [F], [1]
  Pair cond;                 // [C, gin], [C]
  size_t total;
  int n_src;                 // source tensors of *_pack_weights
};
// the one walk over the blob: offsets in blob order, source indices in the order include/ttsdec.h documents (src ends as their count)
struct Walk : BlobWalk {
  Pair pair(size_t nw, size_t nb) { return {vec(nw), vec(nb)}; }
  KConv conv(int N, int Cin, int taps) {
    KConv c{0, 0, N, Cin, taps, src};
    c.w = cv.take_off(c.n());
    c.b = cv.take_off(N);
    src += 2;
    return c;
  }
  void dds(DdsW& w, int C) {
    for (DdsLayer& l : w) {
      l.dw = conv(C, 1, 3);
      l.pw = conv(C, C, 1);
      l.n1 = pair(C, C);
      l.n2 = pair(C, C);
    }
  }
  void flow(Flow& f, int C) {
    f.pre = pair(C, C);
    dds(f.convs, C);
    f.proj = conv(kProj, C, 1);
  }
  void trunk(Trunk& t, int C) {
    dds(t.convs, C);
    t.proj = conv(C, C, 1);
    t.m = vec(2);
    t.logs = vec(2);
  }
  // full: every parameter of the module (ttsvits_durnll_*); else what the reverse pass reads: no flows.1, no post_*
  void sdp(Sdp& s, int C, int n_flows, bool full) {
    s.pre = conv(C, C, 1);
    trunk(s.main, C);
    for (int k = full ? 0 : 1; k < n_flows; ++k) flow(s.flow[k], C);
    if (!full) return;
    s.post_pre = pair(C, C);
    trunk(s.post, C);
    for (Flow& f : s.pflow) flow(f, C);
  }
};

struct DurHandle : HandleBase {  // what both handle types are
  ttsdur_dims d;  // (the likelihood's dims as kind 0)
  bool full;      // Walk::sdp
  DurBlob bl;
};
}  // namespace

struct ttsdur_handle : DurHandle {};
struct ttsvits_durnll_handle : DurHandle {};

namespace {

bool dims_ok(const ttsdur_dims& d) {
  if (d.kind != 0 && d.kind != 1) return false;
  if (d.kernel_size != 3) return false;
  if (d.in_channels < 4 || (d.in_channels & 3) || d.in_channels > kMaxC) return false;
  if (d.gin_channels < 0 || d.gin_channels > 4096) return false;
  if (d.kind == 0 && (d.n_flows < 2 || d.n_flows > 8)) return false;
  if (d.kind == 1 && (d.filter_channels < 4 || (d.filter_channels & 3) || d.filter_channels > kMaxC)) return false;
  return true;
}

DurBlob make_layout(const ttsdur_dims& d, bool full) {
  DurBlob L;
  memset(&L, 0, sizeof(L));
  Walk w;
  const int C = d.in_channels;
  if (d.kind == 0) {
    w.sdp(L.sdp, C, d.n_flows, full);
  } else {
    const int F = d.filter_channels;
    L.c1 = w.conv(F, C, 3);
    L.n1 = w.pair(F, F);
    L.c2 = w.conv(F, F, 3);
    L.n2 = w.pair(F, F);
    L.p = w.pair(F, 1);
  }
  if (d.gin_channels > 0) L.cond = w.pair((size_t)C * d.gin_channels, C);
  L.total = w.cv.off;
  L.n_src = w.src;
  return L;
}

template <typename Handle>
int create(const ttsdur_dims& d, bool full, Handle** out) {
  *out = nullptr;
  if (!dims_ok(d)) return TTSDEC_ERR_DIMS;
  Handle* h = new (std::nothrow) Handle();
  if (!h) return TTSDEC_ERR_INVALID_ARG;
  h->d = d;
  h->full = full;
  h->bl = make_layout(d, full);
  h->device = current_device_or_minus1();
  *out = h;
  return TTSDEC_OK;
}

// The workspaces of the two predictors (carved as layout.h's Carver comment says)
// the SDP's: four [M, C] activations (in the likelihood XP holds pre's output, then g_q = x + h_w); [B, 2, T] the flows' state;
// full: [B, T] the per-token log-det sums of the posterior and the main flows; [B, C] cond(g)
struct SdpWs { float *XP, *XA, *XB, *XC, *Z, *LDQ, *LD, *condv; };
SdpWs carve_sdp(Carver& cv, const DurHandle& h, size_t B, size_t T) {
  const size_t MC = B * T * h.d.in_channels;
  SdpWs w{};
  w.XP = cv.take(MC); w.XA = cv.take(MC); w.XB = cv.take(MC); w.XC = cv.take(MC);
  w.Z = cv.take(2 * B * T);
  if (h.full) { w.LDQ = cv.take(B * T); w.LD = cv.take(B * T); }
  w.condv = cv.take(B * h.d.in_channels);
  return w;
}
struct DpWs { float *H1, *condv; };  // [M, F] conv_1's output; [B, C] cond(g)
DpWs carve_dp(Carver& cv, const ttsdur_dims& d, size_t B, size_t T) {
  DpWs w;
  w.H1 = cv.take(B * T * d.filter_channels); w.condv = cv.take(B * d.in_channels);
  return w;
}
size_t carved_bytes(const DurHandle* h, int B, int T) {  // *_workspace_bytes
  if (!h || B <= 0 || T <= 0) return 0;
  Carver cv{nullptr};
  if (h->d.kind == 0) carve_sdp(cv, *h, B, T);
  else carve_dp(cv, h->d, B, T);
  return cv.bytes();
}

// ===========================================================================
// device helpers
// ===========================================================================
__device__ inline float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ inline float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }  // F.gelu, approximate='none'
__device__ inline float softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }                     // F.softplus, beta 1, threshold 20

// LayerNorm over the channels of the rows of buf [kRows][n] in place (modules.LayerNorm, eps 1e-5), one wave per row, then
// act: 0 none, 1 GELU.  relu_first: ReLU before the norm (DurationPredictor).
__device__ void rows_layernorm(float* buf, int n, const float* gamma, const float* beta, int act, bool relu_first) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < kRows; r += kThreads / 64) {
    float* row = buf + (size_t)r * n;
    if (relu_first)
      for (int c = lane; c < n; c += 64) row[c] = fmaxf(row[c], 0.f);
    float s = 0.f;
    for (int c = lane; c < n; c += 64) s += row[c];
    const float mean = wave_sum(s) / (float)n;
    float q = 0.f;
    for (int c = lane; c < n; c += 64) {
      const float dv = row[c] - mean;
      q += dv * dv;
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)n + 1e-5f);
    for (int c = lane; c < n; c += 64) {
      float y = (row[c] - mean) * rstd * gamma[c] + beta[c];
      row[c] = act == 1 ? gelu_erf(y) : y;
    }
  }
}

// out[r][n] = sum_k At[k][r] * W[k][n] for the tile's rows, one column per lane (K-major W from L2, At in LDS: a k step reads
// kRows contiguous floats, a broadcast); ldo: row stride of out in LDS
__device__ void tile_gemm(const float* __restrict__ At, const float* __restrict__ W, const float* __restrict__ bias, int K, int N, float* out,
                          int ldo) {
  for (int n = threadIdx.x; n < N; n += kThreads) {
    float acc[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const float w = W[(size_t)k * N + n];
      const float4* a = reinterpret_cast<const float4*>(At + (size_t)k * kRows);
#pragma unroll
      for (int q = 0; q < kRows / 4; ++q) {
        const float4 v = a[q];
        acc[4 * q + 0] = fmaf(v.x, w, acc[4 * q + 0]);
        acc[4 * q + 1] = fmaf(v.y, w, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(v.z, w, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(v.w, w, acc[4 * q + 3]);
      }
    }
    const float b = bias ? bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < kRows; ++r) out[(size_t)r * ldo + n] = acc[r] + b;
  }
}

// The inverse of transforms.unconstrained_rational_quadratic_spline (tails "linear", tail_bound 5) for one input, with the
// reference's fp32 operation order.  h: the 29 projected values of the row (already masked).
__device__ float spline_inverse(float x, const float* h, float sqrt_c) {
  if (!(x >= -kTail && x <= kTail)) return x;  // outside_interval_mask: identity
  const float kMin = 1e-3f;
  float cw[kBins + 1], ch[kBins + 1], der[kBins + 1];
  auto cum = [&](int base, float* cu) {
    float mx = -INFINITY, e[kBins], s = 0.f;
    for (int i = 0; i < kBins; ++i) mx = fmaxf(mx, h[base + i] / sqrt_c);
    for (int i = 0; i < kBins; ++i) {
      e[i] = expf(h[base + i] / sqrt_c - mx);
      s += e[i];
    }
    float c = 0.f;
    cu[0] = -kTail;
    for (int i = 0; i < kBins; ++i) {
      const float wv = kMin + (1.f - kMin * kBins) * (e[i] / s);
      c += wv;
      cu[i + 1] = (2.f * kTail) * c + (-kTail);
    }
    cu[kBins] = kTail;
  };
  cum(0, cw);
  cum(kBins, ch);
  const float edge = (float)0.5397424172369522;  // np.log(np.exp(1 - 1e-3) - 1), padded at both ends (transforms.py:71-74)
  der[0] = kMin + softplus(edge);
  der[kBins] = der[0];
  for (int i = 1; i < kBins; ++i) der[i] = kMin + softplus(h[2 * kBins + i - 1]);
  // searchsorted(cumheights, x) with the eps on the last edge (transforms.py:45-47)
  int idx = -1;
  for (int i = 0; i <= kBins; ++i) {
    const float e = i == kBins ? ch[kBins] + 1e-6f : ch[i];
    idx += x >= e ? 1 : 0;
  }
  idx = idx < 0 ? 0 : (idx > kBins - 1 ? kBins - 1 : idx);
  const float icw = cw[idx], ibw = cw[idx + 1] - cw[idx];
  const float ich = ch[idx], ih = ch[idx + 1] - ch[idx];
  const float delta = ih / ibw;
  const float d0 = der[idx], d1 = der[idx + 1];
  const float xs = x - ich;
  const float t = d0 + d1 - 2.f * delta;
  const float a = xs * t + ih * (delta - d0);
  const float b = ih * d0 - xs * t;
  const float c = -delta * xs;
  const float disc = b * b - 4.f * a * c;
  const float root = (2.f * c) / (-b - sqrtf(disc));
  return root * ibw + icw;
}

// The forward branch of the same spline (transforms.py:100-209 with inverse=False) and its log |dy/dx|: the knots as above
// (spline_inverse keeps its own copy of them: what it computes is pinned bit for bit), searchsorted on cumwidths.
__device__ float spline_forward(float x, const float* h, float sqrt_c, float* logabsdet) {
  *logabsdet = 0.f;
  if (!(x >= -kTail && x <= kTail)) return x;  // linear tails: identity, log-det 0
  const float kMin = 1e-3f;
  float cw[kBins + 1], ch[kBins + 1], der[kBins + 1];
  auto cum = [&](int base, float* cu) {
    float mx = -INFINITY, e[kBins], s = 0.f;
    for (int i = 0; i < kBins; ++i) mx = fmaxf(mx, h[base + i] / sqrt_c);
    for (int i = 0; i < kBins; ++i) {
      e[i] = expf(h[base + i] / sqrt_c - mx);
      s += e[i];
    }
    float c = 0.f;
    cu[0] = -kTail;
    for (int i = 0; i < kBins; ++i) {
      const float wv = kMin + (1.f - kMin * kBins) * (e[i] / s);
      c += wv;
      cu[i + 1] = (2.f * kTail) * c + (-kTail);
    }
    cu[kBins] = kTail;
  };
  cum(0, cw);
  cum(kBins, ch);
  const float edge = (float)0.5397424172369522;  // the same padding constant as the inverse (transforms.py:69-72)
  der[0] = kMin + softplus(edge);
  der[kBins] = der[0];
  for (int i = 1; i < kBins; ++i) der[i] = kMin + softplus(h[2 * kBins + i - 1]);
  int idx = -1;  // searchsorted(cumwidths, x) with the eps on the last edge (transforms.py:45-47, 147)
  for (int i = 0; i <= kBins; ++i) {
    const float e = i == kBins ? cw[kBins] + 1e-6f : cw[i];
    idx += x >= e ? 1 : 0;
  }
  idx = idx < 0 ? 0 : (idx > kBins - 1 ? kBins - 1 : idx);
  const float icw = cw[idx], ibw = cw[idx + 1] - cw[idx];
  const float ich = ch[idx], ih = ch[idx + 1] - ch[idx];
  const float delta = ih / ibw;
  const float d0 = der[idx], d1 = der[idx + 1];
  const float theta = (x - icw) / ibw;
  const float tomt = theta * (1.f - theta);
  const float num = ih * (delta * (theta * theta) + d0 * tomt);
  const float den = delta + (d0 + d1 - 2.f * delta) * tomt;
  const float dnum = (delta * delta) * (d1 * (theta * theta) + 2.f * delta * tomt + d0 * ((1.f - theta) * (1.f - theta)));
  *logabsdet = logf(dnum) - 2.f * logf(den);
  return ich + num / den;
}
// F.logsigmoid
__device__ inline float logsigmoid(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }

// ===========================================================================
// kernels
// ===========================================================================
// src [N, Cin, taps] (a Conv1d weight) -> dst [taps * Cin][N] (K-major: row tap * Cin + ci)
__global__ void pack_kmajor_kernel(const float* src, float* dst, int N, int Cin, int taps) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)N * Cin * taps;
  if (i >= total) return;
  const int n = (int)(i % N);
  const size_t k = i / N;
  const int tap = (int)(k / Cin), ci = (int)(k % Cin);
  dst[i] = src[((size_t)n * Cin + ci) * taps + tap];
}

struct PwArgs {
  const float* x;          // [M, Cin] channel-last
  int Cin, taps;           // taps 1 or 3 (padding 1)
  const float* in_rowvec;  // [B, Cin]: x + in_rowvec before the conv (DurationPredictor's cond), or null
  int in_mask;             // the conv reads x * mask (zero at frames >= lengths[b] and outside the utterance)
  const float* W;          // [taps * Cin][N] K-major
  const float* bias;       // [N]
  int N;
  const float* out_rowvec; // [B, N] added after the bias (the SDP's pre(x) + cond(g)), or null
  int relu_ln;             // ReLU then LayerNorm(gamma, beta)
  const float *gamma, *beta;
  const float *proj_w, *proj_b;  // when set: logw[m] = mask * (proj_b + sum_n proj_w[n] * y[n])  instead of out
  float* proj_out;
  float* out;              // [M, N]
  const int* lengths;
  int T, M;
};

__global__ __launch_bounds__(kThreads) void pw_conv_kernel(PwArgs a) {
  extern __shared__ float lds[];
  const int K = a.taps * a.Cin;
  float* At = lds;                         // [K][kRows]
  float* Z = lds + (size_t)K * kRows;      // [kRows][N]
  const int m0 = blockIdx.x * kRows;
  const int half = a.taps / 2;
  for (int idx = threadIdx.x; idx < K * kRows; idx += kThreads) {
    const int r = idx % kRows, k = idx / kRows;
    const int m = m0 + r;
    float v = 0.f;
    if (m < a.M) {
      const int b = m / a.T, t = m % a.T;
      const int tap = k / a.Cin, c = k % a.Cin;
      const int tt = t + tap - half;
      const int lim = a.in_mask ? min(a.lengths[b], a.T) : a.T;  // (a length beyond T reads no frame outside the utterance)
      if (tt >= 0 && tt < lim) {
        v = a.x[((size_t)b * a.T + tt) * a.Cin + c];
        if (a.in_rowvec) v = v + a.in_rowvec[(size_t)b * a.Cin + c];
      }
    }
    At[idx] = v;
  }
  __syncthreads();
  tile_gemm(At, a.W, a.bias, K, a.N, Z, a.N);
  __syncthreads();
  if (a.out_rowvec)
    for (int idx = threadIdx.x; idx < kRows * a.N; idx += kThreads) {
      const int m = m0 + idx / a.N;
      if (m < a.M) Z[idx] = Z[idx] + a.out_rowvec[(size_t)(m / a.T) * a.N + idx % a.N];
    }
  if (a.relu_ln) {
    __syncthreads();
    rows_layernorm(Z, a.N, a.gamma, a.beta, 0, true);
  }
  __syncthreads();
  if (a.proj_out) {  // one wave per row: proj (N -> 1) on y * mask, then * mask
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wave; r < kRows; r += kThreads / 64) {
      const int m = m0 + r;
      if (m >= a.M) continue;
      float s = 0.f;
      for (int n = lane; n < a.N; n += 64) s = fmaf(a.proj_w[n], Z[(size_t)r * a.N + n], s);
      s = wave_sum(s);
      if (lane == 0) a.proj_out[m] = (m % a.T) < a.lengths[m / a.T] ? s + a.proj_b[0] : 0.f;
    }
    return;
  }
  for (int idx = threadIdx.x; idx < kRows * a.N; idx += kThreads) {
    const int m = m0 + idx / a.N;
    if (m < a.M) a.out[(size_t)m * a.N + idx % a.N] = Z[idx];
  }
}

enum { TAIL_NONE = 0, TAIL_PROJ = 1, TAIL_FLOW = 2, TAIL_FWD = 3 };

struct DdsArgs {
  const float* xin;        // [M, C] the layer's input x (layer > 0, or the conditioning path's first layer)
  // head (a ConvFlow's first layer, xin null): x[m, c] = (pre_w[c] * x0[m] + pre_b[c]) + gadd[m, c], x0 = zin[b, c0, t] * zscale
  const float *zin, *pre_w, *pre_b, *gadd;
  float zscale;
  int c0;                  // physical channel of the flow's x0 in zin / zout (the Flips before it, counted)
  const float *dw_w, *dw_b, *pw_w, *pw_b, *n1g, *n1b, *n2g, *n2b;
  int dil, last;           // last: the DDSConv output is x * mask
  float* xout;             // [M, C] (layers before the last)
  int tail;
  const float *tw, *tb;    // TAIL_PROJ: [C][C], [C] -> xout = (proj(x) + b) * mask;  TAIL_FLOW: [C][29], [29]
  float* zout;             // TAIL_FLOW: [B, 2, T] (may be zin)
  const float *ea_m, *ea_logs;  // TAIL_FLOW of the last ConvFlow: logw = (spline(x1) - m[0]) * exp(-logs[0]) * mask
  float* logw;
  float sqrt_c;
  const int* lengths;
  int C, T, M;
  // dds_layer_kernel<true> only (the likelihood, ttsvits_durnll_forward):
  const float* w;          // [M] durations.  head with w set and zin null (post_convs): x[m, c] = pre_w[c] * w[m] + pre_b[c]
  const float* tadd;       // TAIL_PROJ: xout = (proj(x) + b + tadd[m, :]) * mask  (g_q = x + h_w)
  const float* eq;         // TAIL_PROJ: also zout = ElementwiseAffine(eq * mask) (ea_m, ea_logs) and ldinit = its log-det
  // TAIL_FWD: [C][29] tw -> the spline's forward branch on x1, cat([x0, y1]) * mask -> zout, ldacc[m] += its log |det|.
  // split (the last posterior flow): then u = sigmoid(z_u) * mask, z0 = (w - u) * mask, ldacc += logsigmoid(z_u) +
  // logsigmoid(-z_u); y = Log(z0), zout = ElementwiseAffine(cat([y, z1])) (ea_m, ea_logs: the main flows'), ldinit = their log-dets
  float *ldacc, *ldinit;   // [M] per-token log-det sums, each written by the lane that owns the row
  int split;
};

template <bool kNll>
__device__ inline float dds_input(const DdsArgs& a, int b, int t, int c) {
  const size_t m = (size_t)b * a.T + t;
  if (a.xin) return a.xin[m * a.C + c];
  if constexpr (kNll)
    if (!a.zin) return a.pre_w[c] * a.w[m] + a.pre_b[c];
  const float x0 = a.zin[((size_t)b * 2 + a.c0) * a.T + t] * a.zscale;
  return (a.pre_w[c] * x0 + a.pre_b[c]) + a.gadd[m * a.C + c];
}

template <bool kNll>
__global__ __launch_bounds__(kThreads) void dds_layer_kernel(DdsArgs a) {
  extern __shared__ float lds[];
  const int C = a.C;
  float* X = lds;                          // [kRows][C] the layer's input x, then its output
  float* Y = lds + (size_t)kRows * C;      // [kRows][C]
  float* Tt = lds + (size_t)2 * kRows * C; // [C][kRows] GEMM operand
  const int m0 = blockIdx.x * kRows;
  // depthwise conv of x * mask (kernel 3, dilation d, zero padding d), and the residual x
  for (int idx = threadIdx.x; idx < kRows * C; idx += kThreads) {
    const int r = idx / C, c = idx % C;
    const int m = m0 + r;
    float xv = 0.f, y = 0.f;
    if (m < a.M) {
      const int b = m / a.T, t = m % a.T, len = min(a.lengths[b], a.T);
      xv = dds_input<kNll>(a, b, t, c);
      float acc = 0.f;
      for (int tap = 0; tap < 3; ++tap) {
        const int tt = t + (tap - 1) * a.dil;
        const float v = tt == t ? (t < len ? xv : 0.f) : (tt >= 0 && tt < len ? dds_input<kNll>(a, b, tt, c) : 0.f);
        acc = fmaf(a.dw_w[tap * C + c], v, acc);
      }
      y = acc + a.dw_b[c];
    }
    X[idx] = xv;
    Y[idx] = y;
  }
  __syncthreads();
  rows_layernorm(Y, C, a.n1g, a.n1b, 1, false);
  __syncthreads();
  for (int idx = threadIdx.x; idx < kRows * C; idx += kThreads) {
    const int r = idx % kRows, c = idx / kRows;
    Tt[idx] = Y[r * C + c];
  }
  __syncthreads();
  tile_gemm(Tt, a.pw_w, a.pw_b, C, C, Y, C);
  __syncthreads();
  rows_layernorm(Y, C, a.n2g, a.n2b, 1, false);
  __syncthreads();
  for (int idx = threadIdx.x; idx < kRows * C; idx += kThreads) {
    const int r = idx / C;
    const int m = m0 + r;
    float v = X[idx] + Y[idx];
    if (a.last && (m >= a.M || (m % a.T) >= a.lengths[m / a.T])) v = 0.f;
    X[idx] = v;
    if (a.tail == TAIL_NONE && m < a.M) a.xout[(size_t)m * C + idx % C] = v;
  }
  if (a.tail == TAIL_NONE) return;
  __syncthreads();
  for (int idx = threadIdx.x; idx < kRows * C; idx += kThreads) {
    const int r = idx % kRows, c = idx / kRows;
    Tt[idx] = X[r * C + c];
  }
  __syncthreads();
  if (a.tail == TAIL_PROJ) {
    tile_gemm(Tt, a.tw, a.tb, C, C, Y, C);
    __syncthreads();
    for (int idx = threadIdx.x; idx < kRows * C; idx += kThreads) {
      const int m = m0 + idx / C;
      if constexpr (kNll) {
        if (m < a.M) a.xout[(size_t)m * C + idx % C] = (m % a.T) < a.lengths[m / a.T] ? Y[idx] + (a.tadd ? a.tadd[(size_t)m * C + idx % C] : 0.f) : 0.f;
      } else {
        if (m < a.M) a.xout[(size_t)m * C + idx % C] = (m % a.T) < a.lengths[m / a.T] ? Y[idx] : 0.f;
      }
    }
    if constexpr (kNll)
      if (a.eq && threadIdx.x < kRows && m0 + (int)threadIdx.x < a.M) {  // models.py:95-102: z_q = e_q * mask, then post_flows.0
        const int m = m0 + threadIdx.x, b = m / a.T, t = m % a.T;
        const bool on = t < a.lengths[b];
        for (int ch = 0; ch < 2; ++ch) {
          const size_t i = ((size_t)b * 2 + ch) * a.T + t;
          a.zout[i] = on ? a.ea_m[ch] + expf(a.ea_logs[ch]) * a.eq[i] : 0.f;
        }
        a.ldinit[m] = on ? a.ea_logs[0] + a.ea_logs[1] : 0.f;
      }
    return;
  }
  // TAIL_FLOW: h = proj(x) * mask [kRows][29]; x1 -> spline^-1; cat([x0, x1]) * mask
  tile_gemm(Tt, a.tw, a.tb, C, kProj, Y, kProj);
  __syncthreads();
  if (threadIdx.x < kRows) {
    const int r = threadIdx.x, m = m0 + r;
    if (m < a.M) {
      const int b = m / a.T, t = m % a.T;
      const bool on = t < a.lengths[b];
      float h[kProj];
      for (int j = 0; j < kProj; ++j) h[j] = on ? Y[r * kProj + j] : 0.f;
      const size_t i0 = ((size_t)b * 2 + a.c0) * a.T + t, i1 = ((size_t)b * 2 + (1 - a.c0)) * a.T + t;
      if constexpr (kNll) {  // TAIL_FWD (the only flow tail of the likelihood)
        float lad = 0.f;
        const float x0 = on ? a.zin[i0] : 0.f;
        const float y1 = on ? spline_forward(a.zin[i1], h, a.sqrt_c, &lad) : 0.f;
        float acc = on ? a.ldacc[m] + lad : 0.f;
        if (!a.split) {
          a.zout[i0] = x0;
          a.zout[i1] = y1;
        } else {  // models.py:103-117; the Flip after this flow is the posterior's fourth: channel 0 is z_u, channel 1 is z1
          const float zu = a.c0 == 0 ? x0 : y1, z1 = a.c0 == 0 ? y1 : x0;
          const float u = 1.f / (1.f + expf(-zu));
          const float y = logf(fmaxf(a.w[m] - u, 1e-5f));
          acc += logsigmoid(zu) + logsigmoid(-zu);
          a.zout[((size_t)b * 2 + 0) * a.T + t] = on ? a.ea_m[0] + expf(a.ea_logs[0]) * y : 0.f;
          a.zout[((size_t)b * 2 + 1) * a.T + t] = on ? a.ea_m[1] + expf(a.ea_logs[1]) * z1 : 0.f;
          a.ldinit[m] = on ? -y + (a.ea_logs[0] + a.ea_logs[1]) : 0.f;
        }
        a.ldacc[m] = on ? acc : 0.f;
        return;
      }
      const float x0 = a.zin[i0] * a.zscale, x1 = a.zin[i1] * a.zscale;
      const float y1 = on ? spline_inverse(x1, h, a.sqrt_c) : 0.f;
      if (a.logw) {  // Flip, then ElementwiseAffine reverse on channel 0 (= this flow's x1)
        a.logw[m] = on ? (y1 - a.ea_m[0]) * expf(-a.ea_logs[0]) : 0.f;
      } else {
        a.zout[i0] = on ? x0 : 0.f;
        a.zout[i1] = y1;
      }
    }
  }
}

// w = exp(logw) * mask * length_scale, w_ceil = ceil(w), cum = running sum over the utterance's tokens, y_len = max(1, sum):
// one lane per utterance (sums of integers below 2^24 are exact in fp32 in any order; counted in fp64 here to detect overflow)
__global__ __launch_bounds__(256) void lengths_kernel(const float* logw, const int* lengths, float ls, int B, int T, int* cum, int* y_len,
                                                       int* status) {
  __shared__ int smax[256], sflag[256];
  int mx = 0, fl = 0;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const int len = lengths[b];
    double s = 0.0;
    for (int j = 0; j < T; ++j) {
      const float w = expf(logw[(size_t)b * T + j]) * (j < len ? 1.f : 0.f) * ls;
      if (!isfinite(w)) fl |= 1;
      const float wc = ceilf(w);
      if (isfinite(wc)) s += (double)wc;
      if (s > 16777216.0) fl |= 2;
      cum[(size_t)b * T + j] = s > 16777216.0 || !(s >= 0.0) ? 0 : (int)s;
    }
    const int yl = s > 16777216.0 || !(s >= 1.0) ? 1 : (int)s;
    y_len[b] = yl;
    mx = yl > mx ? yl : mx;
  }
  smax[threadIdx.x] = mx;
  sflag[threadIdx.x] = fl;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      smax[threadIdx.x] = smax[threadIdx.x] > smax[threadIdx.x + o] ? smax[threadIdx.x] : smax[threadIdx.x + o];
      sflag[threadIdx.x] |= sflag[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    status[0] = smax[0];
    status[1] = sflag[0];
  }
}

// the frame-rate prior of kExpFrames frames of one utterance: grid (ceil(T_y / kExpFrames), B)
constexpr int kExpFrames = 32;
__global__ __launch_bounds__(256) void expand_kernel(const int* cum, const float* m, const float* logs, const float* eps, int eps_T, float ns,
                                                      int T, int Cc, int Ty, float* z_p, float* m_p, float* logs_p, float* attn) {
  extern __shared__ float lds[];
  float* E = lds;                                         // [Cc][kExpFrames + 1]
  int* tok = reinterpret_cast<int*>(lds + (size_t)Cc * (kExpFrames + 1));  // [kExpFrames]
  const int b = blockIdx.y, t0 = blockIdx.x * kExpFrames;
  const int* cb = cum + (size_t)b * T;
  if (threadIdx.x < kExpFrames) {
    const int t = t0 + threadIdx.x;
    // first j with cum[j] > t (t < cum[T-1] has one); -1: no token
    int j = -1;
    if (t < Ty && t < cb[T - 1]) {
      int lo = 0, hi = T - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cb[mid] > t) hi = mid; else lo = mid + 1;
      }
      j = lo;
    }
    tok[threadIdx.x] = j;
  }
  for (int idx = threadIdx.x; idx < Cc * kExpFrames; idx += blockDim.x) {
    const int c = idx / kExpFrames, tt = idx % kExpFrames;
    const int t = t0 + tt;
    E[c * (kExpFrames + 1) + tt] = t < Ty ? eps[((size_t)b * Cc + c) * eps_T + t] : 0.f;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < Cc * kExpFrames; idx += blockDim.x) {
    const int tt = idx / Cc, c = idx % Cc;
    const int t = t0 + tt;
    if (t >= Ty) break;
    const int j = tok[tt];
    const float mv = j >= 0 ? m[((size_t)b * T + j) * Cc + c] : 0.f;
    const float lv = j >= 0 ? logs[((size_t)b * T + j) * Cc + c] : 0.f;
    const size_t o = ((size_t)b * Ty + t) * Cc + c;
    m_p[o] = mv;
    logs_p[o] = lv;
    z_p[o] = mv + E[c * (kExpFrames + 1) + tt] * expf(lv) * ns;
  }
  if (attn)
    for (int idx = threadIdx.x; idx < T * kExpFrames; idx += blockDim.x) {
      const int tt = idx / T, j = idx % T;
      const int t = t0 + tt;
      if (t >= Ty) break;
      attn[((size_t)b * Ty + t) * T + j] = tok[tt] == j ? 1.f : 0.f;
    }
}

// models.py:109-112, 121-125 for one utterance per wave: lane l sums tokens l, l + 64, ... below the length, then the lanes are
// summed by a fixed butterfly - the same bits whatever the batch around the utterance.  terms: { sum -0.5 (log 2pi + e_q^2),
// logdet_tot_q, sum 0.5 (log 2pi + z^2), logdet_tot }; nll = (terms[2] - terms[3]) + (terms[0] - terms[1]).
// z [B, 2, T] physical channels: flip = 1 when an odd number of Flips makes logical channel ch the physical 1 - ch.
__global__ __launch_bounds__(64) void nll_reduce_kernel(const float* eq, const float* z, const float* ldq, const float* ld, const int* lengths,
                                                         int T, int flip, float* nll, float* terms, float* z_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int len = min(lengths[b], T);
  const float kLog2Pi = 1.8378770664093453f;
  const float *e0 = eq + (size_t)b * 2 * T, *e1 = e0 + T, *z0 = z + (size_t)b * 2 * T, *z1 = z0 + T;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int t = lane; t < len; t += 64) {
    s[0] += -0.5f * (kLog2Pi + e0[t] * e0[t]) + -0.5f * (kLog2Pi + e1[t] * e1[t]);
    s[1] += ldq[(size_t)b * T + t];
    s[2] += 0.5f * (kLog2Pi + z0[t] * z0[t]) + 0.5f * (kLog2Pi + z1[t] * z1[t]);
    s[3] += ld[(size_t)b * T + t];
  }
  for (int i = 0; i < 4; ++i) s[i] = wave_sum(s[i]);
  if (lane == 0) {
    nll[b] = (s[2] - s[3]) + (s[0] - s[1]);
    if (terms)
      for (int i = 0; i < 4; ++i) terms[(size_t)b * 4 + i] = s[i];
  }
  if (z_out)
    for (int t = lane; t < T; t += 64) {
      z_out[((size_t)b * 2 + flip) * T + t] = z0[t];
      z_out[((size_t)b * 2 + (1 - flip)) * T + t] = z1[t];
    }
}

size_t dds_lds(int C) { return (size_t)3 * kRows * C * sizeof(float); }
// a DDSConv launch of either direction: dds_lds, and room for the 29 projected columns of a flow tail behind Y where C < 16 leaves
// less than that (Y [kRows][29] starts at kRows * C floats: at C = 4, 8, 12 it ends past 3 * kRows * C)
size_t flow_lds(int C) { return max(dds_lds(C), (size_t)kRows * (C + kProj) * sizeof(float)); }
size_t pw_lds(int Cin, int taps, int N) { return (size_t)kRows * (taps * Cin + N) * sizeof(float); }

// *_pack_weights' steps, one per record: from src into the blob b
void pack_conv(const float* const* src, float* b, const KConv& c, hipStream_t st) {
  hipLaunchKernelGGL(pack_kmajor_kernel, grid1(c.n()), dim3(256), 0, st, src[c.src], b + c.w, c.N, c.Cin, c.taps);
  launch_copy(src[c.src + 1], b + c.b, c.N, st);
}
void pack_vec(const float* const* src, float* b, const Vec& v, hipStream_t st) { launch_copy(src[v.src], b + v.off, v.n, st); }
void pack_pair(const float* const* src, float* b, const Pair& p, hipStream_t st) {
  pack_vec(src, b, p.w, st);
  pack_vec(src, b, p.b, st);
}
void pack_dds(const float* const* src, float* b, const DdsW& w, hipStream_t st) {
  for (const DdsLayer& l : w) {
    pack_conv(src, b, l.dw, st);
    pack_conv(src, b, l.pw, st);
    pack_pair(src, b, l.n1, st);
    pack_pair(src, b, l.n2, st);
  }
}
void pack_flow(const float* const* src, float* b, const Flow& f, hipStream_t st) {
  pack_pair(src, b, f.pre, st);
  pack_dds(src, b, f.convs, st);
  pack_conv(src, b, f.proj, st);
}
void pack_trunk(const float* const* src, float* b, const Trunk& t, hipStream_t st) {
  pack_dds(src, b, t.convs, st);
  pack_conv(src, b, t.proj, st);
  pack_vec(src, b, t.m, st);
  pack_vec(src, b, t.logs, st);
}
// both *_pack_weights: the records in the order the walk made them
int pack_weights(DurHandle* h, const float* const* src, int n_src, void* blob, hipStream_t st) {
  if (!h) return TTSDEC_ERR_INVALID_ARG;
  const int rc = pack_begin(h, src, n_src, h->bl.n_src, false, blob, h->bl.total * sizeof(float), st);
  if (rc != TTSDEC_OK) return rc;
  const ttsdur_dims& d = h->d;
  const DurBlob& L = h->bl;
  float* b = static_cast<float*>(blob);
  if (d.kind == 0) {
    const Sdp& s = L.sdp;
    pack_conv(src, b, s.pre, st);
    pack_trunk(src, b, s.main, st);
    for (int k = h->full ? 0 : 1; k < d.n_flows; ++k) pack_flow(src, b, s.flow[k], st);
    if (h->full) {
      pack_pair(src, b, s.post_pre, st);
      pack_trunk(src, b, s.post, st);
      for (const Flow& f : s.pflow) pack_flow(src, b, f, st);
    }
  } else {
    pack_conv(src, b, L.c1, st);
    pack_pair(src, b, L.n1, st);
    pack_conv(src, b, L.c2, st);
    pack_pair(src, b, L.n2, st);
    pack_pair(src, b, L.p, st);
  }
  if (d.gin_channels > 0) pack_pair(src, b, L.cond, st);
  return pack_end(h, b);
}

template <bool kNll>
void run_dds(const float* b, const DdsW& w, DdsArgs a, const float* x_first, float* bufA, float* bufB, int tail, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.M + kRows - 1) / kRows);
  const float* in = x_first;
  for (int i = 0; i < 3; ++i) {
    DdsArgs l = a;
    l.xin = i > 0 ? in : x_first;  // (zin stays: the head reads it in layer 0, the spline epilogue in layer 2)
    l.dw_w = b + w[i].dw.w; l.dw_b = b + w[i].dw.b; l.pw_w = b + w[i].pw.w; l.pw_b = b + w[i].pw.b;
    l.n1g = b + w[i].n1.w.off; l.n1b = b + w[i].n1.b.off; l.n2g = b + w[i].n2.w.off; l.n2b = b + w[i].n2.b.off;
    l.dil = i == 0 ? 1 : (i == 1 ? 3 : 9);  // kernel_size ** i
    l.last = i == 2;
    l.tail = i == 2 ? tail : TAIL_NONE;
    float* out = (i % 2 == 0) ? bufA : bufB;
    if (i < 2) l.xout = out;
    hipLaunchKernelGGL(dds_layer_kernel<kNll>, dim3(nblk), dim3(kThreads), flow_lds(a.C), st, l);
    in = out;
  }
}

// The guards in front of the forward calls, in the order their codes take precedence.  args_ok: the call's own pointers.
int check_call(const DurHandle* h, int kind, bool args_ok, const float* g, int B, int T, const void* ws, size_t ws_bytes) {
  if (!h || !args_ok || !ws || B <= 0 || T <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (h->d.kind != kind) return TTSDEC_ERR_INVALID_ARG;
  if (g != nullptr && h->d.gin_channels <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (!h->blob) return TTSDEC_ERR_NOT_BOUND;
  if ((size_t)B * T > (size_t)1 << 30) return TTSDEC_ERR_DIMS;
  if (ws_bytes < carved_bytes(h, B, T) || (reinterpret_cast<uintptr_t>(ws) & 255)) return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(h->device)) return TTSDEC_ERR_DEVICE;
  return TTSDEC_OK;
}

DdsArgs dds_args(const DurHandle* h, const int* lengths, int B, int T) {  // what every DDSConv launch of a call starts from
  DdsArgs a;
  memset(&a, 0, sizeof(a));
  a.lengths = lengths; a.C = h->d.in_channels; a.T = T; a.M = B * T; a.zscale = 1.f; a.sqrt_c = sqrtf((float)a.C);
  return a;
}

// models.py:79-85, the opening of both directions: cond(g); x = pre(x) (+ cond(g)) -> XP; x = proj(convs(x, x_mask)) * x_mask -> XC
template <bool kNll>
void run_trunk(const DurHandle* h, const DdsArgs& a, const float* x, const float* g, int B, const SdpWs& w, hipStream_t st) {
  const Sdp& s = h->bl.sdp;
  const float* b = h->blob;
  const int C = a.C;
  if (g) launch_cond(g, b + h->bl.cond.w.off, b + h->bl.cond.b.off, w.condv, B, C, h->d.gin_channels, st);
  PwArgs p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.Cin = C; p.taps = 1; p.W = b + s.pre.w; p.bias = b + s.pre.b; p.N = C; p.out_rowvec = g ? w.condv : nullptr;
  p.out = w.XP; p.lengths = a.lengths; p.T = a.T; p.M = a.M;
  hipLaunchKernelGGL(pw_conv_kernel, dim3((unsigned)((a.M + kRows - 1) / kRows)), dim3(kThreads), pw_lds(C, 1, C), st, p);
  DdsArgs c = a;
  c.tw = b + s.main.proj.w; c.tb = b + s.main.proj.b; c.xout = w.XC;  // (layer 2's tail writes xout)
  run_dds<kNll>(b, s.main.convs, c, w.XP, w.XA, w.XB, TAIL_PROJ, st);
}

}  // namespace

extern "C" {

int ttsdur_create(const ttsdur_dims* dims, ttsdur_handle** out) {
  if (!dims || !out) return TTSDEC_ERR_INVALID_ARG;
  return create(*dims, false, out);
}
int ttsdur_destroy(ttsdur_handle* h) {
  delete h;
  return TTSDEC_OK;
}
const char* ttsdur_last_hip_error(const ttsdur_handle* h) { return last_hip_error(h); }
int ttsdur_num_weight_tensors(const ttsdur_handle* h) { return h ? h->bl.n_src : TTSDEC_ERR_INVALID_ARG; }
size_t ttsdur_packed_bytes(const ttsdur_handle* h) { return h ? h->bl.total * sizeof(float) : 0; }
int ttsdur_pack_weights(ttsdur_handle* h, const float* const* src, int n_src, void* blob, void* stream) {
  return pack_weights(h, src, n_src, blob, static_cast<hipStream_t>(stream));
}
int ttsdur_bind_weights(ttsdur_handle* h, const void* blob) { return bind_blob(h, blob); }
size_t ttsdur_workspace_bytes(const ttsdur_handle* h, int B, int T) { return carved_bytes(h, B, T); }

int ttsdur_sdp_reverse(ttsdur_handle* h, const float* x, const int32_t* lengths, const float* g, const float* noise, float noise_scale, int B,
                       int T, float* logw, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_call(h, 0, x && lengths && logw, g, B, T, workspace, workspace_bytes);
  if (rc != TTSDEC_OK) return rc;
  if (!noise) return TTSDEC_ERR_INVALID_ARG;  // (behind the guards above: an unbound handle answers NOT_BOUND first)
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Sdp& s = h->bl.sdp;
  const float* b = h->blob;
  const int n_flows = h->d.n_flows;
  Carver cv{static_cast<float*>(workspace)};
  const SdpWs w = carve_sdp(cv, *h, B, T);
  const DdsArgs a = dds_args(h, lengths, B, T);
  run_trunk<false>(h, a, x, g, B, w, st);
  // :127-133: the flows reversed, flows.1 dropped: [Flip, flow[n_flows-1], Flip, ..., flow[1], Flip, ElementwiseAffine];
  // z = noise * noise_scale
  int c0 = 1;  // the first Flip
  for (int k = n_flows - 1; k >= 1; --k) {
    const Flow& f = s.flow[k];
    DdsArgs c = a;
    c.zin = k == n_flows - 1 ? noise : w.Z;
    c.zscale = k == n_flows - 1 ? noise_scale : 1.f;
    c.c0 = c0;
    c.pre_w = b + f.pre.w.off; c.pre_b = b + f.pre.b.off; c.gadd = w.XC;
    c.tw = b + f.proj.w; c.tb = b + f.proj.b;
    c.zout = w.Z;
    if (k == 1) {
      c.logw = logw;
      c.ea_m = b + s.main.m.off;
      c.ea_logs = b + s.main.logs.off;
    }
    run_dds<false>(b, f.convs, c, nullptr, w.XA, w.XB, TAIL_FLOW, st);
    c0 ^= 1;  // the Flip after it
  }
  return record_hip_error(h, "sdp_reverse");
}

int ttsdur_dp_forward(ttsdur_handle* h, const float* x, const int32_t* lengths, const float* g, int B, int T, float* logw, void* workspace,
                      size_t workspace_bytes, void* stream) {
  int rc = check_call(h, 1, x && lengths && logw, g, B, T, workspace, workspace_bytes);
  if (rc != TTSDEC_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ttsdur_dims& d = h->d;
  const DurBlob& L = h->bl;
  const float* b = h->blob;
  const int C = d.in_channels, Fc = d.filter_channels, M = B * T;
  Carver cv{static_cast<float*>(workspace)};
  const DpWs w = carve_dp(cv, d, B, T);
  float *H1 = w.H1, *condv = w.condv;
  const unsigned nblk = (unsigned)((M + kRows - 1) / kRows);
  if (g) launch_cond(g, b + L.cond.w.off, b + L.cond.b.off, condv, B, C, d.gin_channels, st);
  PwArgs p;
  memset(&p, 0, sizeof(p));
  p.lengths = lengths; p.T = T; p.M = M; p.taps = 3; p.in_mask = 1; p.relu_ln = 1;
  // models.py:171-174: x = norm_1(relu(conv_1((x + cond(g)) * x_mask)))
  p.x = x; p.Cin = C; p.in_rowvec = g ? condv : nullptr; p.W = b + L.c1.w; p.bias = b + L.c1.b; p.N = Fc;
  p.gamma = b + L.n1.w.off; p.beta = b + L.n1.b.off; p.out = H1;
  hipLaunchKernelGGL(pw_conv_kernel, dim3(nblk), dim3(kThreads), pw_lds(C, 3, Fc), st, p);
  // :175-180: x = norm_2(relu(conv_2(x * x_mask))); proj(x * x_mask) * x_mask
  p.x = H1; p.Cin = Fc; p.in_rowvec = nullptr; p.W = b + L.c2.w; p.bias = b + L.c2.b;
  p.gamma = b + L.n2.w.off; p.beta = b + L.n2.b.off; p.out = nullptr;
  p.proj_w = b + L.p.w.off; p.proj_b = b + L.p.b.off; p.proj_out = logw;
  hipLaunchKernelGGL(pw_conv_kernel, dim3(nblk), dim3(kThreads), pw_lds(Fc, 3, Fc), st, p);
  return record_hip_error(h, "dp_forward");
}

int ttsdur_lengths(ttsdur_handle* h, const float* logw, const int32_t* lengths, float length_scale, int B, int T, int32_t* cum,
                   int32_t* y_len, int32_t* status, void* stream) {
  if (!h || !logw || !lengths || !cum || !y_len || !status || B <= 0 || T <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (!device_is_current(h->device)) return TTSDEC_ERR_DEVICE;
  hipLaunchKernelGGL(lengths_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), logw, lengths, length_scale, B, T, cum, y_len,
                     status);
  return record_hip_error(h, "lengths");
}

int ttsdur_expand(ttsdur_handle* h, const int32_t* cum, const float* m, const float* logs, const float* eps, int eps_T, float noise_scale,
                  int B, int T, int inter, int T_y, float* z_p, float* m_p, float* logs_p, float* attn, void* stream) {
  if (!h || !cum || !m || !logs || !eps || !z_p || !m_p || !logs_p || B <= 0 || T <= 0 || T_y <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (inter <= 0 || inter > kMaxC || eps_T < T_y || B > 65535) return TTSDEC_ERR_DIMS;
  if (!device_is_current(h->device)) return TTSDEC_ERR_DEVICE;
  const size_t lds = (size_t)inter * (kExpFrames + 1) * sizeof(float) + kExpFrames * sizeof(int);
  hipLaunchKernelGGL(expand_kernel, dim3((unsigned)((T_y + kExpFrames - 1) / kExpFrames), (unsigned)B), dim3(256), lds,
                     static_cast<hipStream_t>(stream), cum, m, logs, eps, eps_T, noise_scale, T, inter, T_y, z_p, m_p, logs_p, attn);
  return record_hip_error(h, "expand");
}

// ---------------------------------------------------------------------------------------------------------------------------
// ttsvits_durnll_*: StochasticDurationPredictor.forward(x, x_mask, w, g) (models.py:78-125), the duration likelihood
// ---------------------------------------------------------------------------------------------------------------------------
int ttsvits_durnll_create(const ttsvits_durnll_dims* dims, ttsvits_durnll_handle** out) {
  if (!dims || !out) return TTSDEC_ERR_INVALID_ARG;
  return create(ttsdur_dims{0, dims->in_channels, dims->in_channels, dims->kernel_size, dims->n_flows, dims->gin_channels}, true, out);
}
int ttsvits_durnll_destroy(ttsvits_durnll_handle* h) {
  delete h;
  return TTSDEC_OK;
}
const char* ttsvits_durnll_last_hip_error(const ttsvits_durnll_handle* h) { return last_hip_error(h); }
int ttsvits_durnll_num_weight_tensors(const ttsvits_durnll_handle* h) { return h ? h->bl.n_src : TTSDEC_ERR_INVALID_ARG; }
size_t ttsvits_durnll_packed_bytes(const ttsvits_durnll_handle* h) { return h ? h->bl.total * sizeof(float) : 0; }
int ttsvits_durnll_pack_weights(ttsvits_durnll_handle* h, const float* const* src, int n_src, void* blob, void* stream) {
  return pack_weights(h, src, n_src, blob, static_cast<hipStream_t>(stream));
}
int ttsvits_durnll_bind_weights(ttsvits_durnll_handle* h, const void* blob) { return bind_blob(h, blob); }
size_t ttsvits_durnll_workspace_bytes(const ttsvits_durnll_handle* h, int B, int T) { return carved_bytes(h, B, T); }

int ttsvits_durnll_forward(ttsvits_durnll_handle* h, const float* x, const int32_t* lengths, const float* g, const float* w, const float* noise,
                           int B, int T, float* nll_out, float* terms_out, float* z_out, void* workspace, size_t workspace_bytes,
                           void* stream) {
  int rc = check_call(h, 0, x && lengths && w && noise && nll_out, g, B, T, workspace, workspace_bytes);
  if (rc != TTSDEC_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Sdp& s = h->bl.sdp;
  const float* b = h->blob;
  Carver cv{static_cast<float*>(workspace)};
  const SdpWs ws = carve_sdp(cv, *h, B, T);
  DdsArgs a = dds_args(h, lengths, B, T);
  a.w = w;
  run_trunk<true>(h, a, x, g, B, ws, st);
  {  // :92-96: g_q = x + post_proj(post_convs(post_pre(w))) * x_mask -> XP; z_q = post_flows.0(e_q * x_mask) -> Z, LDQ
    DdsArgs c = a;
    c.pre_w = b + s.post_pre.w.off; c.pre_b = b + s.post_pre.b.off;
    c.tw = b + s.post.proj.w; c.tb = b + s.post.proj.b; c.tadd = ws.XC; c.xout = ws.XP;
    c.eq = noise; c.ea_m = b + s.post.m.off; c.ea_logs = b + s.post.logs.off; c.zout = ws.Z; c.ldinit = ws.LDQ;
    run_dds<true>(b, s.post.convs, c, nullptr, ws.XA, ws.XB, TAIL_PROJ, st);
  }
  // a ConvFlow forward and the Flip after it (modules.py:486-514): x0 is the physical channel c0 of Z
  int c0 = 0;
  auto flow = [&](const Flow& f, const float* cond, float* ldacc, bool split) {
    DdsArgs c = a;
    c.zin = ws.Z; c.zout = ws.Z; c.c0 = c0;
    c.pre_w = b + f.pre.w.off; c.pre_b = b + f.pre.b.off; c.gadd = cond;
    c.tw = b + f.proj.w; c.tb = b + f.proj.b;
    c.ldacc = ldacc;
    if (split) {  // :103-117, and flows.0
      c.split = 1;
      c.ea_m = b + s.main.m.off; c.ea_logs = b + s.main.logs.off; c.ldinit = ws.LD;
    }
    run_dds<true>(b, f.convs, c, nullptr, ws.XA, ws.XB, TAIL_FWD, st);
    c0 ^= 1;
  };
  for (int k = 0; k < 4; ++k) flow(s.pflow[k], ws.XP, ws.LDQ, k == 3);
  // (four Flips: channel 0 is z_u again, and c0 == 0)
  for (int k = 0; k < h->d.n_flows; ++k) flow(s.flow[k], ws.XC, ws.LD, false);
  hipLaunchKernelGGL(nll_reduce_kernel, dim3((unsigned)B), dim3(64), 0, st, noise, ws.Z, ws.LDQ, ws.LD, lengths, T, c0, nll_out, terms_out, z_out);
  return record_hip_error(h, "durnll_forward");
}

}  // extern "C"
