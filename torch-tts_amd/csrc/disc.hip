// C ABI of the VITS2 waveform discriminators (vits2/models.py:977-1083): DiscriminatorP(period) and DiscriminatorS, eval mode,
// exact fp32, inference only.  A second handle of the ttsvits_ family (include/ttsdec.h ttsvits_disc_*); MultiPeriodDiscriminator
// is six such handles on the host side.  Every layer's activated output is a result of the call (the feature maps), so no layer is
// fused into its neighbour.
//
// Activations are channels-last and PERIOD-MAJOR: [B, p, H, C] for the waveform folded to [B, 1, H, p] (models.py:1043), so a
// (k, 1) conv walks one contiguous column and the k taps of one output are ONE contiguous run of k * Ci floats.  DiscriminatorS
// is the same picture with p = 1 and H = T.  H = ceil(T / p); the fold and the reflect pad of the tail (models.py:1039-1043) are
// an index computation of the first layer, never a buffer.
//   layer 0 (Ci = 1)        direct: a thread owns 4 output channels of one position
//   grouped convs           (DiscriminatorS convs.1-4: 4 inputs per group, k 41, stride 4) direct: a workgroup stages ONE group's
//                           weights in LDS, a thread owns one position's outputs of that group
//   dense convs             implicit GEMM on gemm_tile.h: M = B * p * Ho rows, K = k * Ci (one K segment), N = Co; a per-row k
//                           window takes out the taps in front of the column's first row and behind its last
//   conv_post (Co = 1)      one wave per output: lanes stride the 3 * C run, then the fixed wave sum
// Bias and leaky_relu(0.1) ride in every epilogue.
#include <string.h>

#include <new>

#include "step_bodies.h"

using namespace ttsdec;

namespace {
constexpr float kLrelu = 0.1f;  // modules.LRELU_SLOPE
constexpr int kMaxConvs = TTSVITS_DISC_MAX_CONVS;
constexpr int kMaxK0 = 15, kMaxC0 = 32;     // layer 0: taps and channels its weights may take in LDS
constexpr int kGroupIn = 4, kMaxGroupK = 41, kMaxGroupOut = 16;  // the grouped convs

// One conv: where its packed weight and bias lie in the blob (floats), its shape, and its first source tensor (weight, then bias).
// Packed weight: [k][Co] for Ci = 1 (layer 0), [Co][k][Ci / groups] otherwise.
struct Conv {
  size_t w, b;
  int Ci, Co, k, stride, pad, groups, src;
  size_t n() const { return (size_t)Co * k * (Ci / groups); }
  int out_len(int Hi) const { return (Hi + 2 * pad - k) / stride + 1; }
};
struct DiscBlob {
  Conv conv[kMaxConvs], post;
  int n_convs, n_src;
  size_t total;
};
// the one walk over the blob: offsets in blob order, source indices in the order include/ttsdec.h documents
struct Walk : BlobWalk {
  Conv conv(int Ci, int Co, int k, int stride, int groups = 1) {
    Conv c{0, 0, Ci, Co, k, stride, (k - 1) / 2, groups, src};
    c.w = cv.take_off(c.n());
    c.b = cv.take_off(Co);
    src += 2;
    return c;
  }
};
}  // namespace

struct ttsvits_disc_handle : HandleBase {
  ttsvits_disc_dims d;
  DiscBlob bl;
  int p;  // columns per utterance: the period, 1 for DiscriminatorS
};

namespace {
DiscBlob make_layout(const ttsvits_disc_dims& d) {
  DiscBlob L;
  memset(&L, 0, sizeof(L));
  Walk w;
  int n = 0;
  if (d.period == 0) {  // models.py:1060-1070
    L.conv[n++] = w.conv(1, 16, 15, 1);
    L.conv[n++] = w.conv(16, 64, 41, 4, 4);
    L.conv[n++] = w.conv(64, 256, 41, 4, 16);
    L.conv[n++] = w.conv(256, 1024, 41, 4, 64);
    L.conv[n++] = w.conv(1024, 1024, 41, 4, 256);
    L.conv[n++] = w.conv(1024, 1024, 5, 1);
  } else {  // models.py:983-1032
    const int ch[6] = {1, 32, 128, 512, 1024, 1024};
    for (int i = 0; i < 5; ++i) L.conv[n++] = w.conv(ch[i], ch[i + 1], d.kernel_size, i < 4 ? d.stride : 1);
  }
  L.n_convs = n;
  L.post = w.conv(1024, 1, 3, 1);
  L.n_src = w.src;
  L.total = w.cv.off;
  return L;
}

// The shape of one call: rows per column after every layer, and whether every index stays inside 32 bits.
struct CallDims {
  int H[kMaxConvs + 2];  // H[0]: the folded input, H[i + 1]: after conv i, H[n_convs + 1]: after conv_post
  bool ok;
};
CallDims call_dims(const ttsvits_disc_handle* h, int B, int T) {
  CallDims c;
  memset(&c, 0, sizeof(c));
  const DiscBlob& L = h->bl;
  const int p = h->p;
  if (B <= 0 || T <= 0 || (size_t)B * T > 0x7fffffffu) return c;
  if (T % p != 0 && p - T % p >= T) return c;  // the reflect pad reads at most T - 1 samples back (models.py:1041)
  c.H[0] = (T + p - 1) / p;
  c.ok = true;
  for (int i = 0; i <= L.n_convs; ++i) {
    const Conv& cv = i < L.n_convs ? L.conv[i] : L.post;
    c.H[i + 1] = cv.out_len(c.H[i]);
    if ((size_t)B * p * c.H[i + 1] * cv.Co > 0x7fffffffu) c.ok = false;  // element indices of an activation
  }
  return c;
}

// scores-only calls keep the activations in the workspace: conv i writes act[i & 1]
struct DiscWs {
  float* act[2];
  size_t total;
};
DiscWs carve(const ttsvits_disc_handle* h, const CallDims& c, int B, float* base) {
  DiscWs W;
  Carver cv{base};
  size_t n[2] = {1, 1};
  for (int i = 0; i < h->bl.n_convs; ++i) {
    const size_t e = (size_t)B * h->p * c.H[i + 1] * h->bl.conv[i].Co;
    if (e > n[i & 1]) n[i & 1] = e;
  }
  W.act[0] = cv.take(n[0]);
  W.act[1] = cv.take(n[1]);
  W.total = cv.bytes();
  return W;
}

// ===========================================================================
// kernels
// ===========================================================================
__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : mul_rn(v, kLrelu); }

// Layer 0: out[b, w, ho, c] = lrelu(bias[c] + sum_tap x[b, stride * ho + tap - pad, w] * wt[tap][c]), x the folded waveform:
// x[b, hi, w] = y[b, i], i = hi * p + w, and past the end i -> 2 (T - 1) - i (F.pad(..., "reflect") on the right).  A thread
// owns 4 channels (one 16-byte store); the Co / 4 threads of a position read the same k samples.
struct FirstArgs {
  const float *y, *w, *bias;  // w [k][Co]
  float* out;
  int T, p, H, Ho, Co, k, stride, pad;
  long n_pos;  // B * p * Ho
};
__global__ __launch_bounds__(256) void disc_first_kernel(FirstArgs g) {
  __shared__ __attribute__((aligned(16))) float sw[kMaxK0 * kMaxC0 + kMaxC0];
  float* sb = sw + kMaxK0 * kMaxC0;
  for (int i = threadIdx.x; i < g.k * g.Co; i += 256) sw[i] = g.w[i];
  for (int i = threadIdx.x; i < g.Co; i += 256) sb[i] = g.bias[i];
  __syncthreads();
  const int C4 = g.Co >> 2;
  const int ppb = 256 / C4;  // positions per workgroup and pass (Co / 4 divides 256: Co is 16 or 32)
  const int c4 = threadIdx.x % C4, pin = threadIdx.x / C4;
  const f32x4 bias = *reinterpret_cast<const f32x4*>(sb + c4 * 4);
  for (long pos = (long)blockIdx.x * ppb + pin; pos < g.n_pos; pos += (long)gridDim.x * ppb) {
    const int ho = (int)(pos % g.Ho);
    const long bw = pos / g.Ho;
    const int w = (int)(bw % g.p);
    const long b = bw / g.p;
    const float* yb = g.y + (size_t)b * g.T;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < g.k; ++tap) {  // taps in order: the k-order of an output is fixed
      const int hi = g.stride * ho + tap - g.pad;
      if (hi < 0 || hi >= g.H) continue;
      long i = (long)hi * g.p + w;
      if (i >= g.T) i = 2 * ((long)g.T - 1) - i;
      const float x = yb[i];
      const f32x4 wt = *reinterpret_cast<const f32x4*>(sw + tap * g.Co + c4 * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(x, wt[j], acc[j]);
    }
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = lrelu(add_rn(acc[j], bias[j]));
    *reinterpret_cast<f32x4*>(g.out + (size_t)pos * g.Co + c4 * 4) = v;
  }
}

// The grouped convs of DiscriminatorS: group gr reads input channels 4 gr .. 4 gr + 3 and writes COG output channels.  One
// workgroup = one group (blockIdx.y) and 256 consecutive output positions: the group's weights [COG][k][4] go to LDS once, every
// lane then reads the SAME weight address (a broadcast, no bank conflicts) and its own position's 16-byte input taps.
struct GroupArgs {
  const float *in, *w, *bias;  // in [B * Li, Ci], w [Co][k][4]
  float* out;                  // [B * Lo, Co]
  int Li, Lo, Ci, Co, k, stride, pad;
  long M;  // B * Lo
};
template <int COG>
__global__ __launch_bounds__(256) void disc_group_kernel(GroupArgs g) {
  __shared__ __attribute__((aligned(16))) float sw[kMaxGroupOut * kMaxGroupK * kGroupIn];
  const int gr = blockIdx.y;
  const int nw = COG * g.k * kGroupIn;
  const float* wg = g.w + (size_t)gr * nw;
  for (int i = threadIdx.x; i < nw; i += 256) sw[i] = wg[i];
  __syncthreads();
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= g.M) return;
  const int lo = (int)(m % g.Lo);
  const long b = m / g.Lo;
  const float* xb = g.in + (size_t)b * g.Li * g.Ci + gr * kGroupIn;
  float acc[COG];
#pragma unroll
  for (int j = 0; j < COG; ++j) acc[j] = 0.f;
  for (int tap = 0; tap < g.k; ++tap) {
    const int t = g.stride * lo + tap - g.pad;
    if (t < 0 || t >= g.Li) continue;
    const f32x4 x = *reinterpret_cast<const f32x4*>(xb + (size_t)t * g.Ci);
#pragma unroll
    for (int j = 0; j < COG; ++j) {
      const f32x4 wt = *reinterpret_cast<const f32x4*>(sw + (j * g.k + tap) * kGroupIn);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[j] = fmaf(x[c], wt[c], acc[j]);
    }
  }
  float* o = g.out + (size_t)m * g.Co + gr * COG;
  const float* bs = g.bias + gr * COG;
#pragma unroll
  for (int j4 = 0; j4 < COG / 4; ++j4) {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = lrelu(add_rn(acc[j4 * 4 + j], bs[j4 * 4 + j]));
    *reinterpret_cast<f32x4*>(o + j4 * 4) = v;
  }
}

// The dense convs as an implicit GEMM.  Row m = col * Ho + ho (col = b * p + w, a column of the folded picture) contracts the
// k * Ci floats that start at act[col, stride * ho - pad, 0]: ONE K segment.  Outside the column: the first (pad - stride * ho)
// taps of its first rows, the taps at or behind Hi of its last rows - the per-row k window [k_lo, k_hi); Ci % 4 == 0 keeps every
// 16-byte column inside one tap.  A window never reaches into the next column: it is clipped at Hi first.
struct LoaderConvH {
  const void* x;
  int m0, M, Hi, Ho, Ci, k, stride, pad;
  static constexpr bool kRange = true;
  __device__ __forceinline__ int nseg() const { return 1; }
  __device__ __forceinline__ int seglen(int s) const { return s == 0 ? k * Ci : 0; }
  __device__ __forceinline__ bool row_ok(int r) const { return m0 + r < M; }
  __device__ __forceinline__ int first_row(int m) const { return stride * (m % Ho) - pad; }  // may be negative
  // element index of k = 0 of row m (may lie in front of x: only lanes inside the window are dereferenced)
  __device__ __forceinline__ long elem(int m) const { return ((long)(m / Ho) * Hi + first_row(m)) * Ci; }
  __device__ __forceinline__ gbyte* row_ptr(int r, int, int) const { return as_global(x) + elem(m0 + r) * 4; }
  __device__ __forceinline__ int k_lo(int r) const {
    const int t0 = first_row(m0 + r);
    return t0 < 0 ? -t0 * Ci : 0;
  }
  __device__ __forceinline__ int k_hi(int r) const {
    const int n = Hi - first_row(m0 + r);  // (>= pad + 1: the last output's window starts at or before row Hi - 1 - pad)
    return (n < k ? n : k) * Ci;
  }
  __device__ __forceinline__ long col_off(int c16) const { return (long)c16 * 16; }
  __device__ __forceinline__ long tile_inc(int rowb) const { return rowb; }
  // buffer-descriptor form: based at the run of THIS workgroup's first row.  elem() ascends with m - inside a column by stride * Ci,
  // across a column boundary by (Hi - stride * (Ho - 1)) * Ci >= Ci - so every offset is non-negative, and a tile's rows stay
  // within BM * stride * Ci floats of the base
  __device__ __forceinline__ const void* seg_base(int, int) const { return static_cast<const char*>(x) + elem(m0) * 4; }
  __device__ __forceinline__ unsigned row_off(int r, int) const { return (unsigned)((elem(m0 + r) - elem(m0)) * 4); }
};

// rows n0.. of the packed conv weight [Co][K]
struct LoaderRowsW {
  const float* w;
  int n0, N, K;
  static constexpr bool kRange = false;
  __device__ __forceinline__ int nseg() const { return 1; }
  __device__ __forceinline__ int seglen(int s) const { return s == 0 ? K : 0; }
  __device__ __forceinline__ bool row_ok(int r) const { return n0 + r < N; }
  __device__ __forceinline__ gbyte* row_ptr(int r, int, int) const { return as_global(w) + (long)(n0 + r) * K * 4; }
  __device__ __forceinline__ long col_off(int c16) const { return (long)c16 * 16; }
  __device__ __forceinline__ long tile_inc(int rowb) const { return rowb; }
  __device__ __forceinline__ const void* seg_base(int, int) const { return w + (size_t)n0 * K; }
  __device__ __forceinline__ unsigned row_off(int r, int) const { return (unsigned)r * (unsigned)K * 4u; }
};

struct ConvArgs {
  const float* in;  // [B * p, Hi, Ci]
  const float *w, *bias;
  float* out;  // [M, Co]
  int M, Hi, Ho, Ci, Co, k, stride, pad;
};
template <class Cfg>
__global__ __launch_bounds__(kGemmThreads, Cfg::kWavesPerSimd) void disc_conv_kernel(ConvArgs g) {
  __shared__ __attribute__((aligned(16))) float smem[Cfg::kLdsFloats];
  constexpr int BM = Cfg::BM, BN = Cfg::BN, LDO = Cfg::LDO;
  // a 1-D grid, the column tiles of one row tile side by side: workgroups that run together share their A rows in L2
  const int NT = (g.Co + BN - 1) / BN;
  const int m0 = (int)(blockIdx.x / NT) * BM, n0 = (int)(blockIdx.x % NT) * BN;
  const LoaderConvH la{g.in, m0, g.M, g.Hi, g.Ho, g.Ci, g.k, g.stride, g.pad};
  const LoaderRowsW lb{g.w, n0, g.Co, g.k * g.Ci};
  gemm_tile<Cfg, LoaderConvH, LoaderRowsW, NoGate, DmaDesc::PerSegment>(la, lb, smem);
  // models.py:1046-1047: leaky_relu(conv + bias); four columns per thread, one 16-byte store
  constexpr int Q = BN / 4;
  for (int e = threadIdx.x; e < BM * Q; e += kGemmThreads) {
    const int row = e / Q, col = (e % Q) * 4;
    const int m = m0 + row, n = n0 + col;
    if (m >= g.M || n >= g.Co) continue;  // (Co % 4 == 0: a group of four is inside or outside as a whole)
    const f32x4 bias = *reinterpret_cast<const f32x4*>(g.bias + n);
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = lrelu(add_rn(smem[row * LDO + col + j], bias[j]));
    *reinterpret_cast<f32x4*>(g.out + (size_t)m * g.Co + n) = v;
  }
}
// The tile is fixed - 64 x 64, K-sequential - whatever M is: an output's k-order then depends on nothing but the layer, and a row
// gets the same bits alone and in any batch.  (Every dense conv here has Co >= 128; the wide ones carry the family's work at
// M of 10^4 .. 10^5 rows, where the 64 x 64 tile stages half the bytes per multiply-add of the 32 x 32 split-K one.)
//
// Beyond the reference's own K (5 taps of 1024 channels) one fp32 accumulator per output is too long a chain: at 15 taps of 512
// and 1024 channels (K = 7 680, 15 360) its rounding error reached the parity bar of rtol 1e-4 / atol 1e-5 on its own
// (tests/test_dims_corners_hip.py, 1.02 of it at K = 7 680), four times the error of a blocked CPU sum.  Such layers take the
// 32 x 32 tile whose four MFMA waves each sum a quarter of every K tile (the row GEMM's small-M tile), so no accumulator sums more
// than 5 120 products in any accepted configuration.  The choice depends on the layer alone, like the tile above.
typedef TileCfg<2, 2, 1, 4> ConvTile;
typedef TileCfg<1, 1, 4, 4> LongKTile;
constexpr int kMaxSeqK = 5 * 1024;
template <class Cfg>
void launch_conv_tile(const ConvArgs& a, hipStream_t st) {
  const size_t mt = ((size_t)a.M + Cfg::BM - 1) / Cfg::BM, nt = ((size_t)a.Co + Cfg::BN - 1) / Cfg::BN;
  hipLaunchKernelGGL((disc_conv_kernel<Cfg>), dim3((unsigned)(mt * nt)), dim3(kGemmThreads), 0, st, a);
}
void launch_conv(const ConvArgs& a, hipStream_t st) {
  if (a.k * a.Ci > kMaxSeqK) launch_conv_tile<LongKTile>(a, st);
  else launch_conv_tile<ConvTile>(a, st);
}

// conv_post (C -> 1, 3 taps, models.py:1032 / 1070): one wave per output.  The taps inside the column are one run of floats
// starting at act[m - 1 + tap_lo]; a lane sums its 16-byte pieces (stride 64 pieces) in order, the wave sum is the fixed DPP tree
// of common.h.  The score lands where torch.flatten of [B, 1, H, p] puts it: scores[b, h * p + w].
struct PostArgs {
  const float *in, *w, *bias;  // in [M, C], w [k][C]
  float* scores;
  int M, H, p, C, k, pad;
};
__global__ __launch_bounds__(256) void disc_post_kernel(PostArgs g) {
  const int lane = threadIdx.x & 63;
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= g.M) return;  // (a whole wave)
  const int hh = (int)(m % g.H);
  const long col = m / g.H;
  const int lo = hh - g.pad < 0 ? g.pad - hh : 0;              // first tap inside the column
  const int hi = g.H - (hh - g.pad) < g.k ? g.H - (hh - g.pad) : g.k;  // one past the last
  const f32x4* x = reinterpret_cast<const f32x4*>(g.in + ((size_t)m - g.pad + lo) * g.C);
  const f32x4* w = reinterpret_cast<const f32x4*>(g.w + (size_t)lo * g.C);
  const int n4 = (hi - lo) * (g.C >> 2);
  float acc = 0.f;
  for (int i = lane; i < n4; i += 64) {
    const f32x4 a = x[i], b = w[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(a[j], b[j], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    const long b = col / g.p;
    const int wv = (int)(col % g.p);
    g.scores[(size_t)b * g.H * g.p + (size_t)hh * g.p + wv] = add_rn(acc, g.bias[0]);
  }
}
}  // namespace

extern "C" {

int ttsvits_disc_create(const ttsvits_disc_dims* dims, ttsvits_disc_handle** out) {
  if (!dims || !out) return TTSDEC_ERR_INVALID_ARG;
  *out = nullptr;
  const ttsvits_disc_dims& d = *dims;
  if (d.period < 0 || d.period > 4096) return TTSDEC_ERR_DIMS;
  if (d.period > 0) {  // (k, 1) convs with padding (k - 1) / 2: odd k, as get_padding assumes; layer 0 keeps its taps in LDS
    if (d.kernel_size < 1 || !(d.kernel_size & 1) || d.kernel_size > kMaxK0) return TTSDEC_ERR_DIMS;
    if (d.stride < 1 || d.stride > 16) return TTSDEC_ERR_DIMS;
  }
  ttsvits_disc_handle* h = new (std::nothrow) ttsvits_disc_handle();
  if (!h) return TTSDEC_ERR_INVALID_ARG;
  h->d = d;
  h->p = d.period > 0 ? d.period : 1;
  h->bl = make_layout(d);
  h->device = current_device_or_minus1();
  *out = h;
  return TTSDEC_OK;
}

int ttsvits_disc_destroy(ttsvits_disc_handle* h) {
  delete h;
  return TTSDEC_OK;
}

const char* ttsvits_disc_last_hip_error(const ttsvits_disc_handle* h) { return last_hip_error(h); }
int ttsvits_disc_num_weight_tensors(const ttsvits_disc_handle* h) { return h ? h->bl.n_src : TTSDEC_ERR_INVALID_ARG; }
size_t ttsvits_disc_packed_bytes(const ttsvits_disc_handle* h) { return h ? h->bl.total * sizeof(float) : 0; }
size_t ttsvits_disc_workspace_bytes(const ttsvits_disc_handle* h, int B, int T) {
  if (!h) return 0;
  const CallDims c = call_dims(h, B, T);
  return c.ok ? carve(h, c, B, nullptr).total : 0;
}

int ttsvits_disc_pack_weights(ttsvits_disc_handle* h, const float* const* src, int n_src, void* blob, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = pack_begin(h, src, n_src, ttsvits_disc_num_weight_tensors(h), false, blob, ttsvits_disc_packed_bytes(h), st);
  if (rc != TTSDEC_OK) return rc;
  const DiscBlob& L = h->bl;
  float* b = static_cast<float*>(blob);
  for (int i = 0; i <= L.n_convs; ++i) {
    const Conv& c = i < L.n_convs ? L.conv[i] : L.post;
    // [Co][Ci / groups][k] -> [Co][k][Ci / groups]; layer 0 and conv_post, read as [1][Co * Ci][k] -> [k][Co * Ci]
    if (c.Ci == 1 || c.Co == 1) launch_conv_transpose(src[c.src], b + c.w, 1, c.Co * c.Ci, c.k, st);
    else launch_conv_transpose(src[c.src], b + c.w, c.Co, c.Ci / c.groups, c.k, st);
    launch_copy(src[c.src + 1], b + c.b, c.Co, st);
  }
  return pack_end(h, b);
}

int ttsvits_disc_bind_weights(ttsvits_disc_handle* h, const void* blob) { return bind_blob(h, blob); }

int ttsvits_disc_forward(ttsvits_disc_handle* h, const float* y, int B, int T, float* scores, float* const* fmaps, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (!h || !y || !scores || B <= 0 || T <= 0) return TTSDEC_ERR_INVALID_ARG;
  const DiscBlob& L = h->bl;
  const int p = h->p;
  if (fmaps)
    for (int i = 0; i < L.n_convs; ++i)
      if (!fmaps[i] || (reinterpret_cast<uintptr_t>(fmaps[i]) & 15)) return TTSDEC_ERR_INVALID_ARG;
  if (!h->blob) return TTSDEC_ERR_NOT_BOUND;
  if (!device_is_current(h->device)) return TTSDEC_ERR_DEVICE;
  const CallDims c = call_dims(h, B, T);
  if (!c.ok) return TTSDEC_ERR_DIMS;
  DiscWs W{{nullptr, nullptr}, 0};
  if (!fmaps) {  // scores only: the activations live in the workspace
    if (!workspace || workspace_bytes < carve(h, c, B, nullptr).total || (reinterpret_cast<uintptr_t>(workspace) & 255))
      return TTSDEC_ERR_WORKSPACE;
    W = carve(h, c, B, static_cast<float*>(workspace));
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* blob = h->blob;
  const float* in = nullptr;
  for (int i = 0; i < L.n_convs; ++i) {
    const Conv& cv = L.conv[i];
    float* out = fmaps ? fmaps[i] : W.act[i & 1];
    const int Hi = c.H[i], Ho = c.H[i + 1];
    const long M = (long)B * p * Ho;
    if (cv.Ci == 1) {
      FirstArgs a;
      a.y = y; a.w = blob + cv.w; a.bias = blob + cv.b; a.out = out;
      a.T = T; a.p = p; a.H = Hi; a.Ho = Ho; a.Co = cv.Co; a.k = cv.k; a.stride = cv.stride; a.pad = cv.pad;
      a.n_pos = M;
      const int ppb = 256 / (cv.Co / 4);
      long blocks = (M + ppb - 1) / ppb;
      if (blocks > 256 * 16) blocks = 256 * 16;  // a few passes per thread: the weights are staged once per workgroup
      hipLaunchKernelGGL(disc_first_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    } else if (cv.groups > 1) {
      GroupArgs a;
      a.in = in; a.w = blob + cv.w; a.bias = blob + cv.b; a.out = out;
      a.Li = Hi; a.Lo = Ho; a.Ci = cv.Ci; a.Co = cv.Co; a.k = cv.k; a.stride = cv.stride; a.pad = cv.pad;
      a.M = M;
      const dim3 grid((unsigned)((M + 255) / 256), cv.groups);
      if (cv.Co / cv.groups == 16) hipLaunchKernelGGL(disc_group_kernel<16>, grid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL(disc_group_kernel<4>, grid, dim3(256), 0, st, a);
    } else {
      ConvArgs a;
      a.in = in; a.w = blob + cv.w; a.bias = blob + cv.b; a.out = out;
      a.M = (int)M; a.Hi = Hi; a.Ho = Ho; a.Ci = cv.Ci; a.Co = cv.Co; a.k = cv.k; a.stride = cv.stride; a.pad = cv.pad;
      launch_conv(a, st);
    }
    in = out;
  }
  {
    const Conv& cv = L.post;
    PostArgs a;
    a.in = in; a.w = blob + cv.w; a.bias = blob + cv.b; a.scores = scores;
    a.H = c.H[L.n_convs]; a.p = p; a.C = cv.Ci; a.k = cv.k; a.pad = cv.pad;
    a.M = B * p * a.H;
    hipLaunchKernelGGL(disc_post_kernel, dim3((unsigned)((a.M + 3) / 4)), dim3(256), 0, st, a);
  }
  return record_hip_error(h, "disc forward");
}

}  // extern "C"
