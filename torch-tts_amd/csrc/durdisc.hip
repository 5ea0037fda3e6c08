// C ABI of the VITS2 duration discriminators (vits2/models.py:183-329): DurationDiscriminatorV1 and DurationDiscriminatorV2, eval
// mode, exact fp32, inference only.  A third handle kind of the ttsvits_ family (include/ttsdec.h ttsvits_durdisc_*).
//
// Activations are CHANNEL-LAST [B * T, C], one row per token, as the text encoder writes them.  C = in_channels, F =
// filter_channels, every conv has 3 taps.
//   trunk (once per call)        V2: h = norm_2(relu(conv_2(norm_1(relu(conv_1(x m))) m)));  V1: h = conv_2(conv_1(x m) m)
//   probability (per duration)   u = pre_out_conv_1(cat([h, dur_proj(dur)]) m)  [V2: pre_out_norm_1(relu(u))]
//                                u = pre_out_conv_2(u m)                        [V2: pre_out_norm_2(relu(u))]
//                                p = sigmoid(output_layer(u m))
// The four wide convs (conv_1, conv_2, the h half of pre_out_conv_1, pre_out_conv_2) are implicit GEMMs of the GEMM core
// (launch_gemm, A_CONV + EPI_GENERIC, exact fp32) on its 32 x 32 split-K tile whatever M is (GemmArgs::fixed_tile): an output's
// summation order depends on nothing but the layer, so an utterance gets the same bits alone and in any batch.
// cat([h, d]) is never built.  d = dur_proj(dur) is rank one (d[c, t] = w_dur[c] dur[t] + b_dur[c]), so its half of pre_out_conv_1
// folds at pack time into two [3][F] tables, S[tap][n] = sum_c W[n, F + c, tap] w_dur[c] and O[tap][n] = sum_c W[n, F + c, tap]
// b_dur[c] (c ascending), and contributes sum_tap m[t + tap - 1] (S[tap][n] dur[t + tap - 1] + O[tap][n]) at token t.  The h half is
// one GEMM per call, shared by the call's durations; pre_out_conv_2 then runs over the n_dur * M rows in one launch.
// The masks are SELECTS on the token's position against its utterance's length, never multiplications: what x, hidden and dur hold
// at masked tokens is not read into any result.  No atomics; every sum has a fixed order.
#include <string.h>

#include <new>

#include "kernels.h"

using namespace ttsdec;

namespace {
constexpr int kTaps = 3;
constexpr int kMaxChannels = TTSVITS_DURDISC_MAX_CHANNELS;  // launch_layernorm's and the row kernels' widest row
constexpr float kLnEps = 1e-5f;                             // modules.LayerNorm

struct Conv {  // packed weight [N][3][K] (tap-major, as the GEMM core reads it) and bias [N]; offsets in floats
  size_t w, b;
  int N, K, src;
};
struct Norm {  // modules.LayerNorm gamma, beta [F]
  size_t g, b;
  int src;
};
struct DurDiscBlob {
  Conv c1, c2, p1, p2;       // conv_1, conv_2, the h half of pre_out_conv_1, pre_out_conv_2
  Norm n1, n2, pn1, pn2;     // V2 only
  size_t slope, offset;      // the folded dur_proj half of pre_out_conv_1: [3][F] each
  int dur_src;               // dur_proj.weight, dur_proj.bias
  size_t ow, ob;             // output_layer.0: weight [F], bias [1]
  int out_src;
  int n_src;
  size_t total;
};
// the one walk over the blob: offsets in blob order, source indices in the order include/ttsdec.h documents
struct Walk : BlobWalk {
  Conv conv(int N, int K, int n_src = 2) {
    Conv c{0, 0, N, K, src};
    c.w = cv.take_off((size_t)N * kTaps * K);
    c.b = cv.take_off(N);
    src += n_src;
    return c;
  }
  Norm norm(int F) {
    Norm n{cv.take_off(F), 0, src};
    n.b = cv.take_off(F);
    src += 2;
    return n;
  }
};
}  // namespace

struct ttsvits_durdisc_handle : HandleBase {
  ttsvits_durdisc_dims d;
  DurDiscBlob bl;
};

namespace {
DurDiscBlob make_layout(const ttsvits_durdisc_dims& d) {
  DurDiscBlob L;
  memset(&L, 0, sizeof(L));
  Walk w;
  const int C = d.in_channels, F = d.filter_channels;
  const bool v2 = d.version == 2;
  L.c1 = w.conv(F, C);
  if (v2) L.n1 = w.norm(F);
  L.c2 = w.conv(F, F);
  if (v2) L.n2 = w.norm(F);
  L.dur_src = w.src;
  w.src += 2;
  L.slope = w.cv.take_off((size_t)kTaps * F);
  L.offset = w.cv.take_off((size_t)kTaps * F);
  L.p1 = w.conv(F, F);
  if (v2) L.pn1 = w.norm(F);
  L.p2 = w.conv(F, F);
  if (v2) L.pn2 = w.norm(F);
  L.out_src = w.src;
  w.src += 2;
  L.ow = w.cv.take_off(F);
  L.ob = w.cv.take_off(1);
  L.n_src = w.src;
  L.total = w.cv.off;
  return L;
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// Pack time: the dur_proj half of pre_out_conv_1 (w [F][2F][3]) folded with dur_proj (wd, bd [F]).  One thread per (tap, n).
__global__ void durdisc_fold_kernel(const float* w, const float* wd, const float* bd, float* slope, float* offset, int F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kTaps * F) return;
  const int tap = i / F, n = i - tap * F;
  const float* row = w + ((size_t)n * 2 * F + F) * kTaps + tap;
  float s = 0.f, o = 0.f;
  for (int c = 0; c < F; ++c) {
    const float wv = row[(size_t)c * kTaps];
    s = fmaf(wv, wd[c], s);
    o = fmaf(wv, bd[c], o);
  }
  slope[i] = s;
  offset[i] = o;
}

// out[m, :] = token m is inside its utterance ? in[m, :] : 0, and (mask != nullptr) mask[m] = 1 / 0.  One thread per four channels.
__global__ __launch_bounds__(256) void durdisc_mask_kernel(const float* in, const int* lengths, float* out, float* mask, int T, int C4, size_t n4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int m = (int)(i / C4);
  const bool live = m % T < lengths[m / T];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (live) v = reinterpret_cast<const f32x4*>(in)[i];
  reinterpret_cast<f32x4*>(out)[i] = v;
  if (mask != nullptr && i % C4 == 0) mask[m] = live ? 1.0f : 0.0f;
}

// A row of F <= 256 NJ channels spread over a wave as f32x4: piece j of a lane holds channels 4 (lane + 64 j) .. + 3.
template <int NJ>
struct RowLanes {
  int lane, F4;
  __device__ __forceinline__ bool has(int j) const { return lane + 64 * j < F4; }
  __device__ __forceinline__ f32x4 load(const float* p, int j) const {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    return has(j) ? reinterpret_cast<const f32x4*>(p)[lane + 64 * j] : z;
  }
  __device__ __forceinline__ void store(float* p, int j, f32x4 v) const {
    if (has(j)) reinterpret_cast<f32x4*>(p)[lane + 64 * j] = v;
  }
  // V2's relu -> LayerNorm of the row held in v, in place
  __device__ __forceinline__ void relu_layernorm(f32x4 (&v)[NJ], const float* gamma, const float* beta, int F) const {
    float s[4 * NJ];
    bool ok[4 * NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ok[4 * j + e] = has(j);
        s[4 * j + e] = v[j][e] > 0.f ? v[j][e] : 0.f;
      }
    float mean, rstd;
    wave_layernorm_stats(s, ok, F, kLnEps, mean, rstd);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const f32x4 g = load(gamma, j), b = load(beta, j);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[j][e] = layernorm_value(s[4 * j + e], mean, rstd, g[e], b[e]);
    }
  }
};

// Between the two pre_out convs, one wave per token row m = (b, t): u0 [M, F] is the h half of pre_out_conv_1 without its bias.
// For every duration j < n_dur:  u = u0[m] + bias + sum_tap (token t + tap - 1 inside the utterance ? S[tap] dur[j, b, t + tap - 1] +
// O[tap] : 0);  V2: u = pre_out_norm_1(relu(u));  out[j, m] = token t inside the utterance ? u : 0  - the input of pre_out_conv_2.
struct MidArgs {
  const float *u0, *bias, *slope, *offset, *gamma, *beta, *dur;
  const int* lengths;
  float* out;
  int M, T, F, n_dur, v2;
};
template <int NJ>
__global__ __launch_bounds__(256) void durdisc_mid_kernel(MidArgs g) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= g.M) return;  // (a whole wave)
  const RowLanes<NJ> rl{(int)(threadIdx.x & 63), g.F >> 2};
  const int b = m / g.T, t = m - b * g.T, len = g.lengths[b] < g.T ? g.lengths[b] : g.T;  // (never a token beyond the row of dur)
  const size_t MF = (size_t)g.M * g.F;
  float* orow = g.out + (size_t)m * g.F;
  if (t >= len) {  // (the same in every lane)
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < g.n_dur; ++j)
#pragma unroll
      for (int i = 0; i < NJ; ++i) rl.store(orow + j * MF, i, z);
    return;
  }
  f32x4 base[NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    const f32x4 u = rl.load(g.u0 + (size_t)m * g.F, i), bs = rl.load(g.bias, i);
#pragma unroll
    for (int e = 0; e < 4; ++e) base[i][e] = add_rn(u[e], bs[e]);
  }
  for (int j = 0; j < g.n_dur; ++j) {
    const float* dur = g.dur + ((size_t)j * g.M + (size_t)b * g.T);
    f32x4 v[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) v[i] = base[i];
#pragma unroll
    for (int tap = 0; tap < kTaps; ++tap) {
      const int tt = t + tap - 1;
      if (tt < 0 || tt >= len) continue;  // (the same in every lane)
      const float dv = dur[tt];
#pragma unroll
      for (int i = 0; i < NJ; ++i) {
        const f32x4 s = rl.load(g.slope + (size_t)tap * g.F, i), o = rl.load(g.offset + (size_t)tap * g.F, i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][e] = add_rn(v[i][e], add_rn(mul_rn(s[e], dv), o[e]));
      }
    }
    if (g.v2) rl.relu_layernorm(v, g.gamma, g.beta, g.F);
#pragma unroll
    for (int i = 0; i < NJ; ++i) rl.store(orow + j * MF, i, v[i]);
  }
}

// After pre_out_conv_2, one wave per row r of the n_dur * M rows of u (bias added by the GEMM; V2: ReLU too):
// V2: u = pre_out_norm_2(u);  logit = (token inside its utterance ? sum_n u[n] w[n] : 0) + b;  prob = sigmoid(logit).
struct OutArgs {
  const float *u, *gamma, *beta, *w, *b;
  const int* lengths;
  float *prob, *logit;  // [n_dur * M]; logit may be nullptr
  int rows, M, T, F, v2;
};
template <int NJ>
__global__ __launch_bounds__(256) void durdisc_out_kernel(OutArgs g) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= g.rows) return;  // (a whole wave)
  const RowLanes<NJ> rl{(int)(threadIdx.x & 63), g.F >> 2};
  const int m = r % g.M, b = m / g.T, t = m - b * g.T;
  float acc = 0.f;
  if (t < g.lengths[b]) {  // (the same in every lane)
    f32x4 v[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) v[i] = rl.load(g.u + (size_t)r * g.F, i);
    if (g.v2) rl.relu_layernorm(v, g.gamma, g.beta, g.F);  // (the GEMM's ReLU left nothing negative: relu is the identity here)
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
      const f32x4 w = rl.load(g.w, i);  // (zero beyond F)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(v[i][e], w[e], acc);
    }
    acc = wave_sum(acc);
  }
  if ((threadIdx.x & 63) == 0) {
    const float logit = add_rn(acc, g.b[0]);
    g.prob[r] = sigmoid_f(logit);
    if (g.logit != nullptr) g.logit[r] = logit;
  }
}

template <class Args>
void launch_rows(void (*k1)(Args), void (*k2)(Args), void (*k4)(Args), const Args& a, int rows, int F, hipStream_t st) {
  hipLaunchKernelGGL(F <= 256 ? k1 : (F <= 512 ? k2 : k4), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a);
}

// out [M, c.N] = [mask *] [relu](conv_3(a [M, c.K]) [+ bias]); M = rows of period T
void conv(const float* blob, const Conv& c, const float* a, float* out, int M, int T, bool bias, int act, const float* mask, hipStream_t st) {
  GemmArgs g = conv_gemm_args(planes_f32(a), planes_f32(blob + c.w), PREC_F32, M, T, c.K, kTaps, c.N);
  g.bias = bias ? blob + c.b : nullptr;
  g.act = act; g.row_mask = mask;
  g.out = out;
  g.fixed_tile = 1;
  launch_gemm<A_CONV, EPI_GENERIC>(g, st);
}

struct DurDiscWs {
  float *mask, *xm, *a, *b, *u0, *v, *w;  // [M]; [M, max(C, F)]; [M, F] x 3; [n_dur M, F] x 2
};
DurDiscWs carve(Carver& cv, const ttsvits_durdisc_dims& d, size_t M, size_t n_dur) {
  const size_t C = d.in_channels, F = d.filter_channels;
  DurDiscWs w;
  w.mask = cv.take(M); w.xm = cv.take(M * (C > F ? C : F));
  w.a = cv.take(M * F); w.b = cv.take(M * F); w.u0 = cv.take(M * F);
  w.v = cv.take(n_dur * M * F); w.w = cv.take(n_dur * M * F);
  return w;
}
// rows and element offsets of the GEMM core are 32-bit: n_dur * B * T rows of up to 4096 channels have to fit
bool rows_fit(int B, int T, int n_dur) { return (size_t)n_dur * B * T <= (size_t)INT32_MAX / 4096; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the guards of the two calls, in the order their codes take precedence
int check_call(const ttsvits_durdisc_handle* h, bool args_ok, int B, int T, int n_dur, const void* ws, size_t ws_bytes) {
  if (!h || !args_ok || B <= 0 || T <= 0 || (n_dur != 1 && n_dur != 2)) return TTSDEC_ERR_INVALID_ARG;
  if (!h->blob) return TTSDEC_ERR_NOT_BOUND;
  if (!rows_fit(B, T, n_dur)) return TTSDEC_ERR_DIMS;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_bytes < ttsvits_durdisc_workspace_bytes(h, B, T, n_dur)) return TTSDEC_ERR_INVALID_ARG;
  if (!device_is_current(h->device)) return TTSDEC_ERR_DEVICE;
  return TTSDEC_OK;
}
}  // namespace

extern "C" {

int ttsvits_durdisc_create(const ttsvits_durdisc_dims* dims, ttsvits_durdisc_handle** out) {
  if (!dims || !out) return TTSDEC_ERR_INVALID_ARG;
  *out = nullptr;
  const ttsvits_durdisc_dims& d = *dims;
  if (d.version != 1 && d.version != 2) return TTSDEC_ERR_DIMS;
  if (d.kernel_size != kTaps) return TTSDEC_ERR_DIMS;
  for (int c : {d.in_channels, d.filter_channels})
    if (c <= 0 || (c & 3) || c > kMaxChannels) return TTSDEC_ERR_DIMS;
  ttsvits_durdisc_handle* h = new (std::nothrow) ttsvits_durdisc_handle();
  if (!h) return TTSDEC_ERR_INVALID_ARG;
  h->d = d;
  h->bl = make_layout(d);
  h->device = current_device_or_minus1();
  *out = h;
  return TTSDEC_OK;
}

int ttsvits_durdisc_destroy(ttsvits_durdisc_handle* h) {
  delete h;
  return TTSDEC_OK;
}

const char* ttsvits_durdisc_last_hip_error(const ttsvits_durdisc_handle* h) { return last_hip_error(h); }
int ttsvits_durdisc_num_weight_tensors(const ttsvits_durdisc_handle* h) { return h ? h->bl.n_src : TTSDEC_ERR_INVALID_ARG; }
size_t ttsvits_durdisc_packed_bytes(const ttsvits_durdisc_handle* h) { return h ? h->bl.total * sizeof(float) : 0; }

int ttsvits_durdisc_pack_weights(ttsvits_durdisc_handle* h, const float* const* src, int n_src, void* blob, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = pack_begin(h, src, n_src, ttsvits_durdisc_num_weight_tensors(h), false, blob, ttsvits_durdisc_packed_bytes(h), st);
  if (rc != TTSDEC_OK) return rc;
  const DurDiscBlob& L = h->bl;
  const int F = h->d.filter_channels;
  float* b = static_cast<float*>(blob);
  for (const Conv* c : {&L.c1, &L.c2, &L.p1, &L.p2}) {
    // [N][K][3] -> [N][3][K]; pre_out_conv_1 is [F][2F][3], of which the GEMM takes input channels 0 .. F-1
    launch_conv_transpose(src[c->src], b + c->w, c->N, c->K, kTaps, st, c == &L.p1 ? (size_t)2 * F * kTaps : 0);
    launch_copy(src[c->src + 1], b + c->b, c->N, st);
  }
  hipLaunchKernelGGL(durdisc_fold_kernel, grid1((size_t)kTaps * F), dim3(256), 0, st, src[L.p1.src], src[L.dur_src], src[L.dur_src + 1],
                     b + L.slope, b + L.offset, F);
  if (h->d.version == 2)
    for (const Norm* n : {&L.n1, &L.n2, &L.pn1, &L.pn2}) {
      launch_copy(src[n->src], b + n->g, F, st);
      launch_copy(src[n->src + 1], b + n->b, F, st);
    }
  launch_copy(src[L.out_src], b + L.ow, F, st);
  launch_copy(src[L.out_src + 1], b + L.ob, 1, st);
  return pack_end(h, b);
}

int ttsvits_durdisc_bind_weights(ttsvits_durdisc_handle* h, const void* blob) { return bind_blob(h, blob); }

size_t ttsvits_durdisc_workspace_bytes(const ttsvits_durdisc_handle* h, int B, int T, int n_dur) {
  if (!h || B <= 0 || T <= 0 || n_dur <= 0 || n_dur > 2 || !rows_fit(B, T, n_dur)) return 0;
  Carver cv{nullptr};
  carve(cv, h->d, (size_t)B * T, n_dur);
  return cv.bytes();
}

int ttsvits_durdisc_trunk(ttsvits_durdisc_handle* h, const float* x, const int32_t* lengths, int B, int T, float* hidden_out, void* workspace,
                          size_t workspace_bytes, void* stream) {
  const int rc = check_call(h, x && lengths && hidden_out && aligned16(x) && aligned16(hidden_out), B, T, 1, workspace, workspace_bytes);
  if (rc != TTSDEC_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const DurDiscBlob& L = h->bl;
  const float* blob = h->blob;
  const int M = B * T, C = h->d.in_channels, F = h->d.filter_channels;
  Carver cv{static_cast<float*>(workspace)};
  const DurDiscWs w = carve(cv, h->d, M, 1);
  const size_t n4 = (size_t)M * (C / 4);
  hipLaunchKernelGGL(durdisc_mask_kernel, grid1(n4), dim3(256), 0, st, x, lengths, w.xm, w.mask, T, C / 4, n4);
  if (h->d.version == 2) {  // models.py:317-322
    conv(blob, L.c1, w.xm, w.a, M, T, true, 1, nullptr, st);
    launch_layernorm(w.a, blob + L.n1.g, blob + L.n1.b, w.mask, nullptr, w.b, nullptr, nullptr, M, F, st);
    conv(blob, L.c2, w.b, w.a, M, T, true, 1, nullptr, st);
    launch_layernorm(w.a, blob + L.n2.g, blob + L.n2.b, w.mask, nullptr, hidden_out, nullptr, nullptr, M, F, st);
  } else {  // models.py:243-247
    conv(blob, L.c1, w.xm, w.a, M, T, true, 0, w.mask, st);
    conv(blob, L.c2, w.a, hidden_out, M, T, true, 0, w.mask, st);
  }
  return record_hip_error(h, "durdisc trunk");
}

int ttsvits_durdisc_prob(ttsvits_durdisc_handle* h, const float* hidden, const int32_t* lengths, const float* dur, int n_dur, int B, int T,
                         float* prob_out, float* logit_out, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = check_call(h, hidden && lengths && dur && prob_out && aligned16(hidden), B, T, n_dur, workspace, workspace_bytes);
  if (rc != TTSDEC_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const DurDiscBlob& L = h->bl;
  const float* blob = h->blob;
  const int M = B * T, F = h->d.filter_channels, v2 = h->d.version == 2;
  Carver cv{static_cast<float*>(workspace)};
  const DurDiscWs w = carve(cv, h->d, M, n_dur);
  const size_t n4 = (size_t)M * (F / 4);
  hipLaunchKernelGGL(durdisc_mask_kernel, grid1(n4), dim3(256), 0, st, hidden, lengths, w.xm, (float*)nullptr, T, F / 4, n4);  // (nothing here reads the [M] mask)
  conv(blob, L.p1, w.xm, w.u0, M, T, false, 0, nullptr, st);
  MidArgs ma;
  ma.u0 = w.u0; ma.bias = blob + L.p1.b; ma.slope = blob + L.slope; ma.offset = blob + L.offset;
  ma.gamma = blob + L.pn1.g; ma.beta = blob + L.pn1.b; ma.dur = dur; ma.lengths = lengths; ma.out = w.v;
  ma.M = M; ma.T = T; ma.F = F; ma.n_dur = n_dur; ma.v2 = v2;
  launch_rows(durdisc_mid_kernel<1>, durdisc_mid_kernel<2>, durdisc_mid_kernel<4>, ma, M, F, st);
  conv(blob, L.p2, w.v, w.w, n_dur * M, T, true, v2, nullptr, st);
  OutArgs oa;
  oa.u = w.w; oa.gamma = blob + L.pn2.g; oa.beta = blob + L.pn2.b; oa.w = blob + L.ow; oa.b = blob + L.ob; oa.lengths = lengths;
  oa.prob = prob_out; oa.logit = logit_out;
  oa.rows = n_dur * M; oa.M = M; oa.T = T; oa.F = F; oa.v2 = v2;
  launch_rows(durdisc_out_kernel<1>, durdisc_out_kernel<2>, durdisc_out_kernel<4>, oa, n_dur * M, F, st);
  return record_hip_error(h, "durdisc prob");
}

}  // extern "C"
