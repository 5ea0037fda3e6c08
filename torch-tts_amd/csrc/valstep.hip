// The loss terms of the Tacotron validation step (include/ttsdec.h ttsdec_val_losses / ttsdec_mel_loss): what run_training_step
// (tacotron/tacotron.py:100-138) and TacotronTask.train_forward (tacotron/tacotron_lightning.py:50-99) compute from the forward's
// y, y_post, s and w - mel_loss_fn with and without a mask on the frames and on their differences, the pos_weight BCE on the stop
// logits, alignment_std_loss and alignment_max_loss - in one pass over each operand, from lengths instead of a mask tensor.
//
//   frames_kernel<TERM, DIFF, VEC, NI>  a workgroup owns kFrameRun consecutive frames of one utterance, each of its 4 waves
//                      kWaveRun of them plus the frame that follows its run (the halo).  A frame's D channels are spread over
//                      the wave - lane l holds channels 4 l + 256 i + e, e < 4, i < NI, as one 16-byte load where D is a
//                      multiple of 4 and the bases are aligned (VEC), as four 4-byte loads otherwise: the same map, so the same
//                      sums - and frame t + 1 stays in registers as the next iteration's frame t: each operand is read once by
//                      its wave (the halo twice).  Per frame: the sum over channels of TERM(y, x) (and of y_post), and with DIFF
//                      of |(y[t+1] - y[t]) - (x[t+1] - x[t])|, to the workspace.
//   wrows_kernel       one wave per row of L attention weights, lane l taking weights l + 64 j: S0 = sum w, m1 = sum w l,
//                      max w, then (second read, from cache) q = sum w (l - m1)^2; var = q + m1^2 (1 - S0) - the reference's
//                      sum w l^2 - (sum w l)^2 without its cancellation - clipped at 0, and 1 - max, to the workspace.
//   rows_kernel        one workgroup per utterance: the frame sums below len_b (A), below T - 1 (Dall), below len_b - 1 (Dmsk),
//                      the stop BCE of its T logits, and its steps' variances and 1 - max; thread i takes frames i + 256 j.
//   terms_kernel / mel_total_kernel   one wave: the utterances' sums in order, the divisors, the terms.
// Every sum has a fixed order that depends on D, T, S, L and the utterance's own length only: no atomics, an utterance's row is
// bit for bit what it gets alone, and a call repeats bit for bit.  Enqueue only.
#include <math.h>
#include <stdint.h>

#include "kernels.h"
#include "layout.h"

using namespace ttsdec;

namespace {
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kFrameRun = TTSDEC_VAL_FRAME_RUN;  // frames of a workgroup
constexpr int kWaveRun = kFrameRun / kWaves;     // frames of a wave
constexpr int kRowTerms = 9;                     // rows [B, 9]
enum { ROW_A_Y, ROW_A_P, ROW_DALL_Y, ROW_DALL_P, ROW_DMSK_Y, ROW_DMSK_P, ROW_BCE, ROW_V, ROW_M };
enum { TERM_VOL = 0, TERM_L1 = 1, TERM_SQ = 2 };  // mel_loss_fn's order

typedef float f32x4v __attribute__((ext_vector_type(4)));

inline HandleBase* base(ttsdec_handle* h) { return reinterpret_cast<HandleBase*>(h); }

__device__ inline int clamp_len(int t, int T) { return t < 0 ? 0 : (t > T ? T : t); }
__device__ inline int len_of(const int* lengths, int b, int T) { return lengths ? clamp_len(lengths[b], T) : T; }

// ------------------------------------------------------------------------------------------------------------------------
// frames
// ------------------------------------------------------------------------------------------------------------------------
template <int NI>
struct Frame {
  float v[NI][4];  // channel 4 lane + 256 i + e; 0 beyond D
};

template <bool VEC, int NI>
__device__ __forceinline__ void load_frame(Frame<NI>& f, const float* __restrict__ p, int D, int lane) {
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int c = 4 * lane + 256 * i;
    if constexpr (VEC) {
      f32x4v q = {0.f, 0.f, 0.f, 0.f};
      if (c < D) q = *reinterpret_cast<const f32x4v*>(p + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) f.v[i][e] = q[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) f.v[i][e] = c + e < D ? p[c + e] : 0.f;
    }
  }
}

// the frame's sum over channels of mel_loss_fn's element term (tacotron.py:60-71); vol: clip(mean_d x, 0.1) of the frame (order 0)
template <int TERM, int NI>
__device__ __forceinline__ float term_sum(const Frame<NI>& y, const Frame<NI>& x, float vol) {
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = y.v[i][e] - x.v[i][e];
      if constexpr (TERM == TERM_VOL)
        acc += d > 0.f ? vol * d : -d;
      else if constexpr (TERM == TERM_L1)
        acc += fabsf(d);
      else
        acc += d * d;
    }
  }
  return wave_sum(acc);
}

template <int NI>
__device__ __forceinline__ float diff_sum(const Frame<NI>& y0, const Frame<NI>& y1, const Frame<NI>& x0, const Frame<NI>& x1) {
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += fabsf((y1.v[i][e] - y0.v[i][e]) - (x1.v[i][e] - x0.v[i][e]));
  }
  return wave_sum(acc);
}

template <int NI>
__device__ __forceinline__ float frame_vol(const Frame<NI>& x, int D) {
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += x.v[i][e];
  }
  return fmaxf(wave_sum(acc) / (float)D, 0.1f);
}

struct ValFrameArgs {
  const float *y, *yp, *x;  // yp may be NULL
  size_t x_stride;          // floats from one utterance of x to the next (T_x * D)
  int T, D;
  float *a_y, *a_p, *d_y, *d_p;  // [B * T] each; a_p / d_p unused without yp, d_* without DIFF
};

// grid (ceil(T / kFrameRun), B), 256 threads
template <int TERM, bool DIFF, bool VEC, int NI>
__global__ __launch_bounds__(kThreads) void frames_kernel(ValFrameArgs g) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int t0 = blockIdx.x * kFrameRun + (threadIdx.x >> 6) * kWaveRun;
  if (t0 >= g.T) return;  // (wave-uniform; no barrier in this kernel)
  const int t1 = t0 + kWaveRun < g.T ? t0 + kWaveRun : g.T;
  const size_t yo = (size_t)b * g.T * g.D, xo = (size_t)b * g.x_stride;
  const bool post = g.yp != nullptr;
  Frame<NI> y, p, x, yn, pn, xn;
  load_frame<VEC, NI>(y, g.y + yo + (size_t)t0 * g.D, g.D, lane);
  load_frame<VEC, NI>(x, g.x + xo + (size_t)t0 * g.D, g.D, lane);
  if (post) load_frame<VEC, NI>(p, g.yp + yo + (size_t)t0 * g.D, g.D, lane);
  for (int t = t0; t < t1; ++t) {
    const bool more = t + 1 < (DIFF ? g.T : t1);  // with DIFF the wave's last frame still needs the one behind it: the halo
    if (more) {
      load_frame<VEC, NI>(yn, g.y + yo + (size_t)(t + 1) * g.D, g.D, lane);
      load_frame<VEC, NI>(xn, g.x + xo + (size_t)(t + 1) * g.D, g.D, lane);
      if (post) load_frame<VEC, NI>(pn, g.yp + yo + (size_t)(t + 1) * g.D, g.D, lane);
    }
    const float vol = TERM == TERM_VOL ? frame_vol<NI>(x, g.D) : 0.f;
    const float ay = term_sum<TERM, NI>(y, x, vol);
    const float ap = post ? term_sum<TERM, NI>(p, x, vol) : 0.f;
    float dy = 0.f, dp = 0.f;
    if (DIFF && more) {
      dy = diff_sum<NI>(y, yn, x, xn);
      if (post) dp = diff_sum<NI>(p, pn, x, xn);
    }
    if (lane == 0) {
      const size_t f = (size_t)b * g.T + t;
      g.a_y[f] = ay;
      if (post) g.a_p[f] = ap;
      if (DIFF) {
        g.d_y[f] = dy;
        if (post) g.d_p[f] = dp;
      }
    }
    if (more) {
      y = yn;
      x = xn;
      if (post) p = pn;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// alignment rows: grid ceil(n_rows / 4), 256 threads = 4 waves, one row of L weights each
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void wrows_kernel(const float* __restrict__ w, int n_rows, int L, float* __restrict__ var_out,
                                                        float* __restrict__ max_out) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= n_rows) return;  // (wave-uniform)
  const float* row = w + (size_t)r * L;
  float s0 = 0.f, m1 = 0.f, mx = -INFINITY;
  for (int l = lane; l < L; l += 64) {
    const float v = row[l];
    s0 += v;
    m1 += v * (float)l;
    mx = fmaxf(mx, v);
  }
  s0 = wave_sum(s0);
  m1 = wave_sum(m1);
  mx = wave_max(mx);
  float q = 0.f;
  for (int l = lane; l < L; l += 64) {
    const float d = (float)l - m1;
    q += row[l] * (d * d);
  }
  q = wave_sum(q);
  if (lane == 0) {
    const float var = q + (m1 * m1) * (1.f - s0);
    var_out[r] = var < 0.f ? 0.f : var;  // torch.clip(min = 0): a NaN goes through, as there
    max_out[r] = 1.f - mx;
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// per utterance: grid B, 256 threads.  n_out = 9: the row of ttsdec_val_losses; 1: a_y alone (ttsdec_mel_loss)
// ------------------------------------------------------------------------------------------------------------------------
struct ValRowArgs {
  const float *a_y, *a_p, *d_y, *d_p;  // frame sums [B * T]; NULL: the term is zero
  const float* s;                      // stop logits [B * T] or NULL
  const float *var, *one_minus_max;    // [B * S] or NULL
  const int* lengths;                  // or NULL: every utterance has T frames
  int T, S, n_out;
  float pos_weight;
  float* rows;
};

__global__ __launch_bounds__(kThreads) void rows_kernel(ValRowArgs g) {
  __shared__ float sh[kWaves][kRowTerms];
  const int b = blockIdx.x, T = g.T;
  const int len = len_of(g.lengths, b, T);
  const size_t fo = (size_t)b * T;
  float acc[kRowTerms];
#pragma unroll
  for (int k = 0; k < kRowTerms; ++k) acc[k] = 0.f;
  for (int t = threadIdx.x; t < T; t += kThreads) {
    if (t < len) {
      if (g.a_y) acc[ROW_A_Y] += g.a_y[fo + t];
      if (g.a_p) acc[ROW_A_P] += g.a_p[fo + t];
    }
    if (t < T - 1) {
      if (g.d_y) acc[ROW_DALL_Y] += g.d_y[fo + t];
      if (g.d_p) acc[ROW_DALL_P] += g.d_p[fo + t];
      if (t + 1 < len) {
        if (g.d_y) acc[ROW_DMSK_Y] += g.d_y[fo + t];
        if (g.d_p) acc[ROW_DMSK_P] += g.d_p[fo + t];
      }
    }
    if (g.s) {  // binary_cross_entropy_with_logits(s, z, pos_weight) in its stable form
      const float s = g.s[fo + t], z = t < len ? 1.f : 0.f;
      const float sp = log1pf(expf(-fabsf(s))) + fmaxf(-s, 0.f);
      acc[ROW_BCE] += (1.f - z) * s + (1.f + (g.pos_weight - 1.f) * z) * sp;
    }
  }
  if (g.var) {
    const size_t so = (size_t)b * g.S;
    for (int i = threadIdx.x; i < g.S; i += kThreads) {
      acc[ROW_V] += g.var[so + i];
      acc[ROW_M] += g.one_minus_max[so + i];
    }
  }
#pragma unroll
  for (int k = 0; k < kRowTerms; ++k) {
    const float v = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < g.n_out) {
    float v = sh[0][threadIdx.x];
#pragma unroll
    for (int i = 1; i < kWaves; ++i) v += sh[i][threadIdx.x];
    g.rows[(size_t)b * g.n_out + threadIdx.x] = v;
  }
}

// the utterances' sums of column k of rows [B, n], lane l taking utterances l + 64 j (the same value in every lane)
__device__ inline float column_sum(const float* rows, int B, int n, int k, int lane) {
  float acc = 0.f;
  for (int b = lane; b < B; b += 64) acc += rows[(size_t)b * n + k];
  return wave_sum(acc);
}

// sum over b of max(len_b - less, 0), in lane 0
__device__ inline long long count_frames(const int* lengths, int B, int T, int less, long long* cnt, int lane) {
  long long n = 0;
  for (int b = lane; b < B; b += 64) {
    const int l = len_of(lengths, b, T) - less;
    n += l > 0 ? l : 0;
  }
  __syncthreads();  // (cnt is reused)
  cnt[lane] = n;
  __syncthreads();
  long long all = 0;
  if (lane == 0)
    for (int i = 0; i < 64; ++i) all += cnt[i];
  return all;
}

// one wave.  A divisor of zero gives NaN (0 / 0), as the reference's does.
__global__ __launch_bounds__(64) void terms_kernel(const float* __restrict__ rows, const int* __restrict__ lengths, int B, int T, int D, int S,
                                                   int has_frames, int has_post, int has_stop, int has_w, float* __restrict__ terms) {
  __shared__ long long cnt[64];
  const int lane = threadIdx.x;
  float sum[kRowTerms];
#pragma unroll
  for (int k = 0; k < kRowTerms; ++k) sum[k] = column_sum(rows, B, kRowTerms, k, lane);
  const long long n = count_frames(lengths, B, T, 0, cnt, lane), n1 = count_frames(lengths, B, T, 1, cnt, lane);
  if (lane != 0) return;
  const double dn = (double)D * (double)n, dn1 = (double)D * (double)n1, dall = (double)B * (double)(T - 1) * (double)D;
  float out[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = 0.f;
  if (has_frames) {
    out[0] = (float)((double)sum[ROW_A_Y] / dn);
    out[2] = (float)((double)sum[ROW_DALL_Y] / dall);
    out[4] = (float)((double)sum[ROW_DMSK_Y] / dn1);
    if (has_post) {
      out[1] = (float)((double)sum[ROW_A_P] / dn);
      out[3] = (float)((double)sum[ROW_DALL_P] / dall);
      out[5] = (float)((double)sum[ROW_DMSK_P] / dn1);
    }
  }
  if (has_stop) out[6] = (float)((double)sum[ROW_BCE] / ((double)B * (double)T));
  if (has_w) {
    out[7] = sqrtf((float)((double)sum[ROW_V] / ((double)B * (double)S)));
    out[8] = (float)((double)sum[ROW_M] / ((double)B * (double)S));
  }
  out[9] = (float)n;
  out[10] = (float)n1;
#pragma unroll
  for (int i = 0; i < 16; ++i) terms[i] = out[i];
}

// one wave: out[0] = mel_loss_fn's value from rows [B]: sum / (D N) with lengths, / (B T D) without; order 2: its root
__global__ __launch_bounds__(64) void mel_total_kernel(const float* __restrict__ rows, const int* __restrict__ lengths, int B, int T, int D,
                                                       int order, float* __restrict__ out) {
  __shared__ long long cnt[64];
  const int lane = threadIdx.x;
  const float sum = column_sum(rows, B, 1, 0, lane);
  const long long n = count_frames(lengths, B, T, 0, cnt, lane);
  if (lane != 0) return;
  const float v = (float)((double)sum / ((double)D * (double)n));
  out[0] = order == 2 ? sqrtf(v) : v;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct Carved {
  float *a_y, *a_p, *d_y, *d_p, *var, *omm;
};
Carved carve(Carver& cv, int B, int T, int S) {
  Carved c;
  const size_t f = (size_t)B * T, r = (size_t)B * S;
  c.a_y = cv.take(f);
  c.a_p = cv.take(f);
  c.d_y = cv.take(f);
  c.d_p = cv.take(f);
  c.var = cv.take(r);
  c.omm = cv.take(r);
  return c;
}

template <int TERM, bool DIFF>
void launch_frames(const ValFrameArgs& a, int B, bool vec, hipStream_t st) {
  const dim3 grid((unsigned)((a.T + kFrameRun - 1) / kFrameRun), (unsigned)B), block(kThreads);
  const int ni = (a.D + 255) / 256;  // 1 .. 4
#define TTS_FRAMES(V, N) hipLaunchKernelGGL((frames_kernel<TERM, DIFF, V, N>), grid, block, 0, st, a)
  if (vec) {
    if (ni == 1) TTS_FRAMES(true, 1);
    else if (ni == 2) TTS_FRAMES(true, 2);
    else if (ni == 3) TTS_FRAMES(true, 3);
    else TTS_FRAMES(true, 4);
  } else {
    if (ni == 1) TTS_FRAMES(false, 1);
    else if (ni == 2) TTS_FRAMES(false, 2);
    else if (ni == 3) TTS_FRAMES(false, 3);
    else TTS_FRAMES(false, 4);
  }
#undef TTS_FRAMES
}

constexpr size_t kMaxElems = (size_t)1 << 31;

// sizes every entry point shares: TTSDEC_OK, or the refusal
int check_frame_sizes(const void* h, int B, int T, int D, int T_x) {
  if (!h || B <= 0 || T <= 0 || D <= 0 || T_x <= 0 || T_x < T) return TTSDEC_ERR_INVALID_ARG;
  if (B > 65535 || D > 1024 || (size_t)B * T_x * D > kMaxElems) return TTSDEC_ERR_DIMS;
  return TTSDEC_OK;
}

}  // namespace

extern "C" {

size_t ttsdec_val_losses_workspace_bytes(const ttsdec_handle* h, int B, int T, int S) {
  if (!h || B <= 0 || T <= 0 || S < 0 || B > 65535 || (size_t)B * T > kMaxElems || (size_t)B * S > kMaxElems) return 0;
  Carver cv{nullptr};
  carve(cv, B, T, S);
  return cv.bytes();
}

int ttsdec_val_losses(ttsdec_handle* h, const float* y, const float* y_post, const float* x, int T_x, const float* s, const float* w,
                      const int32_t* lengths, int B, int T, int D, int S, int L, float pos_weight, float* rows, float* terms, void* workspace,
                      size_t workspace_bytes, void* stream) {
  int rc = check_frame_sizes(h, B, T, D, T_x);
  if (rc != TTSDEC_OK) return rc;
  if (w && (S <= 0 || L <= 0)) return TTSDEC_ERR_INVALID_ARG;
  if (w && (size_t)B * S * L > kMaxElems) return TTSDEC_ERR_DIMS;
  if (!rows || !terms || (!y != !x) || (y_post && !y) || (!y && !s && !w)) return TTSDEC_ERR_INVALID_ARG;
  const int Sw = w ? S : 0;
  const size_t need = ttsdec_val_losses_workspace_bytes(h, B, T, Sw);
  if (!workspace || !need || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255)) return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Carver cv{static_cast<float*>(workspace)};
  const Carved c = carve(cv, B, T, Sw);
  if (y) {
    // 16-byte loads only where every frame of every operand starts on a multiple of 16 bytes
    const bool vec = !(D & 3) && aligned16(y) && aligned16(x) && aligned16(y_post);
    launch_frames<TERM_L1, true>(ValFrameArgs{y, y_post, x, (size_t)T_x * D, T, D, c.a_y, c.a_p, c.d_y, c.d_p}, B, vec, st);
  }
  if (w) {
    const int n_rows = B * S;
    hipLaunchKernelGGL(wrows_kernel, dim3((unsigned)((n_rows + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, w, n_rows, L, c.var, c.omm);
  }
  ValRowArgs r{};
  if (y) {
    r.a_y = c.a_y;
    r.d_y = c.d_y;
    if (y_post) {
      r.a_p = c.a_p;
      r.d_p = c.d_p;
    }
  }
  r.s = s;
  if (w) {
    r.var = c.var;
    r.one_minus_max = c.omm;
  }
  r.lengths = lengths;
  r.T = T;
  r.S = Sw;
  r.n_out = kRowTerms;
  r.pos_weight = pos_weight;
  r.rows = rows;
  hipLaunchKernelGGL(rows_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, r);
  hipLaunchKernelGGL(terms_kernel, dim3(1), dim3(64), 0, st, rows, lengths, B, T, D, Sw, y ? 1 : 0, y_post ? 1 : 0, s ? 1 : 0, w ? 1 : 0, terms);
  return record_hip_error(base(h), "val_losses");
}

int ttsdec_mel_loss(ttsdec_handle* h, const float* y, const float* x, int T_x, const int32_t* lengths, int B, int T, int D, int order,
                    float* rows, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_frame_sizes(h, B, T, D, T_x);
  if (rc != TTSDEC_OK) return rc;
  if (order < 0 || order > 2) return TTSDEC_ERR_INVALID_ARG;
  if (!y || !x || !rows || !out) return TTSDEC_ERR_INVALID_ARG;
  const size_t need = ttsdec_val_losses_workspace_bytes(h, B, T, 0);
  if (!workspace || !need || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255)) return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Carver cv{static_cast<float*>(workspace)};
  const Carved c = carve(cv, B, T, 0);
  const bool vec = !(D & 3) && aligned16(y) && aligned16(x);
  const ValFrameArgs a{y, nullptr, x, (size_t)T_x * D, T, D, c.a_y, nullptr, nullptr, nullptr};
  if (order == 0) launch_frames<TERM_VOL, false>(a, B, vec, st);
  else if (order == 1) launch_frames<TERM_L1, false>(a, B, vec, st);
  else launch_frames<TERM_SQ, false>(a, B, vec, st);
  ValRowArgs r{};
  r.a_y = c.a_y;
  r.lengths = lengths;
  r.T = T;
  r.n_out = 1;
  r.rows = rows;
  hipLaunchKernelGGL(rows_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, r);
  hipLaunchKernelGGL(mel_total_kernel, dim3(1), dim3(64), 0, st, rows, lengths, B, T, D, order, out);
  return record_hip_error(base(h), "mel_loss");
}

}  // extern "C"
