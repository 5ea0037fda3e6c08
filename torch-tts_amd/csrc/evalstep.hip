// The glue of the VITS2 validation step (include/ttsdec.h ttsvits_kl_loss / ttsvits_slice_segments / ttsvits_sliced_l1): what
// SynthesizerTrn.forward and train.py:357-418 do between the encoders, the generator and the loss terms - the prior expanded along
// the alignment (models.py:1270-1271), losses.kl_loss (losses.py:37-46), commons.slice_segments (commons.py:50-56) and the mel L1.
//
//   kl_frames_kernel   one wave per frame of the channel-last z_p / logs_q: the frame's token row of m_p / logs_p is gathered
//                      through frame_token (16-byte loads, lane l takes channels 4 l + 256 i), written out only when the caller
//                      wants the expanded prior, and the frame's sum of logs_p - logs_q - 0.5 + 0.5 (z_p - m_p)^2 exp(-2 logs_p)
//                      goes to the workspace.  One pass over the four operands.
//   kl_rows_kernel     one workgroup per utterance: the frame sums below t_y[b], thread i taking frames i + 256 j in order.
//   kl_total_kernel    one wave: the utterances' sums in order, and the reference's divisor sum(t_y).
//   slice_kernel<V>    out[b, o, t, i] = x[b, o, ids[b] * scale + t, i]: within an (utterance, o) the seg * inner elements are
//                      contiguous on both sides; V = 4 floats where inner is a multiple of 4 (every address is then 16-byte
//                      aligned), else one float - with inner = 1 the start is an arbitrary element offset.
//   l1_rows_kernel     one workgroup per utterance: sum |a[b, c, ids[b] + t] - y[b, c, t]| over its C * seg elements, thread i
//                      taking elements i + 256 j in order (scalar loads: the start is an arbitrary element offset).
//   l1_total_kernel    one wave: the utterances' sums in order, and the mean.
// Every sum has a fixed order that depends on C, seg and the utterance's own t_y only: no atomics in a reduction (the status
// flag alone is an atomicOr), an utterance's sum is bit for bit what it gets alone, and a call repeats bit for bit.
#include <math.h>
#include <stdint.h>

#include "kernels.h"
#include "layout.h"

using namespace ttsdec;

namespace {
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr size_t kMaxCount = (size_t)INT32_MAX - kThreads;  // frames / elements a launch indexes with an int, its last workgroup's overshoot included
enum { FLAG_START = 1 };  // status word: some ids[b] * scale < 0 or > T - seg

typedef float f32x4v __attribute__((ext_vector_type(4)));

inline HandleBase* base(ttsvits_handle* h) { return reinterpret_cast<HandleBase*>(h); }

__device__ inline int clamp_len(int t, int T) { return t < 0 ? 0 : (t > T ? T : t); }

// the workgroup's sum of v, thread order fixed: each wave's lanes, then the kWaves wave sums in order (valid in thread 0)
__device__ inline float block_sum(float v, float* sh) {
  const float w = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
  __syncthreads();
  float s = sh[0];
#pragma unroll
  for (int i = 1; i < kWaves; ++i) s += sh[i];
  return s;
}

// ------------------------------------------------------------------------------------------------------------------------
// KL: grid ceil(B * T_y / 4), 256 threads = 4 waves, one frame each
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void kl_frames_kernel(const float* __restrict__ z_p, const float* __restrict__ logs_q,
                                                            const float* __restrict__ m_p, const float* __restrict__ logs_p,
                                                            const int* __restrict__ frame_token, const int* __restrict__ t_ys, int Ty, int Tx,
                                                            int C, int n_frames, float* __restrict__ m_exp, float* __restrict__ logs_exp,
                                                            float* __restrict__ frame_sum) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (f >= n_frames) return;  // (wave-uniform)
  const int b = f / Ty, t = f - b * Ty;
  const bool live = t < clamp_len(t_ys[b], Ty);
  const int tok = frame_token ? frame_token[f] : t;
  const bool has = tok >= 0 && tok < Tx;  // no token: the reference's one-hot row is all zeros, and so is the expanded prior
  const size_t fo = (size_t)f * C, po = ((size_t)b * Tx + (has ? tok : 0)) * C;
  float acc = 0.f;
  if (live || m_exp || logs_exp) {  // (wave-uniform)
    for (int c = lane * 4; c < C; c += 256) {
      f32x4v m = {0.f, 0.f, 0.f, 0.f}, lp = m;
      if (has) {
        m = *reinterpret_cast<const f32x4v*>(m_p + po + c);
        lp = *reinterpret_cast<const f32x4v*>(logs_p + po + c);
      }
      if (m_exp) *reinterpret_cast<f32x4v*>(m_exp + fo + c) = m;
      if (logs_exp) *reinterpret_cast<f32x4v*>(logs_exp + fo + c) = lp;
      if (live) {
        const f32x4v z = *reinterpret_cast<const f32x4v*>(z_p + fo + c);
        const f32x4v lq = *reinterpret_cast<const f32x4v*>(logs_q + fo + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = z[e] - m[e];
          acc += ((lp[e] - lq[e]) - 0.5f) + (0.5f * (d * d)) * expf(-2.f * lp[e]);
        }
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) frame_sum[f] = live ? acc : 0.f;
}

// grid B, 256 threads
__global__ __launch_bounds__(kThreads) void kl_rows_kernel(const float* __restrict__ frame_sum, const int* __restrict__ t_ys, int Ty,
                                                          float* __restrict__ kl_rows) {
  __shared__ float sh[kWaves];
  const int b = blockIdx.x;
  const int ty = clamp_len(t_ys[b], Ty);
  const float* fs = frame_sum + (size_t)b * Ty;
  float acc = 0.f;
  for (int t = threadIdx.x; t < ty; t += kThreads) acc += fs[t];
  const float s = block_sum(acc, sh);
  if (threadIdx.x == 0) kl_rows[b] = s;
}

// one wave: total[0] = sum of rows, total[1] = total[0] / n with n = sum over b of t_y[b] (t_ys given) or n_each * B
__global__ __launch_bounds__(64) void total_kernel(const float* __restrict__ rows, const int* __restrict__ t_ys, int Ty, int B, double n_each,
                                                   float* __restrict__ total) {
  __shared__ long long cnt[64];
  const int lane = threadIdx.x;
  float acc = 0.f;
  long long n = 0;
  for (int b = lane; b < B; b += 64) {
    acc += rows[b];
    if (t_ys) n += clamp_len(t_ys[b], Ty);
  }
  acc = wave_sum(acc);
  cnt[lane] = n;
  __syncthreads();
  if (lane == 0) {
    long long all = 0;
    for (int i = 0; i < 64; ++i) all += cnt[i];
    total[0] = acc;
    total[1] = acc / (t_ys ? (float)all : (float)(n_each * (double)B));
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// slices
// ------------------------------------------------------------------------------------------------------------------------
// the start of utterance b's slice in frames of x, or -1 when it lies outside [0, T - seg]
__device__ inline long long slice_start(const void* ids, int ids_int64, int b, int scale, int T, int seg) {
  if (!ids) return 0;
  const long long id = ids_int64 ? static_cast<const long long*>(ids)[b] : (long long)static_cast<const int*>(ids)[b];
  if (id < 0 || id > (long long)(T - seg)) return -1;  // (before the product: no overflow)
  const long long s = id * scale;
  return s > (long long)(T - seg) ? -1 : s;
}

// grid (ceil(outer * seg * inner / V / 256), B); V: floats per element of the copy
template <typename V>
__global__ __launch_bounds__(kThreads) void slice_kernel(const float* __restrict__ x, const void* __restrict__ ids, int ids_int64, int outer, int T,
                                                        int inner, int seg, int scale, float* __restrict__ out, int* __restrict__ status) {
  constexpr int kV = sizeof(V) / sizeof(float);
  const int b = blockIdx.y;
  const long long start = slice_start(ids, ids_int64, b, scale, T, seg);
  const int run = seg * inner / kV;  // elements of one (utterance, o): contiguous in x and in out
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0 && start < 0) atomicOr(status, FLAG_START);
  if (i >= outer * run) return;
  const int o = i / run, r = i - o * run;
  const size_t row = (size_t)b * outer + o;
  V v;
  if (start >= 0) {
    v = reinterpret_cast<const V*>(x + (row * T + (size_t)start) * inner)[r];
  } else {
    v = V{};
  }
  reinterpret_cast<V*>(out + row * seg * inner)[r] = v;
}

// grid B, 256 threads
__global__ __launch_bounds__(kThreads) void l1_rows_kernel(const float* __restrict__ a, const float* __restrict__ y, const void* __restrict__ ids,
                                                          int ids_int64, int C, int Ta, int seg, float* __restrict__ l1_rows,
                                                          int* __restrict__ status) {
  __shared__ float sh[kWaves];
  const int b = blockIdx.x;
  const long long start = slice_start(ids, ids_int64, b, 1, Ta, seg);
  if (threadIdx.x == 0 && start < 0) atomicOr(status, FLAG_START);
  const float* ab = a + (size_t)b * C * Ta + (start < 0 ? 0 : (size_t)start);
  const float* yb = y + (size_t)b * C * seg;
  const int n = C * seg;
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const int c = i / seg, t = i - c * seg;
    const float av = start < 0 ? 0.f : ab[(size_t)c * Ta + t];
    acc += fabsf(av - yb[i]);
  }
  const float s = block_sum(acc, sh);
  if (threadIdx.x == 0) l1_rows[b] = s;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_kl_sizes(const ttsvits_handle* h, int B, int Ty, int Tx, int C) {
  if (!h || B <= 0 || Ty <= 0 || Tx <= 0 || C <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (C < 4 || (C & 3) || C > 4096 || B > 65535 || (size_t)B * Ty > kMaxCount || (size_t)B * Tx > kMaxCount) return TTSDEC_ERR_DIMS;
  return TTSDEC_OK;
}

}  // namespace

extern "C" {

size_t ttsvits_kl_loss_workspace_bytes(const ttsvits_handle* h, int B, int T_y) {
  if (!h || B <= 0 || T_y <= 0 || B > 65535 || (size_t)B * T_y > kMaxCount) return 0;
  Carver cv{nullptr};
  cv.take((size_t)B * T_y);
  return cv.bytes();
}

int ttsvits_kl_loss(ttsvits_handle* h, const float* z_p, const float* logs_q, const float* m_p, const float* logs_p, const int32_t* frame_token,
                    const int32_t* t_y, int B, int T_y, int T_x, int C, float* m_p_exp, float* logs_p_exp, float* kl_rows, float* kl,
                    void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_kl_sizes(h, B, T_y, T_x, C);
  if (rc != TTSDEC_OK) return rc;
  if (!z_p || !logs_q || !m_p || !logs_p || !t_y || !kl_rows || !kl) return TTSDEC_ERR_INVALID_ARG;
  if (!frame_token && T_x != T_y) return TTSDEC_ERR_INVALID_ARG;  // the identity form: the prior is per frame
  if (!aligned16(z_p) || !aligned16(logs_q) || !aligned16(m_p) || !aligned16(logs_p) || !aligned16(m_p_exp) || !aligned16(logs_p_exp))
    return TTSDEC_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < ttsvits_kl_loss_workspace_bytes(h, B, T_y) || (reinterpret_cast<uintptr_t>(workspace) & 255))
    return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* frame_sum = static_cast<float*>(workspace);
  const int n_frames = B * T_y;
  hipLaunchKernelGGL(kl_frames_kernel, dim3((unsigned)((n_frames + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, z_p, logs_q, m_p, logs_p, frame_token,
                     t_y, T_y, T_x, C, n_frames, m_p_exp, logs_p_exp, frame_sum);
  hipLaunchKernelGGL(kl_rows_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, frame_sum, t_y, T_y, kl_rows);
  hipLaunchKernelGGL(total_kernel, dim3(1), dim3(64), 0, st, kl_rows, t_y, T_y, B, 0.0, kl);
  return record_hip_error(base(h), "kl_loss");
}

int ttsvits_slice_segments(ttsvits_handle* h, const float* x, const void* ids, int ids_int64, int B, int outer, int T, int inner, int seg, int scale,
                           float* out, int32_t* status, void* stream) {
  if (!h || B <= 0 || outer <= 0 || T <= 0 || inner <= 0 || seg <= 0 || scale <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (seg > T || B > 65535 || (size_t)B * outer * T * inner > (size_t)1 << 31 || (size_t)outer * seg * inner > kMaxCount) return TTSDEC_ERR_DIMS;
  if (!x || !ids || !out || !status) return TTSDEC_ERR_INVALID_ARG;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
  if (e != hipSuccess) return hip_fail(base(h), e, "slice_segments");
  // 16-byte elements only where every address is a multiple of 16 bytes: inner a multiple of 4 floats and both bases aligned
  const bool vec = !(inner & 3) && aligned16(x) && aligned16(out);
  const size_t n = (size_t)outer * seg * inner / (vec ? 4 : 1);
  const dim3 grid((unsigned)((n + kThreads - 1) / kThreads), (unsigned)B);
  if (vec)
    hipLaunchKernelGGL(slice_kernel<f32x4v>, grid, dim3(kThreads), 0, st, x, ids, ids_int64, outer, T, inner, seg, scale, out, status);
  else
    hipLaunchKernelGGL(slice_kernel<float>, grid, dim3(kThreads), 0, st, x, ids, ids_int64, outer, T, inner, seg, scale, out, status);
  return record_hip_error(base(h), "slice_segments");
}

int ttsvits_sliced_l1(ttsvits_handle* h, const float* a, const float* y, const void* ids, int ids_int64, int B, int C, int T_a, int seg,
                      float* l1_rows, float* l1, int32_t* status, void* stream) {
  if (!h || B <= 0 || C <= 0 || T_a <= 0 || seg <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (seg > T_a || B > 65535 || (size_t)B * C * T_a > (size_t)1 << 31 || (size_t)C * seg > kMaxCount) return TTSDEC_ERR_DIMS;
  if (!a || !y || !l1_rows || !l1 || !status) return TTSDEC_ERR_INVALID_ARG;
  if (!ids && seg != T_a) return TTSDEC_ERR_INVALID_ARG;  // the plain form: two tensors of one shape
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
  if (e != hipSuccess) return hip_fail(base(h), e, "sliced_l1");
  hipLaunchKernelGGL(l1_rows_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, a, y, ids, ids_int64, C, T_a, seg, l1_rows, status);
  hipLaunchKernelGGL(total_kernel, dim3(1), dim3(64), 0, st, l1_rows, static_cast<const int*>(nullptr), 0, B, (double)C * (double)seg, l1);
  return record_hip_error(base(h), "sliced_l1");
}

}  // extern "C"
