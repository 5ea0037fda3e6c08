// Monotonic alignment search and its cost matrix (include/ttsdec.h ttsvits_neg_cent / ttsvits_maximum_path / ttsvits_align): the
// `with torch.no_grad():` block of SynthesizerTrn.forward, vits2/models.py:1224-1254, and monotonic_align/core.pyx:7-33.
//
//   neg_cent_kernel   neg_cent[y, x] = sum_d(-0.5 z^2 s + z m s) + sum_d(-0.5 log 2pi - logs - 0.5 m^2 s), s = exp(-2 logs): one wave per
//                     32 x 32 tile, the T_y x T_x x 2C contraction in exact fp32 on v_mfma_f32_32x32x2_f32 with both operands built
//                     in registers from the channel-last z_p / m_p / logs_p (a lane's B operand is its own token column, so the
//                     per-column term is summed beside it); zeros outside an utterance's t_y x t_x.
//   mas_kernel        one utterance per single-wave workgroup.  Rows are sequential; lane l owns the CPL contiguous columns from
//                     l * CPL, so a row step needs one neighbour value (a DPP wave shift, no LDS).  value[y, x] lives in registers
//                     only: what leaves a row is one decision bit per cell (v_cur < v_prev, or x == y), a CPL-bit mask per lane.
//                     Rows of neg_cent are loaded kPrefetch rows ahead of the recurrence.  The backtrack stages kBackRows rows of
//                     masks through LDS per block and walks them with one LDS read per row; it emits frame_token and dur.
//   path_kernel       the reference's dense 0 / 1 path in the caller's dtype from frame_token, over a full grid.
// The recurrence is fp32 `+` and a compare-select in the reference's order, so the path is the reference's bit for bit.
#include <math.h>
#include <stdint.h>

#include "kernels.h"

using namespace ttsdec;

namespace {
constexpr int kWave = 64;
constexpr int kMaxTx = 1024;     // 64 lanes x 16 columns
constexpr int kPrefetch = 4;     // rows of neg_cent in flight ahead of the recurrence
constexpr int kBackRows = 128;   // rows of decision masks staged through LDS per backtrack block
constexpr float kNeg = -1e9f;    // core.pyx max_neg_val
enum { FLAG_EMPTY = 1, FLAG_SHORT = 2, FLAG_RANGE = 4 };  // status word: t < 1; t_y < t_x; a length beyond the tensor

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x16v __attribute__((ext_vector_type(16)));

// every family's handle is `struct tts*_handle : HandleBase` (single, non-virtual base: it sits at offset 0); the ttsvits one is
// complete only inside vits2.hip, and these calls use nothing but the base (device, error text)
inline HandleBase* base(ttsvits_handle* h) { return reinterpret_cast<HandleBase*>(h); }

// ------------------------------------------------------------------------------------------------------------------------
// neg_cent: grid (ceil(T_x / 32), ceil(T_y / 128), B), 256 threads = 4 waves, wave w owns rows [128 by + 32 w, + 32)
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void neg_cent_kernel(const float* __restrict__ z_p, const float* __restrict__ m_p,
                                                       const float* __restrict__ logs_p, const int* __restrict__ t_ys,
                                                       const int* __restrict__ t_xs, int Ty, int Tx, int C, float* __restrict__ out) {
  const int b = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l32 = lane & 31, half = lane >> 5;
  const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 128 + wave * 32;
  if (y0 >= Ty) return;
  int ty = t_ys ? t_ys[b] : Ty, tx = t_xs ? t_xs[b] : Tx;
  ty = ty < 0 ? 0 : (ty > Ty ? Ty : ty);
  tx = tx < 0 ? 0 : (tx > Tx ? Tx : tx);
  float* ob = out + (size_t)b * Ty * Tx;
  f32x16v acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float colterm = 0.f;
  if (y0 < ty && x0 < tx) {  // (wave-uniform)
    // operand rows, clamped into the utterance: the clamped lanes' results are not stored
    const int ya = y0 + l32 < ty ? y0 + l32 : ty - 1;
    const int xb = x0 + l32 < tx ? x0 + l32 : tx - 1;
    const float* zr = z_p + ((size_t)b * Ty + ya) * C;
    const float* mr = m_p + ((size_t)b * Tx + xb) * C;
    const float* lr = logs_p + ((size_t)b * Tx + xb) * C;
    float c1 = 0.f, c4 = 0.f;
    // 8 channels per step: half h takes d0 + 4 h + e at MFMA e (k index = half), first against s, then against m s
    for (int d0 = 0; d0 < C; d0 += 8) {
      const int d = d0 + 4 * half;
      f32x4v z = {0.f, 0.f, 0.f, 0.f}, m = z, s = z, lg = z;
      const bool live = d < C;  // (C is a multiple of 4: a half is whole or absent)
      if (live) {
        z = *reinterpret_cast<const f32x4v*>(zr + d);
        m = *reinterpret_cast<const f32x4v*>(mr + d);
        lg = *reinterpret_cast<const f32x4v*>(lr + d);
      }
      f32x4v a2, ms;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[e] = live ? expf(-2.f * lg[e]) : 0.f;
        a2[e] = -0.5f * (z[e] * z[e]);
        ms[e] = m[e] * s[e];
        if (live) {
          c1 += -0.5f * 1.8378770664093453f - lg[e];  // -0.5 log(2 pi) - logs
          c4 += -0.5f * (m[e] * m[e]) * s[e];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[e], s[e], acc, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(z[e], ms[e], acc, 0, 0, 0);
    }
    c1 += __shfl_xor(c1, 32, 64);
    c4 += __shfl_xor(c4, 32, 64);
    colterm = c1 + c4;
  }
  // C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  const int x = x0 + l32;
  if (x < Tx) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int y = y0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (y < Ty) ob[(size_t)y * Tx + x] = (y < ty && x < tx) ? acc[r] + colterm : 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// MAS: grid B, 64 threads
// ------------------------------------------------------------------------------------------------------------------------
// lane l <- lane l - 1 (lane 0 keeps `fill`): the wave-wide DPP shift of gfx9
__device__ inline float wave_shr1(float v, float fill) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}

template <int CPL> struct MaskOf { typedef uint8_t type; };
template <> struct MaskOf<16> { typedef uint16_t type; };

template <int CPL>
__global__ __launch_bounds__(kWave) void mas_kernel(const float* __restrict__ neg_cent, const int* __restrict__ t_ys,
                                                    const int* __restrict__ t_xs, int Ty, int Tx, int* __restrict__ frame_token,
                                                    int* __restrict__ dur, int* __restrict__ status, void* __restrict__ bits_ws) {
  typedef typename MaskOf<CPL>::type mask_t;
  constexpr int kRowWords = kWave * sizeof(mask_t) / 4;  // 32-bit words of one row of masks
  __shared__ uint32_t sbits[kBackRows * kRowWords];
  __shared__ int stok[kBackRows];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int ty = t_ys[b], tx = t_xs[b];
  int* ft = frame_token + (size_t)b * Ty;
  int* du = dur + (size_t)b * Tx;
  int flags = 0;
  if (ty < 1 || tx < 1) flags |= FLAG_EMPTY;
  if (ty < tx) flags |= FLAG_SHORT;
  if (ty > Ty || tx > Tx) flags |= FLAG_RANGE;
  if (flags) {  // refused (the reference would read out of bounds): no frame has a token
    if (lane == 0) atomicOr(status, flags);
    for (int y = lane; y < Ty; y += kWave) ft[y] = -1;
    for (int x = lane; x < Tx; x += kWave) du[x] = 0;
    return;
  }
  const float* nc = neg_cent + (size_t)b * Ty * Tx;
  mask_t* gb = reinterpret_cast<mask_t*>(bits_ws) + (size_t)b * Ty * kWave;
  const int c0 = lane * CPL;

  // ---- forward: value[y, x] = neg_cent[y, x] + max(value[y-1, x-1], value[y-1, x]) with the reference's edge rules.  Cells outside
  // the reference's band (x > y, x < t_x + y - t_y) are computed too: no cell inside the band reads one of them.
  float buf[kPrefetch][CPL];
  auto load_row = [&](int p, int y) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) buf[p][j] = (y < ty && c0 + j < tx) ? nc[(size_t)y * Tx + c0 + j] : 0.f;
  };
#pragma unroll
  for (int p = 0; p < kPrefetch; ++p) load_row(p, p);
  float prev[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) prev[j] = kNeg;
  for (int yb = 0; yb < ty; yb += kPrefetch) {
#pragma unroll
    for (int p = 0; p < kPrefetch; ++p) {
      const int y = yb + p;
      if (y < ty) {  // (wave-uniform)
        const float left = wave_shr1(prev[CPL - 1], y == 0 ? 0.f : kNeg);  // x == 0: v_prev = 0 at y == 0, else max_neg_val
        unsigned mask = 0;
        float cur[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
          const int x = c0 + j;
          const float v_prev = j == 0 ? left : prev[j - 1];
          const float v_cur = x == y ? kNeg : prev[j];
          cur[j] = buf[p][j] + (v_cur > v_prev ? v_cur : v_prev);
          mask |= (unsigned)(x == y || v_cur < v_prev) << j;
        }
#pragma unroll
        for (int j = 0; j < CPL; ++j) prev[j] = cur[j];
        gb[(size_t)y * kWave + lane] = (mask_t)mask;
        load_row(p, y + kPrefetch);
      }
    }
  }
  __syncthreads();  // the masks are read back by other lanes (one wave: the barrier is its memory fence)

  // ---- backtrack, top block first: index -= 1 where the cell's bit is set (core.pyx:30-33; a tie stays)
  int idx = tx - 1, last = ty - 1;  // `last`: the last frame of token idx
  const uint32_t* gw = reinterpret_cast<const uint32_t*>(gb);
  for (int y0 = ((ty - 1) / kBackRows) * kBackRows; y0 >= 0; y0 -= kBackRows) {
    const int n = ty - y0 < kBackRows ? ty - y0 : kBackRows;
    __syncthreads();
    for (int i = lane; i < n * kRowWords; i += kWave) sbits[i] = gw[(size_t)y0 * kRowWords + i];
    __syncthreads();
    const mask_t* sm = reinterpret_cast<const mask_t*>(sbits);
    for (int y = y0 + n - 1; y >= y0; --y) {
      if (lane == 0) stok[y - y0] = idx;
      const unsigned m = sm[(y - y0) * kWave + idx / CPL];
      if (idx != 0 && ((m >> (idx % CPL)) & 1u)) {
        if (lane == 0) du[idx] = last - y + 1;
        last = y - 1;
        --idx;
      }
    }
    __syncthreads();
    for (int i = lane; i < n; i += kWave) ft[y0 + i] = stok[i];
  }
  if (lane == 0) du[0] = last + 1;
  for (int y = ty + lane; y < Ty; y += kWave) ft[y] = -1;
  for (int x = tx + lane; x < Tx; x += kWave) du[x] = 0;
}

// dense path [B, T_y, T_x] = 1 at (y, frame_token[y]), else 0: grid (ceil(T_y / 16), B); V is the 0 / 1 storage type
template <typename V>
__global__ __launch_bounds__(256) void path_kernel(const int* __restrict__ frame_token, int Ty, int Tx, V one, V* __restrict__ path) {
  const int b = blockIdx.y, y0 = blockIdx.x * 16;
  const int rows = Ty - y0 < 16 ? Ty - y0 : 16;
  V* pb = path + ((size_t)b * Ty + y0) * Tx;
  const int* ft = frame_token + (size_t)b * Ty + y0;
  for (int i = threadIdx.x; i < rows * Tx; i += 256) {
    const int r = i / Tx, x = i - r * Tx;
    pb[i] = ft[r] == x ? one : (V)0;
  }
}

int cpl_of(int Tx) { return Tx <= 64 ? 1 : Tx <= 128 ? 2 : Tx <= 256 ? 4 : Tx <= 512 ? 8 : 16; }
size_t row_bytes(int Tx) { return cpl_of(Tx) == 16 ? 128 : 64; }

int check_sizes(const ttsvits_handle* h, int B, int Ty, int Tx) {
  if (!h || B <= 0 || Ty <= 0 || Tx <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (Tx > kMaxTx || B > 65535 || (size_t)B * Ty * Tx > (size_t)1 << 31) return TTSDEC_ERR_DIMS;
  return TTSDEC_OK;
}

}  // namespace

extern "C" {

size_t ttsvits_align_workspace_bytes(const ttsvits_handle* h, int B, int T_y, int T_x) {
  if (check_sizes(h, B, T_y, T_x) != TTSDEC_OK) return 0;
  return up((size_t)B * T_y * row_bytes(T_x), 256);
}

int ttsvits_neg_cent(ttsvits_handle* h, const float* z_p, const float* m_p, const float* logs_p, const int32_t* t_y, const int32_t* t_x, int B,
                    int T_y, int T_x, int C, float* neg_cent, void* stream) {
  if (!z_p || !m_p || !logs_p || !neg_cent) return TTSDEC_ERR_INVALID_ARG;
  int rc = check_sizes(h, B, T_y, T_x);
  if (rc != TTSDEC_OK) return rc;
  if (C < 4 || (C & 3) || C > 4096) return TTSDEC_ERR_DIMS;
  if ((reinterpret_cast<uintptr_t>(z_p) | reinterpret_cast<uintptr_t>(m_p) | reinterpret_cast<uintptr_t>(logs_p)) & 15) return TTSDEC_ERR_INVALID_ARG;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  const dim3 grid((unsigned)((T_x + 31) / 32), (unsigned)((T_y + 127) / 128), (unsigned)B);
  hipLaunchKernelGGL(neg_cent_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), z_p, m_p, logs_p, t_y, t_x, T_y, T_x, C, neg_cent);
  return record_hip_error(base(h), "neg_cent");
}

int ttsvits_maximum_path(ttsvits_handle* h, const float* neg_cent, const int32_t* t_y, const int32_t* t_x, int B, int T_y, int T_x, void* path,
                        int path_dtype, int32_t* frame_token, int32_t* dur, int32_t* status, void* workspace, size_t workspace_bytes,
                        void* stream) {
  if (!neg_cent || !t_y || !t_x || !frame_token || !dur || !status || !workspace) return TTSDEC_ERR_INVALID_ARG;
  if (path && (path_dtype < TTSVITS_PATH_F32 || path_dtype > TTSVITS_PATH_BF16)) return TTSDEC_ERR_INVALID_ARG;
  int rc = check_sizes(h, B, T_y, T_x);
  if (rc != TTSDEC_OK) return rc;
  if (workspace_bytes < ttsvits_align_workspace_bytes(h, B, T_y, T_x) || (reinterpret_cast<uintptr_t>(workspace) & 255)) return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(base(h)->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
  if (e != hipSuccess) return hip_fail(base(h), e, "maximum_path");
#define TTS_MAS(CPL) \
  hipLaunchKernelGGL(mas_kernel<CPL>, dim3((unsigned)B), dim3(kWave), 0, st, neg_cent, t_y, t_x, T_y, T_x, frame_token, dur, status, workspace)
  switch (cpl_of(T_x)) {
    case 1: TTS_MAS(1); break;
    case 2: TTS_MAS(2); break;
    case 4: TTS_MAS(4); break;
    case 8: TTS_MAS(8); break;
    default: TTS_MAS(16); break;
  }
#undef TTS_MAS
  if (path) {
    const dim3 grid((unsigned)((T_y + 15) / 16), (unsigned)B);
    if (path_dtype == TTSVITS_PATH_F32)
      hipLaunchKernelGGL(path_kernel<float>, grid, dim3(256), 0, st, frame_token, T_y, T_x, 1.f, static_cast<float*>(path));
    else  // 1.0 as fp16 / bf16 bits
      hipLaunchKernelGGL(path_kernel<uint16_t>, grid, dim3(256), 0, st, frame_token, T_y, T_x,
                         (uint16_t)(path_dtype == TTSVITS_PATH_F16 ? 0x3C00 : 0x3F80), static_cast<uint16_t*>(path));
  }
  return record_hip_error(base(h), "maximum_path");
}

int ttsvits_align(ttsvits_handle* h, const float* z_p, const float* m_p, const float* logs_p, const int32_t* t_y, const int32_t* t_x, int B, int T_y,
                 int T_x, int C, float* neg_cent, void* path, int path_dtype, int32_t* frame_token, int32_t* dur, int32_t* status,
                 void* workspace, size_t workspace_bytes, void* stream) {
  if (!t_y || !t_x) return TTSDEC_ERR_INVALID_ARG;
  const int rc = ttsvits_neg_cent(h, z_p, m_p, logs_p, t_y, t_x, B, T_y, T_x, C, neg_cent, stream);
  if (rc != TTSDEC_OK) return rc;
  return ttsvits_maximum_path(h, neg_cent, t_y, t_x, B, T_y, T_x, path, path_dtype, frame_token, dur, status, workspace, workspace_bytes, stream);
}

}  // extern "C"
