// Two-role launches of the decode step.
//
// The step is a serial chain  frame -> lstm_att -> query -> attention -> lstm_dec -> proj  in which the
// two LSTMs are bound by what a CU can take in per microsecond and the other four launches by latency:
// 25-30 us per step in which most of the chip idles.  But most of an LSTM's K axis does not depend on the
// launch just before it (tacotron/decoder_cell.py:187,191):
//     lstm_att(t) = [ x_pre(t) | ctx(t-1) | h_att(t-1) ]      only x_pre waits for the frame kernel
//     lstm_dec(t) = [ h_att(t) | ctx(t)   | h_dec(t-1) ]      only ctx waits for the attention kernel
// So each LSTM shares a launch with the latency-bound kernel in front of it:
//     [frame || lstm_att] -> query -> [attention || lstm_dec] -> proj            (4 launches instead of 6)
// Workgroups [0, n_a) of such a launch run role A (the producer), the rest the LSTM, which walks its K axis
// with the dependent segment LAST and, right before the first tile of that segment, waits for role A's
// arrival counter (common.h role_signal / role_poll: every handed-off byte stored write-through and drained, one lane's
// agent-scope counter add; the consumer's sc1 poll, then sc1 loads - MI355X_MICROARCH.md "Hand-offs measured with sc1 loads
// in place of the acquire", row 1).  Role A has the lowest block ids and waits for nothing, so under the
// observed in-order dispatch it is resident or done before any LSTM workgroup spins; nothing DEPENDS on that order: the spin
// is bounded (~1-4 ms, once per call), a timed-out call is flagged and repeated with one role per launch.  Normally nobody
// waits long: the early segments take about as long as role A.
// What makes it pay is co-residency: the LSTM runs on the "lean" GEMM tile (gemm_tile.h: 64-80 KiB of LDS,
// <= 128 VGPRs), so a CU holds one workgroup of each role and the LSTM's tile stream fills the issue slots
// and memory queues the small kernel leaves empty.
// Measured alternatives: the same overlap as two STREAMS (round 1: slower - cross-stream graph
// edges, one 128-KiB workgroup per CU); the early segments as a separate partial-sum launch beside role A plus
// a "late" launch (round 2: 86.4 vs 88.3 us per step - the extra launch costs what the overlap wins).
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <utility>

#include "frame_body.h"
#include "step_bodies.h"

namespace ttsdec {

// The LSTM role's tiles, per arithmetic mode (PREC_F16S / PREC_F32):
//   Lean64x16: 64 rows x 16 units, 16-KiB stages x 5 = 80 KiB (split-fp16: 32 k per stage on chunked planes; exact fp32:
//              32 k per stage, 128-byte rows).  Two workgroups per CU.
//   Lean64x8:  batches of <= 64 utterances.  Split-fp16: 64 rows x 8 units on two MFMA waves (12-KiB stages x 5), so the weight
//              stream is spread over 128 workgroups instead of 64; rows past the batch read nothing (zeros).  Exact fp32
//              (round 4): 32 rows x 8 units, the tile's K split over all FOUR MFMA waves (64-byte slices, 16-KiB stages of
//              64 k x 5) - 2 x 128 = 256 workgroups at 64 utterances, every matrix pipe of the chip busy.  The 64-row fp32 form
//              (two MFMA waves on 128 workgroups: a quarter of the chip's fp32 matrix rate) is why round 3 had to switch the
//              two-role launches off for exact fp32 between 32 and 192 utterances.
//   SmallFat:  batches of <= 32 utterances: both roles together are fewer workgroups than the chip has CUs, so nothing
//              has to share a CU and the LSTM keeps the stand-alone small-batch tile (128 KiB of LDS, three tiles in
//              flight - a batch-1 LSTM is a pure weight stream and lives on bytes in flight; the lean tiles' 48 KiB
//              took 16.4 us for the attention LSTM at B = 1 against 10.9 us).
template <int PREC>
struct LeanTiles;
template <>
struct LeanTiles<PREC_F16S> {
  using Lean64x16 = TileCfg<2, 2, 1, 5, PREC_F16S, 0, 1, 1, 1>;
  using Lean64x8 = TileCfg<2, 1, 1, 5, PREC_F16S, 0, 1, 1, 1>;
  using SmallFat = TileCfg<1, 1, 2, 4, PREC_F16S>;
};
template <>
struct LeanTiles<PREC_F32> {
  using Lean64x16 = TileCfg<2, 2, 1, 5, PREC_F32>;
  using Lean64x8 = TileCfg<1, 1, 4, 5, PREC_F32, 0, 1, 1, 1>;
  using SmallFat = TileCfg<1, 1, 4, 4, PREC_F32>;
};
// exact fp32: the 32-row tile (every matrix pipe busy from 33 utterances up) while its workgroups - 128 per 32 rows - still fit the
// chip beside the producer role's: us per step at levels 0 / 1 / 2 with it, B = 80 96.3 / 79.4 / 65.4, B = 96 84.8 / 74.4 / 66.5, B = 128
// 86.2 / 84.7 / 88.2 - against the 64-row tile's B = 80 96.3 / 86.8 / 90.7, 96 85.5 / 81.3 / 90.7, 112 86.0 / 81.5 / 91.2, 128 84.8 / 79.4 / 88.0
// (gpurun sessions r4k / r4l)
constexpr int kLean8MaxRowsF32 = 96;
constexpr int kLean8MaxRows = 64;  // (measured with 128: B = 128 56.6 against 49.3 us per step, B = 96 53.6 / 48.1 - profiles/r03_w)
constexpr int kSmallFatMaxRows = 32;
static_assert(LeanTiles<PREC_F16S>::Lean64x16::kLdsBytes <= 80 * 1024 && LeanTiles<PREC_F32>::Lean64x16::kLdsBytes <= 80 * 1024 &&
                  LeanTiles<PREC_F16S>::Lean64x8::kLdsBytes <= 80 * 1024 && LeanTiles<PREC_F32>::Lean64x8::kLdsBytes <= 80 * 1024,
              "lean tiles: two workgroups per CU");

template <int A, int B>
constexpr int cmax() { return A > B ? A : B; }

// ---- role A = frame kernel (finish proj(t-1), PreNet), role B = early part of the attention LSTM ----
// WPE: waves per SIMD the register budget must allow (4 = two 512-thread workgroups per CU, 2 = one)
// kHead: the launch starts with the previous step's mel/stop projection as a third role, [proj(t-1) | frame | lstm_att] by
// block id.  Every role waits only for roles with LOWER ids and the grid dispatches in id order, so whatever a workgroup
// waits for is resident or done.  The frame role has slack for it at large batches (it ends at 10.8 us where the LSTM
// reaches its gate at 14.2, B = 256): the projection's 5.8-us launch disappears from the step.
template <int K0H, int PH, class Cfg, int WPE, bool kHead>
__global__ __launch_bounds__(kGemmThreads, WPE) void frame_lstm_kernel(FrameArgs f, LstmArgs l, ProjArgs pj, int n_proj, int n_frame, int frame_cols,
                                                                       int lstm_cols) {
  constexpr int PREC = Cfg::kPrec;
  __shared__ __attribute__((aligned(16))) float smem[cmax<cmax<Cfg::kLdsFloats, FrameLds<K0H, PH, PREC>::kFloats>(), kHead ? kProjLdsFloats : 1>()];
  loop_stamp(f.ctrl, f.slot, f.node);
  int id = blockIdx.x;
  if constexpr (kHead) {
    if (id < n_proj) {
      __builtin_amdgcn_s_setprio(3);
      proj_body<PREC>(pj, smem, id);
      return;
    }
    id -= n_proj;
  }
  // (Measured and dropped, profiles/r03_y: the frame role LAST in the grid, so that its workgroups draw the first-dispatched
  // LSTM workgroups as CU partners, and the frame role at normal wave priority - the 32 LSTM workgroups that share a CU with a
  // frame workgroup stay the launch's tail either way: they reach their gate ~6 us after the others, 2.5 us after x_pre is there.)
  if (id < n_frame) {
    __builtin_amdgcn_s_setprio(3);  // the producer role is the launch's critical path: it wins issue arbitration
    frame_body<K0H, PH, PREC, 6, WPE == 4, kHead>(f, smem, id % frame_cols, id / frame_cols);
  } else {
    const int j = id - n_frame;
    lstm_body<Cfg, true, true>(l, smem, j % lstm_cols, j / lstm_cols);
  }
}

// ---- role A = attention + context, role B = early part of the decoder LSTM ----
// Query role: the attention role's workgroups first compute the attention query GEMM between them (AttnArgs::q_tiles tiles
// of proj_body, workgroup b the tiles b, b + B, ...), each signalling its tile's 32-row block; an attention pass starts once
// the tiles of its utterance's row block are in.  The step loses the query launch (~6.5 us) and gains a hop inside this one,
// on a role that has slack: the decoder LSTM reaches its gate at ~22 us, the attention pass used to end at ~15.
// All attention-role workgroups must be resident together for this (they have the lowest block ids; B <= the chip's two
// workgroups per CU): the host only asks for it then.
// kVar: the attention pass's form (step_bodies.h AttnVariant), or ATTN_PRIO_SWAP (measurement: the base pass at wave priority 0,
// the decoder LSTM at 3).
constexpr int ATTN_PRIO_SWAP = 4;
template <int NJ, class Cfg, int WPE, int kVar = ATTN_BASE>
__global__ __launch_bounds__(kGemmThreads, WPE) void attn_lstm_kernel(AttnArgs a, LstmArgs l, ProjArgs pq, int n_attn, int lstm_cols) {
  __shared__ __attribute__((aligned(16))) float smem[cmax<cmax<Cfg::kLdsFloats, attn_lds_floats<NJ>()>(), kProjLdsFloats>()];
  loop_stamp(a.ctrl, a.slot, a.node);
  const int id = blockIdx.x;
  if (id < n_attn) {
    if constexpr (kVar != ATTN_PRIO_SWAP) __builtin_amdgcn_s_setprio(3);  // (as above: the decoder LSTM's last segment waits for every one of these)
    if (a.q_tiles > 0) {
      for (int tile = id; tile < a.q_tiles; tile += n_attn) {
        proj_body<Cfg::kPrec>(pq, smem, tile);
        __syncthreads();  // (the reduction tile in LDS is reused by the next tile / the attention pass)
      }
    }
    attn_body<NJ, kVar == ATTN_PRIO_SWAP ? ATTN_BASE : kVar>(a, smem, id);
  } else {
    if constexpr (kVar == ATTN_PRIO_SWAP) __builtin_amdgcn_s_setprio(3);
    const int j = id - n_attn;
    lstm_body<Cfg, true, true>(l, smem, j % lstm_cols, j / lstm_cols);
  }
}

// the early part on its own (profiling / ablation: what the role costs without a partner)
template <class Cfg>
__global__ __launch_bounds__(kGemmThreads, 4) void lstm_lean_kernel(LstmArgs l) {
  __shared__ __attribute__((aligned(16))) float smem[Cfg::kLdsFloats];
  lstm_body<Cfg, false>(l, smem, blockIdx.x, blockIdx.y);
}

static_assert(kFrameThreads == kGemmThreads && kAttnThreads == kGemmThreads, "roles share one block size");

bool fused_supported(int d_mel, int r, int Ph, int P, int D) {
  // (frame role: 6 projection columns per thread; attention role: NJ <= 2 - both to stay within 128 VGPRs)
  return frame_supported(d_mel, r, Ph, P) && r * d_mel + r <= 96 && D / 4 <= 128;
}

int frame_grid_size(int M, int P) { return ((P + kFrameCols - 1) / kFrameCols) * ((M + kFrameRows - 1) / kFrameRows); }

// which tile the LSTM role runs on, by batch size (see the three configurations above)
enum LeanKind { LEAN_64x16, LEAN_64x8, SMALL_FAT };
template <int PREC>
static int lean_bm(LeanKind kind) {  // batch rows of the kind's tile
  using TL = LeanTiles<PREC>;
  return kind == SMALL_FAT ? TL::SmallFat::BM : (kind == LEAN_64x8 ? TL::Lean64x8::BM : TL::Lean64x16::BM);
}
static int lean8_max_rows(bool f16) {
  if (f16) return kLean8MaxRows;
  static const int f32_max = [] { const char* e = getenv("TTSDEC_LEAN8_F32_MAX"); return e ? atoi(e) : kLean8MaxRowsF32; }();  // (measurement)
  return f32_max;
}
static LeanKind lean_kind(int M, int n_producer, int H, bool f16 = true) {
  if (M <= kSmallFatMaxRows && n_producer + (H + 7) / 8 <= 224) return SMALL_FAT;
  return M <= lean8_max_rows(f16) ? LEAN_64x8 : LEAN_64x16;
}

template <int K0H, int PH, int PREC, bool kHead>
static void launch_frame_lstm_ph(const FrameArgs& f, const LstmArgs& l, const ProjArgs& pj, hipStream_t st) {
  using TL = LeanTiles<PREC>;
  const int fcols = (f.P + kFrameCols - 1) / kFrameCols, frows = (f.M + kFrameRows - 1) / kFrameRows;
  const int n_frame = fcols * frows, n_proj = kHead ? proj_grid_size(pj.M, pj.N, pj.ksplit) : 0;
  const LeanKind kind = lean_kind(l.M, n_proj + n_frame, l.H, PREC == PREC_F16S);
  const int lcols = kind == LEAN_64x16 ? (l.H + 15) / 16 : (l.H + 7) / 8;
  const int bm = lean_bm<PREC>(kind);
  const int lrows = (l.M + bm - 1) / bm;
  dim3 grid(n_proj + n_frame + lcols * lrows), block(kGemmThreads);
  if (kind == SMALL_FAT)
    hipLaunchKernelGGL((frame_lstm_kernel<K0H, PH, typename TL::SmallFat, 2, kHead>), grid, block, 0, st, f, l, pj, n_proj, n_frame, fcols, lcols);
  else if (kind == LEAN_64x8)
    hipLaunchKernelGGL((frame_lstm_kernel<K0H, PH, typename TL::Lean64x8, 4, kHead>), grid, block, 0, st, f, l, pj, n_proj, n_frame, fcols, lcols);
  else
    hipLaunchKernelGGL((frame_lstm_kernel<K0H, PH, typename TL::Lean64x16, 4, kHead>), grid, block, 0, st, f, l, pj, n_proj, n_frame, fcols, lcols);
}
template <bool kHead>
static void launch_frame_lstm_any(const FrameArgs& f, const LstmArgs& l, const ProjArgs& pj, hipStream_t st) {
  if (f.M <= 0) return;
  const bool f16 = l.prec == 1;
  if (f.Ph == 256) { if (f16) launch_frame_lstm_ph<40, 256, PREC_F16S, kHead>(f, l, pj, st); else launch_frame_lstm_ph<40, 256, PREC_F32, kHead>(f, l, pj, st); }
  else { if (f16) launch_frame_lstm_ph<40, 128, PREC_F16S, kHead>(f, l, pj, st); else launch_frame_lstm_ph<40, 128, PREC_F32, kHead>(f, l, pj, st); }
}
void launch_frame_lstm(const FrameArgs& f, const LstmArgs& l, hipStream_t st) {
  ProjArgs none;
  memset(&none, 0, sizeof(none));
  launch_frame_lstm_any<false>(f, l, none, st);
}
void launch_proj_frame_lstm(const ProjArgs& pj, const FrameArgs& f, const LstmArgs& l, hipStream_t st) { launch_frame_lstm_any<true>(f, l, pj, st); }

// Workgroups of a multi-role kernel the device holds AT ONCE, as its runtime says: CUs x hipOccupancyMaxActiveBlocksPerMultiprocessor
// (registers, LDS and the wave limit of THIS kernel on THIS device - a partitioned or smaller part answers for itself).  The
// schedule in which workgroups of one role wait for EACH OTHER (the query role) is only taken when all of them fit that
// number; it further assumes the GPU is not shared with another process's kernels (what the number cannot know - the
// bounded spin and Decoder.forward's fallback cover that case).  0 when the query fails: that schedule stays off.
static int resident_slots(const void* fn) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_pair(dev, fn);
  const auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int cus = 0, per_cu = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kGemmThreads, 0) != hipSuccess) {
    (void)hipGetLastError();
    cus = per_cu = 0;
  }
  return cache[key] = cus * per_cu;
}

typedef void (*attn_lstm_fn)(AttnArgs, LstmArgs, ProjArgs, int, int);
// The attention pass per regime: ATTN_LEAN beside the exact-fp32 LSTM on the 64 x 16 tile (B > 96), whose fp32 MFMA chain shares
// each SIMD with the attention waves; ATTN_BASE elsewhere (split-fp16: 16-bit MFMAs leave the vector ALU alone; small batches:
// the roles rarely share a CU).  variant (measurement, option attn_form, exact fp32 64 x 16 tile only): 1 = ATTN_BASE,
// 2 = ATTN_ONE_ROW, 3 = ATTN_PLAIN_SUM, 4 = ATTN_PRIO_SWAP, 5 = ATTN_LEAN.
template <int NJ>
static attn_lstm_fn attn_lstm_f32_wide(int variant) {
  using C = LeanTiles<PREC_F32>::Lean64x16;
  switch (variant) {
    case 1: return attn_lstm_kernel<NJ, C, 4, ATTN_BASE>;
    case 2: return attn_lstm_kernel<NJ, C, 4, ATTN_ONE_ROW>;
    case 3: return attn_lstm_kernel<NJ, C, 4, ATTN_PLAIN_SUM>;
    case 4: return attn_lstm_kernel<NJ, C, 4, ATTN_PRIO_SWAP>;
    default: return attn_lstm_kernel<NJ, C, 4, ATTN_LEAN>;
  }
}
template <int NJ, int PREC>
static attn_lstm_fn attn_lstm_kernel_of(LeanKind kind, int variant) {
  using TL = LeanTiles<PREC>;
  if (kind == SMALL_FAT) return attn_lstm_kernel<NJ, typename TL::SmallFat, 2>;
  if (kind == LEAN_64x8) return attn_lstm_kernel<NJ, typename TL::Lean64x8, 4>;
  if constexpr (PREC == PREC_F32) return attn_lstm_f32_wide<NJ>(variant);
  return attn_lstm_kernel<NJ, typename TL::Lean64x16, 4>;
}
static attn_lstm_fn attn_lstm_kernel_for(int D, bool f16, LeanKind kind, int variant = 0) {
  if (D / 4 <= 64) return f16 ? attn_lstm_kernel_of<1, PREC_F16S>(kind, variant) : attn_lstm_kernel_of<1, PREC_F32>(kind, variant);
  return f16 ? attn_lstm_kernel_of<2, PREC_F16S>(kind, variant) : attn_lstm_kernel_of<2, PREC_F32>(kind, variant);
}
int attn_lstm_resident_slots(int B, int H, int D, bool f16) {
  return resident_slots(reinterpret_cast<const void*>(attn_lstm_kernel_for(D, f16, lean_kind(B, B, H, f16))));
}
void launch_attn_lstm(const AttnArgs& a, const LstmArgs& l, const ProjArgs* q, hipStream_t st, int variant) {
  if (a.B <= 0) return;
  ProjArgs pq;
  if (q != nullptr) pq = *q;
  else memset(&pq, 0, sizeof(pq));
  const LeanKind kind = lean_kind(l.M, a.B, l.H, l.prec == 1);
  const int lcols = kind == LEAN_64x16 ? (l.H + 15) / 16 : (l.H + 7) / 8;
  const int bm = l.prec == 1 ? lean_bm<PREC_F16S>(kind) : lean_bm<PREC_F32>(kind);
  const int lrows = (l.M + bm - 1) / bm;
  dim3 grid(a.B + lcols * lrows), block(kGemmThreads);
  hipLaunchKernelGGL(attn_lstm_kernel_for(a.D, l.prec == 1, kind, variant), grid, block, 0, st, a, l, pq, a.B, lcols);
}

void launch_lstm_lean(const LstmArgs& l, hipStream_t st) {
  if (l.M <= 0) return;
  const bool small = l.M <= lean8_max_rows(l.prec == 1);
  const LeanKind kind = small ? LEAN_64x8 : LEAN_64x16;
  const int bm = l.prec == 1 ? lean_bm<PREC_F16S>(kind) : lean_bm<PREC_F32>(kind);
  dim3 grid(small ? (l.H + 7) / 8 : (l.H + 15) / 16, (l.M + bm - 1) / bm), block(kGemmThreads);
  if (l.prec == 1) {
    if (small) hipLaunchKernelGGL((lstm_lean_kernel<LeanTiles<PREC_F16S>::Lean64x8>), grid, block, 0, st, l);
    else hipLaunchKernelGGL((lstm_lean_kernel<LeanTiles<PREC_F16S>::Lean64x16>), grid, block, 0, st, l);
  } else {
    if (small) hipLaunchKernelGGL((lstm_lean_kernel<LeanTiles<PREC_F32>::Lean64x8>), grid, block, 0, st, l);
    else hipLaunchKernelGGL((lstm_lean_kernel<LeanTiles<PREC_F32>::Lean64x16>), grid, block, 0, st, l);
  }
}

}  // namespace ttsdec
