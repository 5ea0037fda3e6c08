// C ABI of libttsdec.so (see include/ttsdec.h).  Host-side orchestration only:
// argument checks, blob / workspace carving, and the per-step launch sequence.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>

#include "kernels.h"

using namespace ttsdec;

namespace ttsdec {
int current_device_or_minus1() {
  int ndev = 0, dev = -1;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && hipGetDevice(&dev) == hipSuccess) return dev;
  (void)hipGetLastError();
  return -1;
}
bool device_is_current(int device) {
  if (device < 0) return false;
  int cur = -1;
  return hipGetDevice(&cur) == hipSuccess && cur == device;
}

int hip_fail(HandleBase* h, hipError_t e, const char* where) {
  if (h) h->hip_err = std::string(where) + ": " + hipGetErrorString(e);
  return TTSDEC_ERR_HIP;
}
int record_hip_error(HandleBase* h, const char* where) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? TTSDEC_OK : hip_fail(h, e, where);
}

int pack_begin(HandleBase* h, const float* const* src, int n_src, int n_expected, bool null_ok, void* blob, size_t blob_bytes,
               hipStream_t st) {
  if (!h || !src || !blob || n_src != n_expected) return TTSDEC_ERR_INVALID_ARG;
  for (int i = 0; i < n_src && !null_ok; ++i)
    if (!src[i]) return TTSDEC_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(blob) & 255) return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(h->device)) return TTSDEC_ERR_DEVICE;
  const hipError_t e = hipMemsetAsync(blob, 0, blob_bytes, st);
  return e == hipSuccess ? TTSDEC_OK : hip_fail(h, e, "memset");
}
int pack_end(HandleBase* h, const float* blob) {
  const int rc = record_hip_error(h, "pack_weights");
  if (rc == TTSDEC_OK) h->blob = blob;
  return rc;
}
int bind_blob(HandleBase* h, const void* blob) {
  if (!h || !blob || (reinterpret_cast<uintptr_t>(blob) & 255)) return TTSDEC_ERR_INVALID_ARG;
  h->blob = static_cast<const float*>(blob);
  return TTSDEC_OK;
}
int set_precision(HandleBase* h, int precision) {
  if (!h || (precision != TTSDEC_PREC_F32 && precision != TTSDEC_PREC_SPLIT_F16)) return TTSDEC_ERR_INVALID_ARG;
  h->precision = precision;
  return TTSDEC_OK;
}
int get_precision(const HandleBase* h) { return h ? h->precision : TTSDEC_ERR_INVALID_ARG; }
const char* last_hip_error(const HandleBase* h) { return h ? h->hip_err.c_str() : ""; }
}  // namespace ttsdec

namespace {

constexpr int kMaxPostnetLayers = 8;

constexpr size_t kAbsent = ~(size_t)0;  // offset of a form the blob does not hold of a matrix

// One weight matrix [rows, cols] in every form the blob holds.  Offsets in floats; a 16-bit plane takes half a float per element.
struct Mat {
  size_t rows, cols;
  int src;        // the tensor (TTSDEC_W_*) its planes and the range guard are made from, or -1: the blob's own fp32 copy (a repack)
  size_t w;       // fp32
  size_t h, l;    // split-fp16 hi / lo planes
  size_t b;       // bf16 plane (the Postnet's matrices)
  size_t ch, cl;  // hi / lo planes in the chunked layout (common.h Seg3 / launch_pack_lstm_chunked): the LSTMs' when chunk_ok(dims)
  size_t n() const { return rows * cols; }
  size_t plane() const { return (n() + 1) / 2; }  // floats of one 16-bit plane
};

struct BlobLayout {  // offsets in floats
  Mat pre0, pre1, wq, att_ih, att_hh, dec_ih, dec_hh, proj;  // proj: [fc_mel ; fc_stop] stacked on the output axis (decoder.py:13-14)
  Mat conv[kMaxPostnetLayers], fc;                           // MelPostnet
  Mat p2[kMaxPostnetLayers][3];                              // MelPostnet2: per layer three Conv1dFix weights ...
  size_t p2_alpha[kMaxPostnetLayers][2], p2_beta[kMaxPostnetLayers][2];  // ... and two folded BatchNorms
  size_t conv_alpha[kMaxPostnetLayers], conv_beta[kMaxPostnetLayers];
  size_t pre0_b, pre1_b, att_b, dec_b, proj_b;
  size_t pre0_ph, pre0_pl, pre1_ph, pre1_pl;  // the PreNet planes in the frame kernel's lane order (launch_split_frame_order; layer 1 padded to 64 rows)
  size_t h0a, c0a, h0d, c0d;
  size_t wmax;  // [0] max |w| over the decoder matrices that have split-fp16 planes, [1] the same over the Postnet's
  size_t total;
};

}  // namespace

constexpr int kGraphSlots = 30;  // decode steps per captured graph (even: buffer parity is baked per slot)
// Split-K factors of the two small GEMMs of a step (their consumers add the slabs in order):
// at B=256 the query projection then launches 256 workgroups instead of 128 and the mel/stop
// projection 96 instead of 24, each with a proportionally shorter K loop.
constexpr int kQuerySplit = 4;  // (upper bound: 2 slices for K = 1024, 4 for the Taco2 cell's K = 2048)
constexpr int kProjSplit = 4;

struct ttsdec_handle : HandleBase {  // (device -1: no HIP device was available at create; host-only queries still work)
  ttsdec_dims d;
  BlobLayout bl;
  // Two-role launches (fused_kernels.hip) where they apply: 1 = frame || lstm_att; 2 = also attention || lstm_dec;
  // 0 = off; -1 (default) = by batch size: level 2 up to 320 utterances, level 1 above.  Measured us per step for levels
  // 1 / 2 (end of round 2): B = 128 69.0 / 53.7, B = 192 66.2 / 59.5, B = 256 77.2 / 70.2.  Until the attention role's row sums
  // moved from ds_bpermute to DPP (common.h wave_sum) level 2 LOST from 192 utterances on (B = 256: 80.8 / 86.1): the role's
  // LDS-path shuffles queued behind the co-resident LSTM workgroup's LDS traffic, the attention workgroups finished late and
  // every LSTM workgroup waited for the slowest of them.  (Split-fp16; exact fp32: see overlap_level.)
  // Option "overlap" = 0 / 1 / 2 (a larger value means 2).
  int overlap;
  // Four on / off options: -1 = default (on), 0, 1.
  int opt_graph;                  // replay a captured hipGraph instead of launching every kernel (option "graph")
  int opt_chunk_a, opt_chunk_b;   // chunked layout of the activation planes / LSTM weight planes (options "chunk_a" / "chunk_b")
  int opt_proj_regw;              // mel/stop projection on the register-weight kernel where it applies (option "proj_regw")
  bool use_graph() const { return opt_graph != 0; }
  bool chunk_a() const { return opt_chunk_a != 0; }
  bool chunk_b() const { return opt_chunk_b != 0; }
  bool proj_regw() const { return opt_proj_regw != 0; }
  int head_proj;          // that projection as a role at the head of the NEXT step's frame launch: 1 / 0, -1 = by batch size; TTSDEC_HEAD_PROJ
  int attn_form;          // measurement: the form of the exact-fp32 attention pass on the 64 x 16 tile (include/ttsdec.h)
  int query_role;         // attention query as a job of the attention role's workgroups (step_order): 1 / 0, -1 = default
  int profile_ablation;   // ttsdec_profile_step only: the kernels' dbg switches (measurement ablations)
  int debug_flags;        // test hooks, copied into Ctrl::debug_flags: bit 0 = the frame role does not signal, bit 1 = the attention
                          // role does not, bit 2 = the projection head role does not (drives the bounded-spin time-out path)
  int spin_limit;         // polls before a role gives up waiting (common.h role_wait); 0 = kRoleSpinLimit
  hipStream_t cap_stream;
  bool streams_ready;
  // one cached graph: valid for exactly this (workspace, blob, B, L, precision)
  hipGraphExec_t gexec;
  hipGraph_t graph;
  const void* g_ws;
  const void* g_blob;
  int g_B, g_L, g_prec;
  // max |w| read back from the blob header (pack / bind): a weight at or beyond the fp16 range has no
  // split-fp16 form, so the affected GEMMs stay on exact fp32 (ttsdec_get_precision reports it)
  float wmax_dec, wmax_post;
  unsigned long long* stamps_buf;  // measurement only (TTSDEC_STAMPS): device buffer of this handle's device
};

namespace {

// derived sizes that depend on the cell type
inline int pre_hidden(const ttsdec_dims& d) { return d.d_pre_hidden > 0 ? d.d_pre_hidden : d.d_pre; }
inline bool is_taco2(const ttsdec_dims& d) { return d.cell_type == TTSDEC_CELL_TACO2; }
inline int query_ld(const ttsdec_dims& d) { return is_taco2(d) ? d.h_att + d.h_dec + d.d_ctx : d.h_att; }
inline int query_k(const ttsdec_dims& d) { return is_taco2(d) ? d.h_att + d.h_dec : d.h_att; }
inline int proj_ld(const ttsdec_dims& d) { return is_taco2(d) ? d.h_att + d.h_dec + d.d_ctx : d.h_dec + d.d_ctx; }
inline int proj_k(const ttsdec_dims& d) { return is_taco2(d) ? d.h_att + d.h_dec : d.h_dec + d.d_ctx; }
inline int proj_n(const ttsdec_dims& d) { return d.r * d.d_mel + d.r; }
inline int proj_ldp(const ttsdec_dims& d) { return (proj_n(d) + 3) & ~3; }
// The fused frame kernel (frame_kernel.hip) covers the shipped PreNet shapes; other dims keep the
// three-launch form (proj with its own epilogue, prenet0, prenet1).
inline bool use_frame(const ttsdec_dims& d) { return frame_supported(d.d_mel, d.r, pre_hidden(d), d.d_pre); }
// The chunked operand layout of the LSTM GEMMs (common.h Seg3): whole 32-element chunks in every K segment,
// whole 16-unit blocks, and the frame kernel as the producer of the x_pre planes.
inline bool chunk_ok(const ttsdec_dims& d) {
  return use_frame(d) && !((d.d_pre | d.d_ctx | d.h_att | d.h_dec) & 31);
}
inline int rows_pad(int B) { return (B + 63) / 64 * 64; }  // rows per chunk of the activation planes
inline int split_of(int K, int want);
inline int query_split(const ttsdec_dims& d);
inline int split_of(int K, int want) {  // split-K factor: slices must be whole 128-element K tiles
  while (want > 1 && (K % want || (K / want) % 128)) --want;
  return want;
}

inline int query_split(const ttsdec_dims& d) { return split_of(query_k(d), query_k(d) >= 2048 ? kQuerySplit : 2); }
// The mel/stop projection on the register-weight kernel (frame_kernel.hip proj_kernel) in split-fp16 mode where it
// covers the shape: whole 8-element groups in every K segment, K slices of whole 128-element blocks; else the LDS-staged
// split-K GEMM.  Measured, proj launch / step in the loop: B = 256 5.0 / 83.6 us against 6.7 / 84.1, B = 1 4.3 / 46.9
// against 5.5 / 47.9; exact fp32 (64-cycle MFMAs, 8 per k16 step) 7.0 against 6.4 - so split-fp16 only.
// (Exact fp32 takes it where the projection then becomes the head role of the next step's first launch - batches with the
// two-role launches: the role's 7 us hide under the fp32 attention LSTM's 48-us stream and the step loses the projection's own
// launch: 128.6 -> 121.4 us per step at B = 256, 56.2 -> 54.4 at B = 32, 54.0 -> 50.2 at B = 1; profiles/r03_w_fp32_head_proj.txt.)
inline bool proj_regw_shapes(const ttsdec_handle* h) {
  const ttsdec_dims& d = h->d;
  return h->proj_regw() && use_frame(d) && !((d.h_att | d.h_dec | d.d_ctx) & 7) && proj_split(proj_k(d)) > 0 && proj_n(d) <= 192;
}
inline bool proj_regw(const ttsdec_handle* h, int prec) {
  return proj_regw_shapes(h) && (prec || h->head_proj != 0);  // (exact fp32: as a head role - head_proj() - only)
}
inline int proj_parts(const ttsdec_handle* h, int prec) {
  return proj_regw(h, prec) ? proj_split(proj_k(h->d)) : split_of(proj_k(h->d), kProjSplit);
}

// Every matrix's shape is stated here, once; the walk below is the blob: its order must not change.
BlobLayout make_blob_layout(const ttsdec_dims& d) {
  BlobLayout L;
  memset(&L, 0, sizeof(L));
  Carver cv{nullptr};
  const size_t Ha = d.h_att, Hd = d.h_dec, D = d.d_ctx, P = d.d_pre, Mel = d.d_mel, R = d.r, Ph = pre_hidden(d);
  const size_t Hh = d.postnet_hidden, k = d.postnet_kernel;
  auto mat = [](size_t rows, size_t cols, int src) { return Mat{rows, cols, src, kAbsent, kAbsent, kAbsent, kAbsent, kAbsent, kAbsent}; };
  auto take_w = [&](Mat& m) { m.w = cv.take_off(m.n()); };
  auto take_split = [&](Mat& m) { m.h = cv.take_off(m.plane()); m.l = cv.take_off(m.plane()); };
  auto take_w16 = [&](Mat& m) { take_w(m); m.b = cv.take_off(m.plane()); take_split(m); };  // a Postnet matrix: w, wb, wh, wl
  L.pre0 = mat(Ph, Mel, TTSDEC_W_PRE0_W);
  L.pre1 = mat(P, Ph, TTSDEC_W_PRE1_W);
  L.wq = mat(D, query_ld(d), TTSDEC_W_QUERY_W);
  L.att_ih = mat(4 * Ha, P + D, TTSDEC_W_ATT_IH);
  L.att_hh = mat(4 * Ha, Ha, TTSDEC_W_ATT_HH);
  L.dec_ih = mat(4 * Hd, Ha + D, TTSDEC_W_DEC_IH);
  L.dec_hh = mat(4 * Hd, Hd, TTSDEC_W_DEC_HH);
  L.proj = mat(R * Mel + R, proj_ld(d), -1);
  Mat* const lstm[4] = {&L.att_ih, &L.att_hh, &L.dec_ih, &L.dec_hh};

  L.wmax = cv.take_off(2);
  take_w(L.pre0); L.pre0_b = cv.take_off(Ph);
  take_w(L.pre1); L.pre1_b = cv.take_off(P);
  take_w(L.wq);
  take_w(L.att_ih); take_w(L.att_hh); L.att_b = cv.take_off(4 * Ha);
  take_w(L.dec_ih); take_w(L.dec_hh); L.dec_b = cv.take_off(4 * Hd);
  take_split(L.pre0); take_split(L.pre1);
  L.pre0_ph = cv.take_off(L.pre0.plane()); L.pre0_pl = cv.take_off(L.pre0.plane());
  const size_t p64 = (P + 63) / 64 * 64;
  L.pre1_ph = cv.take_off((p64 * Ph + 1) / 2); L.pre1_pl = cv.take_off((p64 * Ph + 1) / 2);
  for (Mat* m : lstm) take_split(*m);
  if (chunk_ok(d))
    for (Mat* m : lstm) { m->ch = cv.take_off(m->plane()); m->cl = cv.take_off(m->plane()); }
  L.h0a = cv.take_off(Ha);
  L.c0a = cv.take_off(Ha);
  L.h0d = cv.take_off(Hd);
  L.c0d = cv.take_off(Hd);
  take_w(L.proj); L.proj_b = cv.take_off(R * Mel + R);
  take_split(L.wq);
  take_split(L.proj);
  if (d.postnet_type == TTSDEC_POSTNET_TYPE_MEL2) {
    const size_t shapes[3][2] = {{Hh, Mel}, {Hh, Hh}, {Mel, Hh}};  // [C_out, C_in] of the three convs
    for (int i = 0; i < d.postnet_layers; ++i) {
      for (int c = 0; c < 3; ++c) take_w16(L.p2[i][c] = mat(shapes[c][0], shapes[c][1] * k, -1));
      for (int c = 0; c < 2; ++c) { L.p2_alpha[i][c] = cv.take_off(Hh); L.p2_beta[i][c] = cv.take_off(Hh); }
    }
    L.total = cv.off;
    return L;
  }
  for (int i = 0; i < d.postnet_layers; ++i) {
    Mat& m = L.conv[i] = mat(Hh, k * (i ? Hh : Mel), -1);
    take_w(m);
    L.conv_alpha[i] = cv.take_off(Hh);
    L.conv_beta[i] = cv.take_off(Hh);
    m.b = cv.take_off(m.plane());
    take_split(m);
  }
  if (d.postnet_layers > 0) take_w16(L.fc = mat(Mel, Hh, TTSDEC_W_DECODER_COUNT + TTSDEC_W_POSTNET_PER_LAYER * d.postnet_layers));
  L.total = cv.off;
  return L;
}

int check_dims(const ttsdec_dims& d) {
  const int v[] = {d.d_mel, d.d_pre, d.d_ctx, d.h_att, d.h_dec};
  for (int x : v)
    if (x <= 0 || (x & 3)) return TTSDEC_ERR_DIMS;
  if (d.r < 1 || d.d_ctx > 1024) return TTSDEC_ERR_DIMS;  // attn_kernel<4> covers d_ctx/4 <= 256 float4 columns
  if (d.d_pre_hidden < 0 || (d.d_pre_hidden & 3)) return TTSDEC_ERR_DIMS;
  if (d.cell_type != TTSDEC_CELL_TACO2PROD && d.cell_type != TTSDEC_CELL_TACO2) return TTSDEC_ERR_DIMS;
  if (d.postnet_type != TTSDEC_POSTNET_TYPE_MEL && d.postnet_type != TTSDEC_POSTNET_TYPE_MEL2) return TTSDEC_ERR_DIMS;
  if (d.postnet_layers < 0 || d.postnet_layers > kMaxPostnetLayers) return TTSDEC_ERR_DIMS;
  if (d.postnet_layers > 0) {
    if (d.postnet_hidden <= 0 || (d.postnet_hidden & 3)) return TTSDEC_ERR_DIMS;
    if (d.postnet_kernel < 1 || !(d.postnet_kernel & 1)) return TTSDEC_ERR_DIMS;
  }
  if (!(d.p_zoneout >= 0.f && d.p_zoneout < 1.f)) return TTSDEC_ERR_DIMS;
  if (!(d.p_dropout >= 0.f && d.p_dropout < 1.f)) return TTSDEC_ERR_DIMS;
  return TTSDEC_OK;
}

#define HIP_TRY(h, expr)                                  \
  do {                                                    \
    hipError_t _e = (expr);                               \
    if (_e != hipSuccess) return hip_fail(h, _e, #expr); \
  } while (0)

int check_device(ttsdec_handle* h) { return device_is_current(h->device) ? TTSDEC_OK : TTSDEC_ERR_DEVICE; }

struct StepBufs {
  Ctrl* ctrl;
  float *xpre0, *xpre, *ctx, *h_att[2], *c_att, *h_dec[2], *c_dec, *q, *ynext, *w[2];
  f16 *xpre_h, *xpre_l, *ctx_h, *ctx_l, *h_att_h[2], *h_att_l[2], *h_dec_h[2], *h_dec_l[2];
  float* jparts;  // split-K partial sums of the mel/stop projection [kProjSplit][B, proj_ldp]
  unsigned long long* loop_stamps;  // measurement only: launch start times of one graph replay [kLoopStampSlots][kLoopStampNodes] (common.h)
  unsigned int* dep;  // arrival counters of the two-role launches: [DEP_KINDS][32-row blocks][kDepLine] (common.h), dep_bytes in all
  size_t dep_bytes;
  size_t bytes;  // the whole layout, or 0: refused (layout.h within_dma_reach)
  int dep_blocks;  // 32-row blocks of the batch: dep + kind * dep_blocks * kDepLine is a hand-off kind's counter array
};

// The decode workspace (carved as layout.h's Carver comment says)
StepBufs carve(Carver& cv, const ttsdec_dims& d, int B, int Lm) {
  StepBufs s;
  s.ctrl = reinterpret_cast<Ctrl*>(cv.take((sizeof(Ctrl) + sizeof(float) - 1) / sizeof(float)));
  const size_t b = (size_t)B;
  s.xpre0 = cv.take(b * pre_hidden(d)); s.xpre = cv.take(b * d.d_pre); s.ctx = cv.take(b * d.d_ctx);
  s.h_att[0] = cv.take(b * d.h_att); s.h_att[1] = cv.take(b * d.h_att); s.c_att = cv.take(b * d.h_att);
  s.h_dec[0] = cv.take(b * d.h_dec); s.h_dec[1] = cv.take(b * d.h_dec); s.c_dec = cv.take(b * d.h_dec);
  s.q = cv.take((size_t)kQuerySplit * b * d.d_ctx);
  s.ynext = cv.take(b * d.d_mel); s.w[0] = cv.take(b * Lm); s.w[1] = cv.take(b * Lm);
  auto takeh = [&](size_t nhalfs) { return cv.take_h((nhalfs + 1) / 2); };
  const size_t bp = (size_t)rows_pad(B);  // (the chunked layout pads the rows of a plane to whole 64-row blocks)
  s.xpre_h = takeh(bp * d.d_pre); s.xpre_l = takeh(bp * d.d_pre);
  s.ctx_h = takeh(bp * d.d_ctx); s.ctx_l = takeh(bp * d.d_ctx);
  for (int i = 0; i < 2; ++i) {
    s.h_att_h[i] = takeh(bp * d.h_att); s.h_att_l[i] = takeh(bp * d.h_att);
    s.h_dec_h[i] = takeh(bp * d.h_dec); s.h_dec_l[i] = takeh(bp * d.h_dec);
  }
  s.jparts = cv.take((size_t)kProjSplit * b * proj_ldp(d));
  // (unused: two [B, 4H] spans that a retired scheme parked gate sums in; kept so that every offset behind them, and the size
  // ttsdec_workspace_bytes reports, stay what callers have allocated for)
  cv.take_off(b * 4 * d.h_att); cv.take_off(b * 4 * d.h_dec);
  s.loop_stamps = reinterpret_cast<unsigned long long*>(cv.take(kLoopStampSlots * kLoopStampNodes * 2));
  s.dep_blocks = (B + 31) / 32;
  s.dep_bytes = (size_t)DEP_KINDS * s.dep_blocks * kDepLine * sizeof(unsigned int);
  s.dep = reinterpret_cast<unsigned int*>(cv.take(s.dep_bytes / sizeof(float)));
  s.bytes = within_dma_reach(cv.bytes());
  return s;
}

// How one step's kernels find "now": inside ttsdec_decode everything per-call lives in the
// device control block and a kernel only gets its slot (use_ctrl); cell_step / profiling pass
// explicit values.
struct StepIo {
  const float* memory;
  int B, L;
  int slot;               // use_ctrl: step = ctrl->t_cur + slot; buffer parity = slot & 1 (t_cur is even)
  int t, t_rel, t_stride;  // !use_ctrl
  int dropout_mode;
  const uint8_t* masks;  // !use_ctrl: [2, B, d_pre] of this step
  uint64_t seed;
  float *y, *s, *w;
  bool use_ctrl;
  int finalize;  // !use_ctrl, frame kernel: the projection partial sums are the previous step's frame
  int dbg;
  int node_pos;  // position of the launch in the step order (measurement: common.h loop_stamp)
};

// The kernels of one decode step.  N_F is the fused frame kernel (finish the previous step's
// projection + both PreNet layers), N_FIN its end-of-call form; N_P0 / N_P1 are the separate
// PreNet layers used when the dims are outside what the frame kernel covers.
// Two-role step (fused_kernels.hip): N_FA = frame || attention LSTM, N_TD = attention || decoder LSTM;
// N_AG / N_DG are those LSTMs alone on the lean tile (profiling).  N_JFA = N_FA with the PREVIOUS step's mel/stop projection as a
// role at its head (then no N_J in the step), N_JFIN = the projection of a call's last step.
// N_QTD = N_TD whose attention-role workgroups first compute the query GEMM between them (then no N_Q in the step).
// N_JF = [proj(t-1) | frame] as one launch (no LSTM role).
enum Node { N_F, N_FIN, N_P0, N_P1, N_A, N_Q, N_T, N_D, N_J, N_FA, N_TD, N_AG, N_DG, N_JFA, N_JFIN, N_QTD, N_JF };

constexpr int kMaxKernelsPerStep = 7;
struct StepOrder {
  int n;
  Node nodes[kMaxKernelsPerStep];
};

// split-fp16 needs every K segment to be whole 16-byte columns of fp16 (multiples of 8)
bool split_ok(const ttsdec_dims& d) { return !((d.d_pre | d.d_ctx | d.h_att | d.h_dec) & 7); }
// launch order of one step: the Prod cell attends between its two LSTMs, the Taco2 cell after both
StepOrder step_order(const ttsdec_handle* h, int B);
const char* node_name(Node n);
bool head_proj(const ttsdec_handle* h);
bool query_role(const ttsdec_handle* h, int B);
int& option_ref(ttsdec_handle* h, int o);
void apply_env_options(ttsdec_handle* h);
void drop_graph(ttsdec_handle* h);
int lstm_prec(const ttsdec_handle* h) {
  return (h->precision == TTSDEC_PREC_SPLIT_F16 && split_ok(h->d) && h->wmax_dec < kSplitMax) ? 1 : 0;
}
// rows per chunk of the activation planes when they are in the chunked layout (common.h Seg3), 0 = row-major
int act_mpad(const ttsdec_handle* h, int B) { return (lstm_prec(h) && chunk_ok(h->d) && h->chunk_a()) ? rows_pad(B) : 0; }

// matrix m of the decoder blob as a GEMM's W / W_lo in `prec` (kernels.h Planes): its fp32 copy | hi + lo planes | bf16 plane
Planes weight(const Mat& m, const float* blob, int prec) {
  if (prec == PREC_F16S) return {blob + m.h, blob + m.l};
  return planes_f32(blob + (prec == PREC_BF16 ? m.b : m.w));
}

// reads the two weight maxima back from the blob header (one small synchronous copy)
int read_wmax(ttsdec_handle* h, hipStream_t st) {
  float v[2] = {0.f, 0.f};
  if (hipStreamSynchronize(st) != hipSuccess) return hip_fail(h, hipGetLastError(), "wmax sync");
  hipError_t e = hipMemcpy(v, h->blob + h->bl.wmax, sizeof(v), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(h, e, "wmax readback");
  // (a NaN maximum compares false below, i.e. also keeps the GEMMs on fp32)
  h->wmax_dec = v[0] == v[0] ? v[0] : INFINITY;
  h->wmax_post = v[1] == v[1] ? v[1] : INFINITY;
  return TTSDEC_OK;
}

// An activation as a GEMM's a / a_lo: its (hi, lo) planes in the layout in use, or fp32 (twice).
struct Act {
  Seg3 a, a_lo;
};
// One K segment of an LSTM cell's gates GEMM; each operand three ways: [0] fp32, [1] / [2] the split-fp16 hi / lo plane
struct KSeg {
  const void* a[3];  // the activation [B, k]
  int k;
  const void* w[3];  // its columns of W_ih or W_hh
  int ldw;           // their leading "dimension": row-major elements per row, or (chunked) the matrix's chunks per unit block
};
// The K walk of a cell, as indices into {0: seg0 = x_pre (attention LSTM) or h_att (decoder LSTM), 1: ctx, 2: the cell's own h}.
// A cell that is a role of a two-role launch (gated) walks the segment that the launch's other role writes LAST, behind the
// gate.  The exact-fp32 outputs are pinned to these three summation orders.
constexpr int kSegOrder[3][3] = {
    {0, 1, 2},  // whole cell: cat[seg0, ctx | h] (decoder_cell.py:187, :191)
    {1, 2, 0},  // gated attention LSTM: x_pre is written by the frame role of the same launch
    {2, 0, 1},  // gated decoder LSTM: ctx is written by the attention role of the same launch
};

// The argument builders of a step's launches: one per kind of kernel argument, over what all of them read.
struct StepArgs {
  const ttsdec_handle* h; const StepBufs& sb; const StepIo& io;
  const ttsdec_dims& d; const BlobLayout& bl; const float* blob;  // (the handle's)
  int p;  // buffer parity of the step: the state it reads is in buffers p, what it writes in 1 - p
  Ctrl* ctrl;
  int B, P, D, Ha, Hd, prec, mpad;

  StepArgs(const ttsdec_handle* h_, const StepBufs& sb_, const StepIo& io_)
      : h(h_), sb(sb_), io(io_), d(h_->d), bl(h_->bl), blob(h_->blob), p((io_.use_ctrl ? io_.slot : io_.t) & 1),
        ctrl(io_.use_ctrl ? sb_.ctrl : nullptr), B(io_.B), P(d.d_pre), D(d.d_ctx), Ha(d.h_att), Hd(d.h_dec), prec(lstm_prec(h_)),
        mpad(act_mpad(h_, io_.B)) {}

  const f16* plane(size_t float_off) const { return reinterpret_cast<const f16*>(blob + float_off); }
  Seg3 act(Seg3 s) const { return chunked(s, mpad); }  // an activation-plane segment list in the layout in use
  unsigned int* dep(int kind) const { return sb.dep + (size_t)kind * sb.dep_blocks * kDepLine; }  // a hand-off kind's arrival counters
  float keep_scale() const { return 1.0f / (1.0f - d.p_dropout); }
  Act pick(bool planes, Seg3 f32, Seg3 hi, Seg3 lo) const { return planes ? Act{act(hi), act(lo)} : Act{f32, f32}; }
  // cat[h_att, h_dec] of buffer parity q: the Taco2 cell's query and projection input, cat[h0, h1, zeros] (decoder_cell.py:126, :136)
  Act h01_in(int q, bool planes) const {
    return pick(planes, make_seg2(sb.h_att[q], Ha, Ha, sb.h_dec[q], Hd, Hd), make_seg2(sb.h_att_h[q], Ha, Ha, sb.h_dec_h[q], Hd, Hd),
                make_seg2(sb.h_att_l[q], Ha, Ha, sb.h_dec_l[q], Hd, Hd));
  }
  // query_layer input: h_att (Prod, decoder_cell.py:188)
  Act query_in(int q, bool planes) const {
    if (is_taco2(d)) return h01_in(q, planes);
    return pick(planes, make_seg1(sb.h_att[q], Ha, Ha), make_seg1(sb.h_att_h[q], Ha, Ha), make_seg1(sb.h_att_l[q], Ha, Ha));
  }
  // projection input: cat[h_dec, ctx] (Prod, decoder_cell.py:192)
  Act proj_in(int q, bool planes) const {
    if (is_taco2(d)) return h01_in(q, planes);
    return pick(planes, make_seg2(sb.h_dec[q], Hd, Hd, sb.ctx, D, D), make_seg2(sb.h_dec_h[q], Hd, Hd, sb.ctx_h, D, D),
                make_seg2(sb.h_dec_l[q], Hd, Hd, sb.ctx_l, D, D));
  }

  // The frame kernel (fin_only: its end-of-call form); signals: as the producer role of a two-role launch
  FrameArgs frame(bool fin_only, bool signals = false) const {
    FrameArgs f;
    memset(&f, 0, sizeof(f));
    const int Ph = pre_hidden(d);
    f.parts = sb.jparts; f.n_parts = proj_parts(h, prec); f.ldp = proj_ldp(d);
    f.part_stride = (size_t)B * proj_ldp(d);
    f.proj_bias = blob + bl.proj_b;
    f.y_out = io.y; f.s_out = io.s; f.ynext = sb.ynext;
    f.r = d.r; f.d_mel = d.d_mel; f.t_rel = io.t_rel; f.t_stride = io.t_stride;
    f.finalize = io.finalize; f.only_finalize = fin_only ? 1 : 0;
    f.dbg = io.dbg;
    if (io.dbg & 1) f.finalize = 0;       // measurement ablations (profile_step only)
    if (io.dbg & 8) f.only_finalize = 1;
    f.W0 = blob + bl.pre0.w; f.b0 = blob + bl.pre0_b; f.W1 = blob + bl.pre1.w; f.b1 = blob + bl.pre1_b;
    f.W0h = plane(bl.pre0_ph); f.W0l = plane(bl.pre0_pl); f.W1h = plane(bl.pre1_ph); f.W1l = plane(bl.pre1_pl);  // (lane order)
    f.prec = prec ? PREC_F16S : PREC_F32;
    f.Ph = Ph; f.P = P;
    f.dropout_mode = io.dropout_mode; f.masks = io.masks; f.mask_step_stride = (size_t)B * (Ph + P);
    f.seed = io.seed; f.keep_scale = keep_scale();
    f.xpre = sb.xpre;
    if (prec) { f.xpre_h = sb.xpre_h; f.xpre_l = sb.xpre_l; f.out_mpad = mpad; }
    f.M = B; f.ctrl = ctrl; f.slot = io.slot; f.node = io.node_pos; f.t = io.t;
    if (signals) { f.dep_signal = 1; f.dep_cnt = dep(DEP_FRAME); }
    return f;
  }

  // One LSTM cell.  which = 0: attention LSTM, cat[x_pre, ctx_prev | h_att] (decoder_cell.py:187); which = 1: decoder LSTM,
  // cat[h_att, ctx | h_dec] (:191).  gated: as the consumer role of a two-role launch (fused_kernels.hip) - the same cell, its
  // K segments in the order kSegOrder gives, with a gate before the last one.  (Always LstmArgs mode 0: the whole cell.)
  LstmArgs lstm(int which, bool gated) const {
    LstmArgs a;
    memset(&a, 0, sizeof(a));
    a.prec = prec;
    const int H = which ? Hd : Ha;
    const int k0 = which ? Ha : P;  // W_ih = [seg0 | ctx] columns
    const bool ck = prec && chunk_ok(d) && h->chunk_b();
    const Mat &ih = which ? bl.dec_ih : bl.att_ih, &hh = which ? bl.dec_hh : bl.att_hh;
    const f16 *wih_h = plane(ck ? ih.ch : ih.h), *wih_l = plane(ck ? ih.cl : ih.l), *whh_h = plane(ck ? hh.ch : hh.h), *whh_l = plane(ck ? hh.cl : hh.l);
    const float *wih = blob + ih.w, *whh = blob + hh.w;
    // column k0 of W_ih: row-major + k0 elements; chunked: chunk k0 / 32 of unit block 0 = k0 / 32 * (64 rows * 32) elements
    const size_t w1_off = ck ? (size_t)k0 * 64 : (size_t)k0;
    const int wld_ih = ck ? (k0 + D) / kChunkK : k0 + D, wld_hh = ck ? H / kChunkK : H;
    const KSeg seg[3] = {
        which ? KSeg{{sb.h_att[1 - p], sb.h_att_h[1 - p], sb.h_att_l[1 - p]}, k0, {wih, wih_h, wih_l}, wld_ih}
              : KSeg{{sb.xpre, sb.xpre_h, sb.xpre_l}, k0, {wih, wih_h, wih_l}, wld_ih},
        KSeg{{sb.ctx, sb.ctx_h, sb.ctx_l}, D, {wih + k0, wih_h + w1_off, wih_l + w1_off}, wld_ih},
        which ? KSeg{{sb.h_dec[p], sb.h_dec_h[p], sb.h_dec_l[p]}, H, {whh, whh_h, whh_l}, wld_hh}
              : KSeg{{sb.h_att[p], sb.h_att_h[p], sb.h_att_l[p]}, H, {whh, whh_h, whh_l}, wld_hh},
    };
    const int* o = kSegOrder[gated ? 1 + which : 0];
    const KSeg &s0 = seg[o[0]], &s1 = seg[o[1]], &s2 = seg[o[2]];
    auto a_segs = [&](int f) { return act(make_seg3(s0.a[f], s0.k, s0.k, s1.a[f], s1.k, s1.k, s2.a[f], s2.k, s2.k)); };
    auto w_segs = [&](int f) { return make_seg3(s0.w[f], s0.ldw, s0.k, s1.w[f], s1.ldw, s1.k, s2.w[f], s2.ldw, s2.k); };
    a.a = a_segs(prec ? 1 : 0); a.a_lo = a_segs(prec ? 2 : 0);
    a.w = w_segs(prec ? 1 : 0); a.w_lo = w_segs(prec ? 2 : 0);
    a.K = k0 + D + H;
    if (gated && which == 0) {
      a.dep_n = frame_grid_size(32, P); a.dep_seg = 2; a.dep_which = 0;  // (the frame workgroups of one 32-row block)
      a.dep_cnt = dep(DEP_FRAME);
      a.live_lag = 1;  // (same launch as the frame kernel: see lstm_body)
    } else if (gated) {
      a.dep_n = 32; a.dep_rows = 1; a.dep_seg = 2; a.dep_which = 1;  // (one attention workgroup per batch row)
      a.dep_cnt = dep(DEP_ATTN);
    }
    if (ck) { a.w.mpad = 1; a.w_lo.mpad = 1; }  // (flag: LoaderWLstm reads the chunked weight image)
    if (prec) { a.h_out_h = which ? sb.h_dec_h[1 - p] : sb.h_att_h[1 - p]; a.h_out_l = which ? sb.h_dec_l[1 - p] : sb.h_att_l[1 - p]; a.out_mpad = mpad; }
    a.bsum = blob + (which ? bl.dec_b : bl.att_b);
    a.h_prev = which ? sb.h_dec[p] : sb.h_att[p];
    a.c = which ? sb.c_dec : sb.c_att;
    a.h_out = which ? sb.h_dec[1 - p] : sb.h_att[1 - p];
    a.M = B; a.H = H; a.pz = d.p_zoneout; a.ctrl = ctrl; a.slot = io.slot; a.node = io.node_pos; a.dbg = io.dbg;
    a.tag = which;
    return a;
  }

  // The attention pass; signals: as the producer role of a two-role launch
  AttnArgs attn(bool signals = false) const {
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    if (prec) { a.ctx_h = sb.ctx_h; a.ctx_l = sb.ctx_l; a.out_mpad = mpad; }
    a.memory = io.memory; a.q = sb.q; a.q_parts = query_split(d); a.q_stride = (size_t)B * D;
    a.w_prev = sb.w[p]; a.w_new = sb.w[1 - p]; a.w_out = io.w; a.ctx = sb.ctx;
    a.B = B; a.L = io.L; a.D = D; a.t_rel = io.t_rel; a.t_stride = io.t_stride; a.ctrl = ctrl; a.slot = io.slot; a.node = io.node_pos;
    if (signals) { a.dep_signal = 1; a.dep_cnt = dep(DEP_ATTN); }
    return a;
  }
  // ... whose workgroups first compute the query tiles of pq between them
  AttnArgs attn_after_query(const ProjArgs& pq) const {
    AttnArgs a = attn(true);
    a.q_parts = pq.ksplit;
    a.q_tiles = proj_grid_size(B, D, pq.ksplit); a.q_wait_n = proj_grid_size(32, D, pq.ksplit); a.q_cnt = pq.dep_cnt;
    return a;
  }

  // What the query and projection GEMMs share, on either kernel (Args: GemmArgs / ProjArgs): [B, N] = in[B, K] * W^T, W = m's
  // first K of ldw columns
  template <class Args>
  Args gemm(const Act& in, const Mat& m, int gprec, int ldw, int N, int K) const {
    Args g = gemm_args_seg<Args>(in.a, in.a_lo, weight(m, blob, gprec), ldw, gprec, B, N, K);
    g.ctrl = ctrl; g.slot = io.slot;
    return g;
  }
  template <class Args>  // its split-K form: slab z of ksplit to out + z * [B, ldo]
  void split_k(Args& g, int ksplit, float* out, int ldo) const {
    g.ksplit = ksplit; g.split_stride = (size_t)B * ldo; g.out = out; g.ldo = ldo;
  }
  void gemm_place(GemmArgs& g) const { g.node = io.node_pos; g.t = io.t; }

  // PreNet layer 0 / 1 as a GEMM of its own (the three-launch form)
  GemmArgs prenet_gemm(int layer) const {
    const int Ph = pre_hidden(d);
    const Mat& m = layer ? bl.pre1 : bl.pre0;  // [Ph, d_mel] / [P, Ph]
    GemmArgs g = gemm_args(planes_f32(layer ? sb.xpre0 : sb.ynext), (int)m.cols, weight(m, blob, PREC_F32), PREC_F32, B, (int)m.rows, (int)m.cols);
    g.bias = blob + (layer ? bl.pre1_b : bl.pre0_b);
    g.out = layer ? sb.xpre : sb.xpre0;
    if (layer && prec) { g.out_h = sb.xpre_h; g.out_l = sb.xpre_l; g.out_kind = 1; }
    g.ctrl = ctrl; g.slot = io.slot;
    g.dropout_mode = io.dropout_mode;
    // masks of one step: layer 0 [B, Ph] then layer 1 [B, P]
    g.mask_step_stride = (size_t)B * (Ph + P);
    g.mask_layer_off = layer ? (size_t)B * Ph : 0;
    g.masks = io.masks ? io.masks + g.mask_layer_off : nullptr;
    g.seed = io.seed; g.layer = layer; g.keep_scale = keep_scale();
    g.r = d.r; g.d_mel = d.d_mel;
    gemm_place(g);
    return g;
  }
  // The attention query (decoder_cell.py:188 -> attention.py:105) from the new h_att (split-fp16 planes: the LSTM epilogues
  // emitted them for h, the pack step for the weights): as a GEMM of its own ...
  GemmArgs query_gemm() const {
    GemmArgs g = gemm<GemmArgs>(query_in(1 - p, prec != 0), bl.wq, prec ? PREC_F16S : PREC_F32, query_ld(d), D, query_k(d));
    split_k(g, query_split(d), sb.q, D);
    g.kchunk = g.K / g.ksplit;
    gemm_place(g);
    return g;
  }
  // ... or as a job of the attention role's workgroups
  ProjArgs query_role() const {
    ProjArgs pq = gemm<ProjArgs>(query_in(1 - p, prec != 0), bl.wq, prec ? PREC_F16S : PREC_F32, query_ld(d), D, query_k(d));
    split_k(pq, proj_split(pq.K), sb.q, D);
    pq.mode = PROJ_QUERY;
    pq.dep_cnt = dep(DEP_QUERY);
    return pq;
  }
  // The mel/stop projection of the step whose new state is in buffers q, in arithmetic jprec: on the register-weight kernel
  // (mode: PROJ_STEP / PROJ_HEAD / PROJ_FINAL) ...
  ProjArgs proj_role(int q, int jprec, int mode) const {
    ProjArgs pa = gemm<ProjArgs>(proj_in(q, jprec != PREC_F32), bl.proj, jprec, proj_ld(d), proj_n(d), proj_k(d));
    split_k(pa, proj_parts(h, prec), sb.jparts, proj_ldp(d));
    pa.node = io.node_pos;
    pa.mode = mode;
    return pa;
  }
  // ... or on the LDS-staged GEMM
  GemmArgs proj_gemm(int q, int jprec) const {
    GemmArgs g = gemm<GemmArgs>(proj_in(q, jprec != PREC_F32), bl.proj, jprec, proj_ld(d), proj_n(d), proj_k(d));
    gemm_place(g);
    if (use_frame(d)) {
      // raw split-K partial sums; bias, leaky-ReLU, y / s / stop rule happen in the next frame kernel
      split_k(g, split_of(g.K, kProjSplit), sb.jparts, proj_ldp(d));
      g.kchunk = g.K / g.ksplit;
      return g;
    }
    g.bias = blob + bl.proj_b;
    g.y_out = io.y; g.s_out = io.s; g.ynext = sb.ynext; g.r = d.r; g.d_mel = d.d_mel;
    g.t_rel = io.t_rel; g.t_stride = io.t_stride; g.stop_thr = 0.f; g.check_stop = 0;
    return g;
  }
};

// One launch of a step: which arguments, which launcher
void launch_node(const ttsdec_handle* h, const StepBufs& sb, const StepIo& io, Node node, hipStream_t st) {
  const StepArgs s(h, sb, io);
  const int attn_variant = h->attn_form > 0 ? h->attn_form : 0;  // (measurement: fused_kernels.hip attn_lstm_f32_wide)
  switch (node) {
    case N_F: launch_frame(s.frame(false), st); break;
    case N_FIN: launch_frame(s.frame(true), st); break;
    case N_FA: launch_frame_lstm(s.frame(false, true), s.lstm(0, true), st); break;
    case N_A: launch_lstm(s.lstm(0, false), st); break;
    case N_D: launch_lstm(s.lstm(1, false), st); break;
    case N_T: launch_attn(s.attn(), st); break;
    case N_TD: launch_attn_lstm(s.attn(true), s.lstm(1, true), nullptr, st, attn_variant); break;
    case N_QTD: {
      const ProjArgs pq = s.query_role();
      launch_attn_lstm(s.attn_after_query(pq), s.lstm(1, true), &pq, st, attn_variant);
      break;
    }
    case N_AG:
    case N_DG: {
      LstmArgs l = s.lstm(node == N_DG ? 1 : 0, true);
      l.dep_n = 0;  // (alone: nothing to wait for)
      launch_lstm_lean(l, st);
      break;
    }
    case N_P0: launch_gemm<A_PLAIN, EPI_RELU_DROPOUT>(s.prenet_gemm(0), st); break;
    case N_P1: launch_gemm<A_PLAIN, EPI_RELU_DROPOUT>(s.prenet_gemm(1), st); break;
    case N_Q: launch_gemm<A_PLAIN, EPI_PLAIN>(s.query_gemm(), st); break;
    case N_JFA:
    case N_JF:
    case N_JFIN:
    case N_J: {
      // N_J: at the end of step t, whose new state is in buffers 1 - p.  N_JFA / N_JF: the same GEMM for step t-1, at the head of
      // step t's launch - step t-1's outputs are this step's "previous" buffers p.  N_JFIN: io.slot carries the last step's parity.
      const bool head = node == N_JFA || node == N_JF;
      const int q = head ? s.p : 1 - s.p;
      const int jprec = (s.prec && use_frame(s.d)) ? PREC_F16S : PREC_F32;  // (the three-launch form keeps the projection on fp32)
      if (!proj_regw(h, s.prec)) {
        if (use_frame(s.d)) launch_gemm<A_PLAIN, EPI_PLAIN>(s.proj_gemm(q, jprec), st);
        else launch_gemm<A_PLAIN, EPI_PROJ>(s.proj_gemm(q, jprec), st);
        break;
      }
      // (same slabs, from the kernel that keeps its weight fragments in registers)
      ProjArgs pa = s.proj_role(q, jprec, head ? PROJ_HEAD : (node == N_JFIN ? PROJ_FINAL : PROJ_STEP));
      if (!head) {
        launch_proj(pa, st);
        break;
      }
      FrameArgs f = s.frame(false, node == N_JFA);  // (N_JF: no LSTM role behind the frame role, nobody to signal - no dep_cnt)
      pa.dep_cnt = f.wait_cnt = s.dep(DEP_PROJ);
      f.wait_n = proj_grid_size(32, pa.N, pa.ksplit);  // (the projection workgroups of one 32-row block)
      if (node == N_JF) launch_proj_frame(pa, f, st);
      else launch_proj_frame_lstm(pa, f, s.lstm(0, true), st);
      break;
    }
  }
}

// the two-role step: LJSpeech-type cell, either arithmetic mode
int overlap_level(const ttsdec_handle* h, int B) {
  const ttsdec_dims& d = h->d;
  if (!fused_supported(d.d_mel, d.r, pre_hidden(d), d.d_pre, d.d_ctx)) return 0;
  if (is_taco2(d)) {
    // Taco2DecoderCell (decoder_cell.py:116-136): its attention pass FOLLOWS both LSTMs, so only the first two-role launch
    // applies - frame || lstm_att, with the projection (which reads the two LSTM states there, not the context) as its head
    // role.  rdh config, us per step without / with (profiles/r03_w_taco2_level1.txt): split-fp16 B = 256 92.3 / 80.7, B = 64
    // 60.5 / 52.8, B = 1 54.6 / 46.9; exact fp32 B = 256 147.2 / 137.1, B = 64 73.0 / 80.6, B = 1 69.3 / 59.3 - the fp32 rule of the
    // other cell: not in the middle batch range.
    if (h->overlap >= 0) return h->overlap > 1 ? 1 : h->overlap;
    // (round 4, with the 32-row fp32 lean tile: exact fp32 B = 64 69.9 / 62.9, B = 128 86.9 / 82.7 - level 1 at every batch size now)
    return 1;
  }
  if (h->overlap >= 0) return h->overlap > 2 ? 2 : h->overlap;
  // Round 3 (after the sc1 hand-offs and the per-row-block counters; profiles/r03_t_levels_sweep.txt, us per step, levels 0 / 1 / 2):
  // split-fp16 B = 96 78.3 / 62.4 / 48.8, 192 80.1 / 64.8 / 59.3, 320 128.5 / 102.5 / 88.8, 384 131.1 / 110.0 / 98.3, 512 147.7 / 131.6 /
  // 117.8, 1024 - / 262.6 / 235.0, 2048 - / 504.1 / 455.8: level 2 at every batch size (round 2 had level 1 above 320, +-1.5 % then).
  if (lstm_prec(h)) return 2;
  // exact fp32 (round 4, after the loaders' buffer-descriptor DMA, the interleaved fragment reads and the 32-row lean tile whose
  // four MFMA waves share a block's K axis - fused_kernels.hip): us per step for levels 0 / 1 / 2: B = 32 68.7 / 60.4 / 50.5,
  // 40 68.6 / 63.4 / 60.0, 64 68.5 / 62.8 / 61.2, 80 96.3 / 79.4 / 65.4, 96 84.8 / 74.4 / 66.5, 112 86.0 / 81.5 / 91.2, 128 84.8 / 79.4 /
  // 88.0, 144 121.3 / 105.7 / 97.5, 176 121.6 / 106.7 / 98.3, 192 122.4 / 107.6 / 99.1, 256 - / - / 102.7 (round 3: level 0 between 32
  // and 192 utterances - its 64-row lean tile kept two of a CU's four matrix pipes busy there: B = 64 77.1 / 87.2 / 111.4).
  // Between 97 and 128 utterances the 64 x 16-unit tile has only two row blocks (128 workgroups): one two-role launch.
  return B <= 96 ? 2 : (B <= 128 ? 1 : 2);
}
// The projection as the head role of the next step's frame launch, wherever the register-weight kernel applies (split-fp16).
// us per step without / with it, same box: B = 1 43.0 / 39.8, B = 64 51.8 / 50.1, B = 128 54.2 / 53.5, B = 256 73.4 / 73.3 (there
// the frame role's chain is what the launch waits for, and it grows by what the projection's own launch cost).
// Round 3: also where the step runs one role per launch (N_JF: [proj | frame]) - us per step without / with it
// (profiles/r03_w_head_proj_level0.txt): exact fp32 B = 64 76.5 / 74.7, B = 128 103.0 / 100.9; sandra config (two frames per
// step) 63.4 / 63.3, B = 1 44.3 / 44.1 - the hop costs there what the launch did.
bool head_proj(const ttsdec_handle* h) {
  return proj_regw_shapes(h) && h->head_proj != 0;  // (-1 = default = on)
}
// The query as a job of the attention role (fused_kernels.hip attn_lstm_kernel): needs every attention-role workgroup resident
// at once - one per utterance, and they wait for each other's query tiles; they have the launch's lowest block ids, so that is
// at most what the device holds of that kernel at once (attn_lstm_resident_slots: CUs x the runtime's occupancy answer, 512 on
// an MI355X; a partitioned or smaller part answers for itself; a GPU shared with another process is what the bounded spin and
// Decoder.forward's fallback are for) - and whole K slices for the register-weight GEMM body.
// Measured, us per step with / without it (same box, profiles/r03_f_*, r03_t_query_role_large_batches.txt): split-fp16 B = 256 60.4 /
// 61.6, 128 49.4 / 50.0, 64 46.6 / 47.0, 320 83.9 / 89.7, 384 98.5 / 99.0, 448 108.5 / 106.9, 512 121.5 / 118.7; B = 32 44.1 / 42.5 (the
// roles do not share CUs there: the hop costs more than the launch), B = 1 175 / 38 (one workgroup would run all 32 tiles); exact
// fp32 B = 256 125.0 / 125.0, B = 32 58.6 / 55.3.  So: split-fp16, 64..384 utterances, at most one tile per workgroup (option
// query_role = 1 forces it wherever it is possible at all).
// Round 5, exact fp32 B = 256 beside the decoder LSTM's 64 x 16 tile (profiles/r05_a_*, same process, 5 interleaved rounds): with
// the lean attention pass (step_bodies.h ATTN_LEAN) 101.0 against 101.8 us per step; with the base pass 102.3 against 102.2 -
// the lean pass ends 2.5 us earlier, and that slack is what absorbs the query tiles.  So also: exact fp32, 192..256 utterances.
bool query_role(const ttsdec_handle* h, int B) {
  const ttsdec_dims& d = h->d;
  if (overlap_level(h, B) < 2 || h->query_role == 0) return false;
  if (B > attn_lstm_resident_slots(B, d.h_dec, d.d_ctx, lstm_prec(h) != 0)) return false;
  const int ps = proj_split(query_k(d));
  if (!(ps > 0 && ps <= kQuerySplit && !(d.h_att & 7))) return false;
  if (h->query_role > 0) return true;
  const bool range = lstm_prec(h) ? (B >= 64 && B <= 384) : (B >= 192 && B <= 256);
  return range && proj_grid_size(B, d.d_ctx, ps) <= B;
}
// The launch's name in profiles (ttsdec_profile_step / _loop; bench.py's byte model splits it at '+' into the roles it holds)
const char* node_name(Node n) {
  switch (n) {
    case N_P0: return "prenet0";
    case N_P1: return "prenet1";
    case N_F: return "prenet";
    case N_JF: return "proj+prenet";
    case N_FA: return "prenet+lstm_att";
    case N_JFA: return "proj+prenet+lstm_att";
    case N_A: return "lstm_att";
    case N_Q: return "query";
    case N_T: return "attention";
    case N_D: return "lstm_dec";
    case N_TD: return "attention+lstm_dec";
    case N_QTD: return "query+attention+lstm_dec";
    case N_J: return "proj";
    default: return nullptr;  // (N_FIN, N_JFIN, N_AG, N_DG: in no step order)
  }
}
StepOrder step_order(const ttsdec_handle* h, int B) {
  const ttsdec_dims& d = h->d;
  const int lv = overlap_level(h, B);
  const bool head = head_proj(h);  // step t-1's projection at the head of step t's first launch (implies use_frame)
  StepOrder o = {0, {}};
  auto add = [&](Node n) { o.nodes[o.n++] = n; };
  // the frame: PreNet layers alone, the frame kernel, or the frame kernel with lstm_att as the launch's second role
  if (lv) add(head ? N_JFA : N_FA);
  else if (use_frame(d)) add(head ? N_JF : N_F);
  else { add(N_P0); add(N_P1); }
  if (!lv) add(N_A);
  if (is_taco2(d)) {  // decoder_cell.py:116-136
    add(N_D); add(N_Q); add(N_T);
  } else if (lv < 2) {  // decoder_cell.py:185-192
    add(N_Q); add(N_T); add(N_D);
  } else if (!query_role(h, B)) {
    add(N_Q); add(N_TD);
  } else {
    add(N_QTD);  // the query as a job of the attention role's workgroups: two launches per step
  }
  if (!head) add(N_J);
  return o;
}

bool has_two_role_node(const StepOrder& order) {
  for (int i = 0; i < order.n; ++i)
    if (order.nodes[i] == N_FA || order.nodes[i] == N_JFA || order.nodes[i] == N_TD || order.nodes[i] == N_QTD) return true;
  return false;
}

// One step on a single stream, in the reference's order.  (For the Taco2 cell the attention
// kernel at the end of step t also produces the context bmm(w_t, memory) that step t+1 starts
// from, decoder_cell.py:118.)
void launch_step_serial(const ttsdec_handle* h, const StepBufs& sb, const StepIo& io0, hipStream_t st) {
  const StepOrder order = step_order(h, io0.B);
  StepIo io = io0;
  for (int i = 0; i < order.n; ++i) {
    io.node_pos = i;
    launch_node(h, sb, io, order.nodes[i], st);
  }
}

int ensure_streams(ttsdec_handle* h) {
  if (h->streams_ready) return TTSDEC_OK;
  if (hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking) != hipSuccess) return TTSDEC_ERR_HIP;
  h->streams_ready = true;
  return TTSDEC_OK;
}

void drop_graph(ttsdec_handle* h) {
  if (h->gexec) { (void)hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }
  if (h->graph) { (void)hipGraphDestroy(h->graph); h->graph = nullptr; }
}

// Captures kGraphSlots steps (+ the t_cur advance) once per (workspace, blob, B, L, mode).
int ensure_graph(ttsdec_handle* h, const StepBufs& sb, const void* ws, int B, int L) {
  const int prec = lstm_prec(h);
  if (h->gexec && h->g_ws == ws && h->g_blob == h->blob && h->g_B == B && h->g_L == L && h->g_prec == prec) return TTSDEC_OK;
  drop_graph(h);
  StepIo io;
  memset(&io, 0, sizeof(io));
  io.B = B; io.L = L; io.use_ctrl = true;
  if (hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeRelaxed) != hipSuccess) return TTSDEC_ERR_HIP;
  int rc = TTSDEC_OK;
  for (int i = 0; i < kGraphSlots; ++i) {
    io.slot = i;
    launch_step_serial(h, sb, io, h->cap_stream);
  }
  launch_advance(sb.ctrl, kGraphSlots, h->cap_stream);
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamEndCapture(h->cap_stream, &graph);
  if (e != hipSuccess || rc != TTSDEC_OK || graph == nullptr) {
    if (graph) (void)hipGraphDestroy(graph);
    h->hip_err = std::string("graph capture: ") + hipGetErrorString(e);
    (void)hipGetLastError();
    return TTSDEC_ERR_HIP;
  }
  hipGraphExec_t exec = nullptr;
  e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(graph);
    h->hip_err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
    return TTSDEC_ERR_HIP;
  }
  h->graph = graph; h->gexec = exec;
  h->g_ws = ws; h->g_blob = h->blob; h->g_B = B; h->g_L = L; h->g_prec = prec;
  return TTSDEC_OK;
}


// ---- options (include/ttsdec.h TTSDEC_OPT_*) ----
const char* const kOptionNames[TTSDEC_OPT_COUNT] = {"graph",     "overlap",    "chunk_a",          "chunk_b",     "proj_regw",
                                                    "head_proj", "query_role", "attn_form",        "profile_ablation", "debug_flags", "spin_limit"};
int& option_ref(ttsdec_handle* h, int o) {
  switch (o) {
    case TTSDEC_OPT_OVERLAP: return h->overlap;
    case TTSDEC_OPT_CHUNK_A: return h->opt_chunk_a;
    case TTSDEC_OPT_CHUNK_B: return h->opt_chunk_b;
    case TTSDEC_OPT_PROJ_REGW: return h->opt_proj_regw;
    case TTSDEC_OPT_HEAD_PROJ: return h->head_proj;
    case TTSDEC_OPT_QUERY_ROLE: return h->query_role;
    case TTSDEC_OPT_ATTN_FORM: return h->attn_form;
    case TTSDEC_OPT_PROFILE_ABLATION: return h->profile_ablation;
    case TTSDEC_OPT_DEBUG_FLAGS: return h->debug_flags;
    case TTSDEC_OPT_SPIN_LIMIT: return h->spin_limit;
    default: return h->opt_graph;
  }
}
void apply_env_options(ttsdec_handle* h) {
  if (const char* e = getenv("TTSDEC_OPTIONS")) {
    std::string str(e);
    size_t pos = 0;
    while (pos < str.size()) {
      size_t end = str.find(',', pos);
      if (end == std::string::npos) end = str.size();
      const std::string item = str.substr(pos, end - pos);
      const size_t eq = item.find('=');
      if (eq != std::string::npos) {
        const std::string name = item.substr(0, eq);
        for (int o = 0; o < TTSDEC_OPT_COUNT; ++o)
          if (name == kOptionNames[o]) {
            const long v = strtol(item.c_str() + eq + 1, nullptr, 10);  // (saturates; the string comes from the environment)
            option_ref(h, o) = v > 0x7fffffffL ? 0x7fffffff : (v < -0x7fffffffL ? -0x7fffffff : (int)v);
          }
      }
      pos = end + 1;
    }
  }
}
}  // namespace

extern "C" {

int ttsdec_version(void) { return TTSDEC_VERSION; }

const char* ttsdec_strerror(int code) {
  switch (code) {
    case TTSDEC_OK: return "ok";
    case TTSDEC_ERR_INVALID_ARG: return "invalid argument";
    case TTSDEC_ERR_DIMS: return "unsupported dimensions (feature sizes must be positive multiples of 4)";
    case TTSDEC_ERR_HIP: return "HIP runtime error";
    case TTSDEC_ERR_NOT_BOUND: return "no packed weights bound to the handle";
    case TTSDEC_ERR_WORKSPACE: return "workspace too small or not 256-byte aligned";
    case TTSDEC_ERR_DEVICE: return "no usable HIP device, or the current device is not the handle's";
    default: return "unknown error";
  }
}

const char* ttsdec_last_hip_error(const ttsdec_handle* h) { return last_hip_error(h); }

int ttsdec_create(const ttsdec_dims* dims, ttsdec_handle** out) {
  if (!dims || !out) return TTSDEC_ERR_INVALID_ARG;
  *out = nullptr;
  const int rc = check_dims(*dims);
  if (rc != TTSDEC_OK) return rc;
  ttsdec_handle* h = new (std::nothrow) ttsdec_handle();
  if (!h) return TTSDEC_ERR_INVALID_ARG;
  h->d = *dims;
  h->bl = make_blob_layout(*dims);
  if (!within_dma_reach(h->bl.total * sizeof(float))) {
    delete h;
    return TTSDEC_ERR_DIMS;
  }
  h->streams_ready = false;
  h->gexec = nullptr;
  h->graph = nullptr;
  h->g_ws = h->g_blob = nullptr;
  h->wmax_dec = h->wmax_post = 0.f;
  h->stamps_buf = nullptr;
  // Tuning / measurement options (include/ttsdec.h TTSDEC_OPT_*): library defaults, then the process-wide
  // TTSDEC_OPTIONS="name=value,..." (read here, once per handle), then ttsdec_set_option.
  // (A two-stream schedule that ran the LSTMs' early K segments beside the small critical-path kernels was built and
  // measured SLOWER on MI355X - 126 vs 96 us per step at B=256: the early GEMM's 256 workgroups hold every CU's LDS, so
  // the small kernels queue behind them - and was removed; see DESIGN.md.)
  for (int o = 0; o < TTSDEC_OPT_COUNT; ++o) option_ref(h, o) = -1;
  h->profile_ablation = 0; h->debug_flags = 0; h->spin_limit = 0; h->attn_form = 0;
  apply_env_options(h);
  h->device = current_device_or_minus1();
  *out = h;
  return TTSDEC_OK;
}

int ttsdec_destroy(ttsdec_handle* h) {
  if (!h) return TTSDEC_OK;
  drop_graph(h);
  if (h->streams_ready) (void)hipStreamDestroy(h->cap_stream);
  if (h->stamps_buf) (void)hipFree(h->stamps_buf);
  delete h;
  return TTSDEC_OK;
}

int ttsdec_num_weight_tensors(const ttsdec_handle* h) {
  if (!h) return TTSDEC_ERR_INVALID_ARG;
  if (h->d.postnet_layers <= 0) return TTSDEC_W_DECODER_COUNT;
  if (h->d.postnet_type == TTSDEC_POSTNET_TYPE_MEL2) return TTSDEC_W_DECODER_COUNT + TTSDEC_W_POSTNET2_PER_LAYER * h->d.postnet_layers;
  return TTSDEC_W_DECODER_COUNT + TTSDEC_W_POSTNET_PER_LAYER * h->d.postnet_layers + 1;
}

int ttsdec_set_precision(ttsdec_handle* h, int precision) { return set_precision(h, precision); }

int ttsdec_get_precision(const ttsdec_handle* h) {
  if (!h) return TTSDEC_ERR_INVALID_ARG;
  return lstm_prec(h) ? TTSDEC_PREC_SPLIT_F16 : TTSDEC_PREC_F32;
}

int ttsdec_set_option(ttsdec_handle* h, int option, int value) {
  if (!h || option < 0 || option >= TTSDEC_OPT_COUNT) return TTSDEC_ERR_INVALID_ARG;
  option_ref(h, option) = value;
  drop_graph(h);  // a captured graph bakes the launch sequence in
  return TTSDEC_OK;
}

int ttsdec_get_option(const ttsdec_handle* h, int option, int* value) {
  if (!h || !value || option < 0 || option >= TTSDEC_OPT_COUNT) return TTSDEC_ERR_INVALID_ARG;
  *value = option_ref(const_cast<ttsdec_handle*>(h), option);
  return TTSDEC_OK;
}

const char* ttsdec_option_name(int option) { return (option >= 0 && option < TTSDEC_OPT_COUNT) ? kOptionNames[option] : nullptr; }

size_t ttsdec_packed_bytes(const ttsdec_handle* h) { return h ? h->bl.total * sizeof(float) : 0; }

int ttsdec_pack_weights(ttsdec_handle* h, const float* const* src, int n_src, void* blob, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  // a NULL entry leaves that tensor's region zero (a module that owns only part of the
  // parameters - a bare decoder cell, a postnet - packs what it has)
  int rc = pack_begin(h, src, n_src, ttsdec_num_weight_tensors(h), true, blob, ttsdec_packed_bytes(h), st);
  if (rc != TTSDEC_OK) return rc;
  const ttsdec_dims& d = h->d;
  const BlobLayout& L = h->bl;
  float* b = static_cast<float*>(blob);
  const size_t Ha = d.h_att, Hd = d.h_dec, Mel = d.d_mel, R = d.r, Dp = proj_ld(d);
  auto hp = [&](size_t float_off) { return reinterpret_cast<f16*>(b + float_off); };
  auto from = [&](const Mat& m) { return m.src < 0 ? b + m.w : src[m.src]; };
  // every 16-bit form the record holds (a NULL source: none, like launch_copy) ...
  auto planes = [&](const Mat& m) {
    launch_split(from(m), hp(m.h), hp(m.l), m.n(), st);
    if (m.b != kAbsent) launch_to_bf16(from(m), b + m.b, m.n(), st);
    if (m.ch != kAbsent) launch_pack_lstm_chunked(from(m), hp(m.ch), hp(m.cl), (int)(m.rows / 4), (int)m.cols, st);
  };
  // ... and the range guard of the split-fp16 planes: max |w| of every matrix that has them, the decoder's into wmax[0], the Postnet's into [1]
  auto guard = [&](const Mat& m, int which) { launch_absmax(from(m), m.n(), b + L.wmax + which, st); };
  const Mat* const dec[7] = {&L.pre0, &L.pre1, &L.wq, &L.att_ih, &L.att_hh, &L.dec_ih, &L.dec_hh};
  for (const Mat* m : dec) {
    launch_copy(src[m->src], b + m->w, m->n(), st);
    planes(*m);
    guard(*m, 0);
  }
  launch_copy(src[TTSDEC_W_PRE0_B], b + L.pre0_b, L.pre0.rows, st);
  launch_copy(src[TTSDEC_W_PRE1_B], b + L.pre1_b, L.pre1.rows, st);
  if (src[TTSDEC_W_ATT_BIH] && src[TTSDEC_W_ATT_BHH])
    launch_add_vec(src[TTSDEC_W_ATT_BIH], src[TTSDEC_W_ATT_BHH], b + L.att_b, (int)(4 * Ha), st);
  if (src[TTSDEC_W_DEC_BIH] && src[TTSDEC_W_DEC_BHH])
    launch_add_vec(src[TTSDEC_W_DEC_BIH], src[TTSDEC_W_DEC_BHH], b + L.dec_b, (int)(4 * Hd), st);
  if (use_frame(d)) {  // (the frame kernel's shapes: frame_supported - d_mel = 80, Ph = 128 or 256)
    launch_split_frame_order(src[TTSDEC_W_PRE0_W], hp(L.pre0_ph), hp(L.pre0_pl), (int)L.pre0.rows, (int)L.pre0.cols, 0, st);
    launch_split_frame_order(src[TTSDEC_W_PRE1_W], hp(L.pre1_ph), hp(L.pre1_pl), (int)L.pre1.rows, (int)L.pre1.cols, 1, st);
  }
  launch_copy(src[TTSDEC_W_INIT_H0], b + L.h0a, Ha, st);
  launch_copy(src[TTSDEC_W_INIT_C0], b + L.c0a, Ha, st);
  launch_copy(src[TTSDEC_W_INIT_H1], b + L.h0d, Hd, st);
  launch_copy(src[TTSDEC_W_INIT_C1], b + L.c0d, Hd, st);
  // [fc_mel ; fc_stop] stacked on the output axis; the planes need both, the guard reads whatever was stacked
  launch_copy(src[TTSDEC_W_MEL_W], b + L.proj.w, R * Mel * Dp, st);
  launch_copy(src[TTSDEC_W_STOP_W], b + L.proj.w + R * Mel * Dp, R * Dp, st);
  launch_copy(src[TTSDEC_W_MEL_B], b + L.proj_b, R * Mel, st);
  launch_copy(src[TTSDEC_W_STOP_B], b + L.proj_b + R * Mel, R, st);
  if (src[TTSDEC_W_MEL_W] && src[TTSDEC_W_STOP_W]) planes(L.proj);
  guard(L.proj, 0);
  const int Hh = d.postnet_hidden, k = d.postnet_kernel;
  if (d.postnet_type == TTSDEC_POSTNET_TYPE_MEL2) {
    for (int i = 0; i < d.postnet_layers; ++i) {
      // per layer: conv1.w, bn1.{w,b,mean,var}, conv2.w, bn2.{w,b,mean,var}, conv3.w
      const float* const* ps = src + TTSDEC_W_DECODER_COUNT + TTSDEC_W_POSTNET2_PER_LAYER * i;
      for (int c = 0; c < 3; ++c) {
        const Mat& m = L.p2[i][c];
        if (!ps[5 * c]) return TTSDEC_ERR_INVALID_ARG;
        launch_conv1dfix_pack(ps[5 * c], b + m.w, (int)m.rows, (int)m.cols / k, k, st);
        planes(m);
        guard(m, 1);
      }
      for (int c = 0; c < 2; ++c) {
        const float* const* bn = ps + 1 + 5 * c;
        if (!bn[0] || !bn[1] || !bn[2] || !bn[3]) return TTSDEC_ERR_INVALID_ARG;
        launch_bn_fold(bn[0], bn[1], bn[2], bn[3], d.bn_eps, b + L.p2_alpha[i][c], b + L.p2_beta[i][c], Hh, st);
      }
    }
  } else if (d.postnet_layers > 0) {
    for (int i = 0; i < d.postnet_layers; ++i) {
      const float* const* ps = src + TTSDEC_W_DECODER_COUNT + TTSDEC_W_POSTNET_PER_LAYER * i;
      const Mat& m = L.conv[i];
      if (!ps[0] || !ps[1] || !ps[2] || !ps[3] || !ps[4]) return TTSDEC_ERR_INVALID_ARG;
      launch_conv_transpose(ps[0], b + m.w, Hh, (int)m.cols / k, k, st);
      planes(m);
      guard(m, 1);
      launch_bn_fold(ps[1], ps[2], ps[3], ps[4], d.bn_eps, b + L.conv_alpha[i], b + L.conv_beta[i], Hh, st);
    }
    launch_copy(src[L.fc.src], b + L.fc.w, L.fc.n(), st);
    planes(L.fc);
    guard(L.fc, 1);
  }
  rc = pack_end(h, b);
  if (rc != TTSDEC_OK) return rc;
  return read_wmax(h, st);
}

int ttsdec_bind_weights(ttsdec_handle* h, const void* blob) {
  if (!h || !blob) return TTSDEC_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(blob) & 255) return TTSDEC_ERR_WORKSPACE;
  const int rc = check_device(h);
  if (rc != TTSDEC_OK) return rc;
  h->blob = static_cast<const float*>(blob);
  return read_wmax(h, nullptr);  // (synchronises the null stream: the blob must be complete, e.g. the broadcast done)
}

size_t ttsdec_workspace_bytes(const ttsdec_handle* h, int B, int L) {
  if (!h || B <= 0 || L <= 0) return 0;
  Carver cv{nullptr};
  return carve(cv, h->d, B, L).bytes;
}

// stamp_loop (ttsdec_profile_loop): every step kernel records its start time (common.h loop_stamp) in the workspace
static int decode_impl(ttsdec_handle* h, const float* memory, int B, int L, int t_begin, int n_steps, int t_stride,
                       float stop_threshold, int check_stop, int dropout_mode, const uint8_t* masks, uint64_t seed,
                       const float* teacher, int teacher_T, const uint8_t* teacher_flags, float* y, float* s, float* w,
                       int32_t* T_out, void* workspace, size_t workspace_bytes, void* stream, bool stamp_loop,
                       int32_t* stop_steps = nullptr) {
  if (!h || !memory || !y || !s || !w || !workspace) return TTSDEC_ERR_INVALID_ARG;
  if ((check_stop == 2) != (stop_steps != nullptr)) return TTSDEC_ERR_INVALID_ARG;  // (2: ttsdec_decode_each only)
  if (B <= 0 || L <= 0 || t_begin < 0 || n_steps < 0 || t_stride < n_steps) return TTSDEC_ERR_INVALID_ARG;
  if (dropout_mode < TTSDEC_DROPOUT_OFF || dropout_mode > TTSDEC_DROPOUT_PHILOX) return TTSDEC_ERR_INVALID_ARG;
  if (dropout_mode == TTSDEC_DROPOUT_MASKS && !masks) return TTSDEC_ERR_INVALID_ARG;
  if (dropout_mode == TTSDEC_DROPOUT_PHILOX && h->d.p_dropout != 0.5f) return TTSDEC_ERR_INVALID_ARG;  // one keep BIT per unit
  if (teacher && (!teacher_flags || teacher_T < (t_begin + n_steps - 1) * h->d.r)) return TTSDEC_ERR_INVALID_ARG;
  if (!h->blob) return TTSDEC_ERR_NOT_BOUND;
  int rc = check_device(h);
  if (rc != TTSDEC_OK) return rc;
  Carver cv{static_cast<float*>(workspace)};
  const StepBufs sb = carve(cv, h->d, B, L);
  if (!sb.bytes || workspace_bytes < sb.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255)) return TTSDEC_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ttsdec_dims& d = h->d;

  if (t_begin & 1) return TTSDEC_ERR_INVALID_ARG;  // buffer parity is tied to the step index
  rc = ensure_streams(h);
  if (rc != TTSDEC_OK) return rc;

  if (t_begin == 0) {
    InitArgs ia;
    ia.ctrl = sb.ctrl;
    ia.h0_att = h->blob + h->bl.h0a; ia.c0_att = h->blob + h->bl.c0a;
    ia.h0_dec = h->blob + h->bl.h0d; ia.c0_dec = h->blob + h->bl.c0d;
    ia.h_att = sb.h_att[0]; ia.c_att = sb.c_att; ia.h_dec = sb.h_dec[0]; ia.c_dec = sb.c_dec;
    ia.ctx = sb.ctx; ia.w = sb.w[0]; ia.ynext = sb.ynext;
    ia.h_att_h = sb.h_att_h[0]; ia.h_att_l = sb.h_att_l[0]; ia.h_dec_h = sb.h_dec_h[0]; ia.h_dec_l = sb.h_dec_l[0];
    ia.ctx_h = sb.ctx_h; ia.ctx_l = sb.ctx_l;
    ia.out_mpad = act_mpad(h, B);
    ia.memory = is_taco2(d) ? memory : nullptr;
    ia.B = B; ia.L = L; ia.D = d.d_ctx; ia.Ha = d.h_att; ia.Hd = d.h_dec; ia.d_mel = d.d_mel;
    ia.stop_steps = stop_steps;
    launch_init(ia, st);
  }
  CallArgs ca;
  ca.t_begin = t_begin; ca.n_steps = n_steps; ca.t_stride = t_stride; ca.check_stop = check_stop;
  ca.dropout_mode = dropout_mode; ca.teacher_T = teacher_T; ca.stop_thr = stop_threshold; ca.seed = seed;
  ca.memory = memory; ca.masks = masks; ca.teacher = teacher; ca.teacher_flags = teacher_flags;
  ca.y = y; ca.s = s; ca.w = w;
  ca.debug_flags = h->debug_flags > 0 ? h->debug_flags : 0;
  ca.spin_limit = h->spin_limit > 0 ? h->spin_limit : kRoleSpinLimit;
  ca.loop_stamps = stamp_loop ? sb.loop_stamps : nullptr;
  ca.stop_steps = stop_steps; ca.stop_rows = B;
  // measurement only: TTSDEC_STAMPS=<file> collects per-workgroup time stamps of the two-role launches of the
  // call's last step and writes them to <file> (synchronises; never set in production)
  const char* stamp_file = getenv("TTSDEC_STAMPS");
  ca.stamps = nullptr;
  if (stamp_file && *stamp_file) {  // (the buffer belongs to the handle, hence to its device; freed by ttsdec_destroy)
    if (!h->stamps_buf) { HIP_TRY(h, hipMalloc(&h->stamps_buf, kStampKinds * 1024 * 8 * sizeof(unsigned long long))); }
    HIP_TRY(h, hipMemsetAsync(h->stamps_buf, 0, kStampKinds * 1024 * 8 * sizeof(unsigned long long), st));
    ca.stamps = h->stamps_buf;
  }
  launch_set_call(sb.ctrl, ca, st);
  HIP_TRY(h, hipMemsetAsync(sb.dep, 0, sb.dep_bytes, st));  // arrival counters count from the call's first step

  StepIo io;
  memset(&io, 0, sizeof(io));
  io.B = B; io.L = L; io.use_ctrl = true;
  if (h->use_graph() && n_steps >= kGraphSlots / 2) {
    rc = ensure_graph(h, sb, workspace, B, L);
    if (rc != TTSDEC_OK) return rc;
    for (int done = 0; done < n_steps; done += kGraphSlots) HIP_TRY(h, hipGraphLaunch(h->gexec, st));
  } else {
    for (int i = 0; i < n_steps; ++i) {
      io.slot = i;
      launch_step_serial(h, sb, io, st);
    }
  }
  io.node_pos = kLoopStampNodes - 1;     // (the end-of-call launches below stamp a node index no step launch uses)
  if (head_proj(h) && n_steps > 0) {  // (that step order leaves each step's projection to the NEXT step's launch)
    io.slot = (n_steps - 1) & 1;        // buffer parity of the call's last step (t_begin is even)
    launch_node(h, sb, io, N_JFIN, st);
  }
  if (use_frame(d)) launch_node(h, sb, io, N_FIN, st);  // the last step's frame: y, s, stop rule, next input
  launch_finish(sb.ctrl, T_out, st);
  if (ca.stamps) {
    std::string buf(kStampKinds * 1024 * 8 * sizeof(unsigned long long), '\0');
    HIP_TRY(h, hipStreamSynchronize(st));
    HIP_TRY(h, hipMemcpy(&buf[0], ca.stamps, buf.size(), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(stamp_file, "wb")) { fwrite(buf.data(), 1, buf.size(), f); fclose(f); }
  }
  return record_hip_error(h, "decode");
}

int ttsdec_decode(ttsdec_handle* h, const float* memory, int B, int L, int t_begin, int n_steps, int t_stride,
                  float stop_threshold, int check_stop, int dropout_mode, const uint8_t* masks, uint64_t seed,
                  const float* teacher, int teacher_T, const uint8_t* teacher_flags, float* y, float* s, float* w,
                  int32_t* T_out, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_impl(h, memory, B, L, t_begin, n_steps, t_stride, stop_threshold, check_stop != 0, dropout_mode, masks, seed, teacher, teacher_T,
                     teacher_flags, y, s, w, T_out, workspace, workspace_bytes, stream, false);
}

int ttsdec_decode_each(ttsdec_handle* h, const float* memory, int B, int L, int t_begin, int n_steps, int t_stride,
                       float stop_threshold, int dropout_mode, const uint8_t* masks, uint64_t seed, const float* teacher,
                       int teacher_T, const uint8_t* teacher_flags, float* y, float* s, float* w, int32_t* stop_steps,
                       int32_t* T_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (teacher || !stop_steps) return TTSDEC_ERR_INVALID_ARG;  // (free-running only: a teacher-forced decode has no stop rule)
  return decode_impl(h, memory, B, L, t_begin, n_steps, t_stride, stop_threshold, 2, dropout_mode, masks, seed, nullptr, teacher_T,
                     teacher_flags, y, s, w, T_out, workspace, workspace_bytes, stream, false, stop_steps);
}

int ttsdec_profile_loop(ttsdec_handle* h, const float* memory, int B, int L, int n_steps, int dropout_mode, const uint8_t* masks,
                        uint64_t seed, float* y, float* s, float* w, int32_t* T_out, void* workspace, size_t workspace_bytes, void* stream,
                        float* ms_out, const char** names_out, int n_out, int* n_kernels, float* step_ms) {
  if (!h || !ms_out || !workspace || n_steps < 2 * kGraphSlots || n_steps % kGraphSlots) return TTSDEC_ERR_INVALID_ARG;
  if (!h->use_graph()) return TTSDEC_ERR_INVALID_ARG;  // (it is the replayed graph this function looks into)
  const StepOrder order = step_order(h, B);
  if (n_kernels) *n_kernels = order.n;
  if (n_out < order.n || order.n >= kLoopStampNodes) return TTSDEC_ERR_INVALID_ARG;
  Carver cv{static_cast<float*>(workspace)};
  const StepBufs sb = carve(cv, h->d, B, L);
  if (!sb.bytes || workspace_bytes < sb.bytes) return TTSDEC_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = decode_impl(h, memory, B, L, 0, n_steps, n_steps, -1e30f, 0, dropout_mode, masks, seed, nullptr, 0, nullptr, y, s, w, T_out, workspace,
                       workspace_bytes, stream, true);
  if (rc != TTSDEC_OK) return rc;
  unsigned long long t[kLoopStampSlots * kLoopStampNodes];
  HIP_TRY(h, hipStreamSynchronize(st));
  HIP_TRY(h, hipMemcpy(t, sb.loop_stamps, sizeof(t), hipMemcpyDeviceToHost));
  // the LAST replay's start times: slots 0 .. kGraphSlots-1; a launch's span = the next launch's start - its own
  // (s_memrealtime ticks of 10 ns); the last launch of the last slot has no successor inside the replay and is left out
  double total = 0.0;
  for (int k = 0; k < order.n; ++k) {
    double sum = 0.0;
    int cnt = 0;
    for (int i = 0; i < kGraphSlots; ++i) {
      const bool last = k + 1 == order.n;
      if (last && i + 1 == kGraphSlots) continue;
      const unsigned long long a = t[i * kLoopStampNodes + k], b = last ? t[(i + 1) * kLoopStampNodes] : t[i * kLoopStampNodes + k + 1];
      if (a == 0 || b <= a) return TTSDEC_ERR_INVALID_ARG;  // (a launch that did not stamp: not a step kernel this function knows)
      sum += (double)(b - a) * 1e-5;  // ms
      ++cnt;
    }
    ms_out[k] = (float)(sum / cnt);
    if (names_out) names_out[k] = node_name(order.nodes[k]);
    total += ms_out[k];
  }
  if (step_ms) *step_ms = (float)total;
  return TTSDEC_OK;
}

// The Postnet's workspace (carved as layout.h's Carver comment says): two activation buffers (fp32, or hi + lo fp16 planes, or one
// bf16 plane), then MelPostnet: the 16-bit planes of the input; MelPostnet2: the fp32 residual stream and its 16-bit planes, both
// ping-pong
struct PostnetWs {
  char *act[2], *yin, *xbuf[2], *xpl[2];
};
static PostnetWs carve_postnet(Carver& cv, const ttsdec_dims& d, size_t M) {
  auto take = [&](size_t nfloats) { return reinterpret_cast<char*>(cv.take(nfloats)); };
  PostnetWs w = {};
  for (char*& a : w.act) a = take(M * d.postnet_hidden);
  if (d.postnet_type != TTSDEC_POSTNET_TYPE_MEL2) {
    w.yin = take(M * d.d_mel);
    return w;
  }
  for (char*& x : w.xbuf) x = take(M * d.d_mel);
  for (char*& x : w.xpl) x = take(M * d.d_mel);
  return w;
}

size_t ttsdec_postnet_workspace_bytes(const ttsdec_handle* h, int B, int T) {
  if (!h || B <= 0 || T <= 0 || h->d.postnet_layers <= 0) return 0;
  Carver cv{nullptr};
  carve_postnet(cv, h->d, (size_t)B * T);
  return cv.bytes();
}

// lengths != nullptr (ttsdec_postnet_ragged): every conv layer's input - y and each hidden activation, in whatever form the
// precision keeps it - is zeroed at frames >= lengths[b] by a write-only pass over the padding (launch_zero_tail), so each
// utterance sees the zero padding it would see alone; the conv kernels, the 256-wide schedule included, are the same launches.
// lengths == nullptr adds no launch and no copy: ttsdec_postnet as it always was.
static int postnet_impl(ttsdec_handle* h, const float* y, const int32_t* lengths, int B, int T, int precision, float* y_post,
                        void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !y || !y_post || !workspace || B <= 0 || T <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (lengths && B > 65535) return TTSDEC_ERR_INVALID_ARG;  // (launch_zero_tail: one grid row per utterance)
  if (h->d.postnet_layers <= 0) return TTSDEC_ERR_DIMS;
  if (precision != TTSDEC_POSTNET_F32 && precision != TTSDEC_POSTNET_BF16 && precision != TTSDEC_POSTNET_SPLIT_F16)
    return TTSDEC_ERR_INVALID_ARG;
  if (!h->blob) return TTSDEC_ERR_NOT_BOUND;
  int rc = check_device(h);
  if (rc != TTSDEC_OK) return rc;
  if (workspace_bytes < ttsdec_postnet_workspace_bytes(h, B, T) || (reinterpret_cast<uintptr_t>(workspace) & 255))
    return TTSDEC_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ttsdec_dims& d = h->d;
  const BlobLayout& L = h->bl;
  // 16-bit modes need whole 16-byte columns of 16-bit elements in every K segment
  int prec = PREC_F32;
  if (!((d.d_mel | d.postnet_hidden) & 7)) {
    if (precision == TTSDEC_POSTNET_BF16) prec = PREC_BF16;
    if (precision == TTSDEC_POSTNET_SPLIT_F16 && h->wmax_post < kSplitMax) prec = PREC_F16S;
  }
  const size_t M = (size_t)B * T;
  Carver cv{static_cast<float*>(workspace)};
  const PostnetWs pw = carve_postnet(cv, d, M);
  const int Hh = d.postnet_hidden;
  // one layer on input a [M, cin]: a conv over `taps` frames (A_CONV), or taps = 0: a plain GEMM
  auto layer = [&](Planes a, int cin, int taps, const Mat& w) {
    const Planes wp = weight(w, h->blob, prec);
    return taps ? conv_gemm_args(a, wp, prec, (int)M, T, cin, taps, (int)w.rows) : gemm_args(a, cin, wp, prec, (int)M, (int)w.rows, cin);
  };
  // ragged batches: the tail of a [M, C] activation in the form of `prec` (fp32 rows, a bf16 plane, or a hi / lo fp16 plane pair)
  const int ew = prec == PREC_F32 ? 1 : 2;  // elements per 32-bit word
  auto mask = [&](Planes a, int C) {
    if (!lengths) return;
    launch_zero_tail(const_cast<void*>(a.p0), lengths, B, T, (size_t)T * C / ew, C / ew, 1, st);
    if (a.p1 != a.p0) launch_zero_tail(const_cast<void*>(a.p1), lengths, B, T, (size_t)T * C / ew, C / ew, 1, st);
  };
  auto mask_f32 = [&](float* a) {
    if (lengths) launch_zero_tail(a, lengths, B, T, (size_t)T * d.d_mel, d.d_mel, 1, st);
  };
  // y as the first layer reads it; ragged and exact fp32: a copy in `buf`, since y itself is the caller's
  auto first_input = [&](char* buf) {
    if (lengths && prec == PREC_F32) {
      launch_copy(y, reinterpret_cast<float*>(buf), M * d.d_mel, st);
      return Planes{buf, buf};
    }
    return act_input(prec, y, buf, M * d.d_mel, st);
  };

  if (d.postnet_type == TTSDEC_POSTNET_TYPE_MEL2) {
    // MelPostnet2.forward (modules.py:213-216): x = x + conv3(lrelu(BN(conv2(lrelu(BN(conv1(x))))))) per layer;
    // the fp32 residual stream and its 16-bit planes ping-pong in xbuf / xpl
    const float* xcur = y;
    Planes x = first_input(pw.xpl[1]);
    mask(x, d.d_mel);  // (the residual stream xcur may stay y: what it adds past an utterance's end is zeroed with the sum)
    for (int i = 0; i < d.postnet_layers; ++i) {
      Planes a = x;
      for (int c = 0; c < 2; ++c) {  // conv1 / conv2 + BN + LeakyReLU
        GemmArgs g = layer(a, c ? Hh : d.d_mel, d.postnet_kernel, L.p2[i][c]);
        g.alpha = h->blob + L.p2_alpha[i][c]; g.beta = h->blob + L.p2_beta[i][c];
        a = set_output(g, prec, pw.act[c], M * Hh);
        launch_gemm<A_CONV, EPI_BN_LRELU>(g, st);
        mask(a, Hh);
      }
      GemmArgs g = layer(a, Hh, d.postnet_kernel, L.p2[i][2]);  // conv3 + residual
      g.resid = xcur;
      const bool last = (i == d.postnet_layers - 1);
      float* xnew = last ? y_post : reinterpret_cast<float*>(pw.xbuf[i & 1]);
      if (!last) x = set_output(g, prec, prec == PREC_F32 ? reinterpret_cast<char*>(xnew) : pw.xpl[i & 1], M * d.d_mel);
      g.out = xnew;  // (the 16-bit modes keep the fp32 stream beside the planes: the next layer's residual)
      launch_gemm<A_CONV, EPI_RESIDUAL>(g, st);
      mask_f32(xnew);
      if (!last && prec != PREC_F32) mask(x, d.d_mel);
      xcur = xnew;
    }
    return record_hip_error(h, "postnet2");
  }

  Planes in = first_input(pw.yin);
  mask(in, d.d_mel);
  for (int i = 0; i < d.postnet_layers; ++i) {
    GemmArgs g = layer(in, i ? Hh : d.d_mel, d.postnet_kernel, L.conv[i]);
    g.alpha = h->blob + L.conv_alpha[i]; g.beta = h->blob + L.conv_beta[i];
    char* o = pw.act[i & 1];
    in = set_output(g, prec, o, M * Hh);
    // the wide hidden -> hidden layers on the 256 x 256 schedule (conv256.hip) where the shape is that kernel's - exact fp32 and
    // bf16; TTSDEC_CONV256=0 keeps the shared tile (measurement)
    static const bool use256 = [] { const char* e = getenv("TTSDEC_CONV256"); return !(e && e[0] == '0'); }();
    if (use256 && prec == PREC_F32 &&
        launch_conv256_f32(static_cast<const float*>(g.a.p0), static_cast<const float*>(g.W), g.alpha, g.beta, g.out, (int)M, T, g.Cin, g.taps, Hh, st)) {
      mask(in, Hh);
      continue;
    }
    if (use256 && prec == PREC_BF16 && launch_conv256_bf16(g.a.p0, g.W, g.alpha, g.beta, o, (int)M, T, g.Cin, g.taps, Hh, st)) {
      mask(in, Hh);
      continue;
    }
    launch_gemm<A_CONV, EPI_BN_ISRU>(g, st);
    mask(in, Hh);
  }
  GemmArgs g = layer(in, Hh, 0, L.fc);
  g.resid = y; g.out = y_post;
  launch_gemm<A_PLAIN, EPI_RESIDUAL>(g, st);
  mask_f32(y_post);
  return record_hip_error(h, "postnet");
}

int ttsdec_postnet(ttsdec_handle* h, const float* y, int B, int T, int precision, float* y_post, void* workspace,
                   size_t workspace_bytes, void* stream) {
  return postnet_impl(h, y, nullptr, B, T, precision, y_post, workspace, workspace_bytes, stream);
}

int ttsdec_postnet_ragged(ttsdec_handle* h, const float* y, const int32_t* lengths, int B, int T, int precision, float* y_post,
                          void* workspace, size_t workspace_bytes, void* stream) {
  return postnet_impl(h, y, lengths, B, T, precision, y_post, workspace, workspace_bytes, stream);
}

int ttsdec_zero_tail(ttsdec_handle* h, float* x, const int32_t* lengths, int B, int T, int64_t batch_stride, int C, int len_div,
                     void* stream) {
  if (!h || !x || !lengths || B <= 0 || B > 65535 || T <= 0 || C <= 0 || len_div <= 0 || batch_stride < (int64_t)T * C)
    return TTSDEC_ERR_INVALID_ARG;
  const int rc = check_device(h);
  if (rc != TTSDEC_OK) return rc;
  launch_zero_tail(x, lengths, B, T, (size_t)batch_stride, C, len_div, static_cast<hipStream_t>(stream));
  return record_hip_error(h, "zero_tail");
}

int ttsdec_cell_step(ttsdec_handle* h, const float* x, const float* memory, int B, int L, float* w, float* ctx,
                     float* h_att, float* c_att, float* h_dec, float* c_dec, int dropout_mode, const uint8_t* masks,
                     uint64_t seed, int step, float* x_dec, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !x || !memory || !w || !ctx || !h_att || !c_att || !h_dec || !c_dec || !x_dec || !workspace)
    return TTSDEC_ERR_INVALID_ARG;
  if (B <= 0 || L <= 0 || step < 0) return TTSDEC_ERR_INVALID_ARG;
  if (dropout_mode == TTSDEC_DROPOUT_MASKS && !masks) return TTSDEC_ERR_INVALID_ARG;
  if (dropout_mode == TTSDEC_DROPOUT_PHILOX && h->d.p_dropout != 0.5f) return TTSDEC_ERR_INVALID_ARG;
  if (!h->blob) return TTSDEC_ERR_NOT_BOUND;
  int rc = check_device(h);
  if (rc != TTSDEC_OK) return rc;
  Carver cv{static_cast<float*>(workspace)};
  const StepBufs sb = carve(cv, h->d, B, L);
  if (!sb.bytes || workspace_bytes < sb.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255)) return TTSDEC_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ttsdec_dims& d = h->d;
  const size_t b = (size_t)B;
  const int p = step & 1;
  const bool t2 = is_taco2(d);
  // caller state -> workspace (the step kernels ping-pong h and w)
  launch_copy(x, sb.ynext, b * d.d_mel, st);
  if (!t2) launch_copy(ctx, sb.ctx, b * d.d_ctx, st);
  launch_copy(w, sb.w[p], b * L, st);
  launch_copy(h_att, sb.h_att[p], b * d.h_att, st);
  launch_copy(c_att, sb.c_att, b * d.h_att, st);
  launch_copy(h_dec, sb.h_dec[p], b * d.h_dec, st);
  launch_copy(c_dec, sb.c_dec, b * d.h_dec, st);
  const int prec = lstm_prec(h);
  const int mp = act_mpad(h, B);
  if (mp) {
    if (!t2) launch_split_chunked(ctx, sb.ctx_h, sb.ctx_l, B, d.d_ctx, mp, st);
    launch_split_chunked(h_att, sb.h_att_h[p], sb.h_att_l[p], B, d.h_att, mp, st);
    launch_split_chunked(h_dec, sb.h_dec_h[p], sb.h_dec_l[p], B, d.h_dec, mp, st);
  } else if (prec) {
    if (!t2) launch_split(ctx, sb.ctx_h, sb.ctx_l, b * d.d_ctx, st);
    launch_split(h_att, sb.h_att_h[p], sb.h_att_l[p], b * d.h_att, st);
    launch_split(h_dec, sb.h_dec_h[p], sb.h_dec_l[p], b * d.h_dec, st);
  }
  StepIo io;
  memset(&io, 0, sizeof(io));
  io.memory = memory; io.B = B; io.L = L; io.t = step; io.t_rel = 0; io.t_stride = 1;
  io.dropout_mode = dropout_mode; io.masks = masks; io.seed = seed;
  io.use_ctrl = false;
  if (t2) {
    // Taco2DecoderCell: ctx = bmm(w_prev, memory) first (decoder_cell.py:118), then both LSTMs,
    // then the weight update; the ctx handed back is the one the LSTMs consumed
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.memory = memory; a.w_prev = sb.w[p]; a.w_new = sb.w[1 - p]; a.ctx = sb.ctx; a.ctx_only = 1;
    if (prec) { a.ctx_h = sb.ctx_h; a.ctx_l = sb.ctx_l; a.out_mpad = mp; }
    a.B = B; a.L = L; a.D = d.d_ctx; a.t_stride = 1;
    launch_attn(a, st);
    if (use_frame(d)) launch_node(h, sb, io, N_F, st);  // (io.finalize = 0: the input frame is x itself)
    else { launch_node(h, sb, io, N_P0, st); launch_node(h, sb, io, N_P1, st); }
    launch_node(h, sb, io, N_A, st);
    launch_node(h, sb, io, N_D, st);
    launch_copy(sb.ctx, ctx, b * d.d_ctx, st);
    launch_node(h, sb, io, N_Q, st);
    launch_node(h, sb, io, N_T, st);
  } else {
    // the projection (fc_mel / fc_stop) belongs to Decoder, not to the cell
    if (use_frame(d)) launch_node(h, sb, io, N_F, st);
    else { launch_node(h, sb, io, N_P0, st); launch_node(h, sb, io, N_P1, st); }
    const Node cell_nodes[4] = {N_A, N_Q, N_T, N_D};
    for (Node n : cell_nodes) launch_node(h, sb, io, n, st);
    launch_copy(sb.ctx, ctx, b * d.d_ctx, st);
  }
  launch_copy(sb.w[1 - p], w, b * L, st);
  launch_copy(sb.h_att[1 - p], h_att, b * d.h_att, st);
  launch_copy(sb.c_att, c_att, b * d.h_att, st);
  launch_copy(sb.h_dec[1 - p], h_dec, b * d.h_dec, st);
  launch_copy(sb.c_dec, c_dec, b * d.h_dec, st);
  if (t2) {
    // x_dec = cat[h0, h1, zeros_like(ctx)] (decoder_cell.py:136)
    const size_t ld = (size_t)(d.h_att + d.h_dec + d.d_ctx) * sizeof(float);
    HIP_TRY(h, hipMemsetAsync(x_dec, 0, ld * b, st));
    HIP_TRY(h, hipMemcpy2DAsync(x_dec, ld, sb.h_att[1 - p], (size_t)d.h_att * sizeof(float), (size_t)d.h_att * sizeof(float), b,
                                hipMemcpyDeviceToDevice, st));
    HIP_TRY(h, hipMemcpy2DAsync(x_dec + d.h_att, ld, sb.h_dec[1 - p], (size_t)d.h_dec * sizeof(float),
                                (size_t)d.h_dec * sizeof(float), b, hipMemcpyDeviceToDevice, st));
  } else {
    // x_dec = cat[h_dec, ctx] (decoder_cell.py:192)
    const size_t ld = (size_t)(d.h_dec + d.d_ctx) * sizeof(float);
    HIP_TRY(h, hipMemcpy2DAsync(x_dec, ld, sb.h_dec[1 - p], (size_t)d.h_dec * sizeof(float), (size_t)d.h_dec * sizeof(float), b,
                                hipMemcpyDeviceToDevice, st));
    HIP_TRY(h, hipMemcpy2DAsync(x_dec + d.h_dec, ld, sb.ctx, (size_t)d.d_ctx * sizeof(float), (size_t)d.d_ctx * sizeof(float), b,
                                hipMemcpyDeviceToDevice, st));
  }
  return record_hip_error(h, "cell_step");
}

int ttsdec_profile_step(ttsdec_handle* h, const float* memory, int B, int L, int iters, int dropout_mode,
                        const uint8_t* masks, uint64_t seed, float* y, float* s, float* w, void* workspace,
                        size_t workspace_bytes, void* stream, float* ms_out, const char** names_out, int n_out,
                        int* n_kernels) {
  if (!h || !memory || !y || !s || !w || !workspace || !ms_out || iters <= 0) return TTSDEC_ERR_INVALID_ARG;
  const StepOrder order = step_order(h, B);
  if (n_kernels) *n_kernels = order.n;
  if (n_out < order.n) return TTSDEC_ERR_INVALID_ARG;
  if (dropout_mode == TTSDEC_DROPOUT_MASKS && !masks) return TTSDEC_ERR_INVALID_ARG;
  if (dropout_mode == TTSDEC_DROPOUT_PHILOX && h->d.p_dropout != 0.5f) return TTSDEC_ERR_INVALID_ARG;
  if (!h->blob) return TTSDEC_ERR_NOT_BOUND;
  int rc = check_device(h);
  if (rc != TTSDEC_OK) return rc;
  Carver cv{static_cast<float*>(workspace)};
  const StepBufs sb = carve(cv, h->d, B, L);
  if (!sb.bytes || workspace_bytes < sb.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255)) return TTSDEC_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  StepIo io;
  memset(&io, 0, sizeof(io));
  io.memory = memory; io.B = B; io.L = L; io.t = 0; io.t_rel = 0; io.t_stride = 1;
  io.dropout_mode = dropout_mode; io.masks = masks; io.seed = seed;
  io.y = y; io.s = s; io.w = w; io.use_ctrl = false;
  io.t = 1; io.t_rel = 1; io.t_stride = 2; io.finalize = 1;  // a mid-sequence step: the frame kernel also finishes step 0's frame
  io.dbg = h->profile_ablation > 0 ? h->profile_ablation : 0;  // measurement only (option "profile_ablation")
  hipEvent_t e0, e1;
  HIP_TRY(h, hipEventCreate(&e0));
  HIP_TRY(h, hipEventCreate(&e1));
  // the step's own launches, then (two-role step only, when the caller left room) each role on its own:
  // what the partner of a two-role launch costs alone
  Node nodes[kMaxKernelsPerStep + 4];
  const char* names[kMaxKernelsPerStep + 4];
  int nn = 0;
  for (int k = 0; k < order.n; ++k) { nodes[nn] = order.nodes[k]; names[nn++] = node_name(order.nodes[k]); }
  if (!is_taco2(h->d) && has_two_role_node(order) && n_out >= order.n + 4) {
    const Node extra[4] = {N_F, N_AG, N_T, N_DG};
    const char* extra_names[4] = {"prenet(alone)", "lstm_att_lean(alone)", "attention(alone)", "lstm_dec_lean(alone)"};
    for (int k = 0; k < 4; ++k) { nodes[nn] = extra[k]; names[nn++] = extra_names[k]; }
  }
  if (n_kernels) *n_kernels = nn;
  for (int k = 0; k < nn; ++k) {
    for (int i = 0; i < 3; ++i) launch_node(h, sb, io, nodes[k], st);  // warm
    HIP_TRY(h, hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) launch_node(h, sb, io, nodes[k], st);
    HIP_TRY(h, hipEventRecord(e1, st));
    HIP_TRY(h, hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&ms, e0, e1));
    ms_out[k] = ms / iters;
    if (names_out) names_out[k] = names[k];
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return record_hip_error(h, "profile_step");
}

}  // extern "C"
