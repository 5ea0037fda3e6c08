// C ABI of the VITS2 HiFi-GAN generator (latent z -> waveform): Generator.forward, vits2/models.py:900-974, with ResBlock1
// (modules.py:221-315) - the `self.dec(...)` of SynthesizerTrn.infer, models.py:1322.
//
// Every conv is one implicit-im2col GEMM of the GEMM core (decode_kernels.hip, A_CONV_DIL + EPI_LRELU2, exact fp32) over
// channel-last activations [B*T, C]:
//   conv_pre         7 taps; epilogue  lrelu(conv_pre(z) [+ cond(g)], 0.1)            (the plain value is never read)
//   ups[i]           ConvTranspose1d(Cin, Cout, k = 2u, stride u, padding u/2) as a polyphase 3-tap conv: output frame
//                    u*q + r sees input frames q-1, q, q+1 through kernel index j = u*(q - q_in) + r + u/2 (two of the three
//                    taps are valid per phase, the third is packed as zeros).  Output [B*T, u*Cout] is the same memory as
//                    [B*T*u, Cout].  Epilogue writes x and lrelu(x, 0.1).
//   ResBlock1 c1     dilated conv; epilogue lrelu(acc + b, 0.1)
//   ResBlock1 c2     epilogue x' = c2 + x and lrelu(x', 0.1); the branch's last c2 instead folds into the stage sum in the
//                    reference's order - xs = rb0(x), xs += rb1(x), xs += rb2(x), x = xs / n_res - and the last branch writes
//                    lrelu(x, 0.1), or lrelu(x, 0.01) after the last stage (models.py:963 has no slope argument)
//   conv_post + tanh a streaming kernel, one output sample per lane, fixed summation order.
// Utterances go in groups whose largest activation stays below 2 GiB (include/ttsdec.h): the workspace holds one group.
//
// Split-fp16 (ttsvits_generator_*, opt-in): the same launches with PREC_F16S tiles.  Only GEMM operands are split - the weights
// once (ttsvits_generator_pack_planes: a split of the packed blob), every conv input by the epilogue that produces it (the
// activated buffers Y / LX / H / LR then hold hi / lo fp16 planes instead of fp32; z by launch_split).  x, the branch's x', the
// branch sum and the bias / cond / residual / sum / division chain stay fp32, in the exact path's order.  A layer the split tiles
// do not cover (split_ok) keeps the exact tiles inside such a call and reads its input as fp32.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>

#include "kernels.h"

using namespace ttsdec;

namespace {
constexpr float kLrelu = 0.1f;       // modules.LRELU_SLOPE
constexpr float kLreluLast = 0.01f;  // F.leaky_relu's default, models.py:963

struct GenBlob {  // offsets in floats
  size_t pre_w, pre_b;                      // [C0, 7 * Cin] tap-major, [C0]
  size_t up_w[TTSGEN_MAX_UP], up_b[TTSGEN_MAX_UP];  // [u * Cout, 3 * Cin] polyphase, [u * Cout] (bias per phase)
  size_t rw[TTSGEN_MAX_UP][TTSGEN_MAX_RES][6], rb[TTSGEN_MAX_UP][TTSGEN_MAX_RES][6];  // convs1.0-2, convs2.0-2: [C, k * C], [C]
  size_t post_w;                            // [7, C_last]
  size_t cond_w, cond_b;                    // [C0, gin], [C0]
  size_t total;
};

// the second blob (ttsvits_generator_pack_planes): the fp16 planes of the conv weights that run in split-fp16.  Offsets in floats;
// a weight of n elements takes n floats - its hi plane, then its lo plane - in the packed (tap-major / polyphase) layout
struct GenPlanes {
  bool pre, up[TTSGEN_MAX_UP], res[TTSGEN_MAX_UP];  // conv_pre / ups[i] / the resblocks of stage i run in split-fp16
  bool all;  // (never none: ups[0] reads upsample_initial_channel = 2 C_0 channels, a multiple of 8 whenever the dims are built)
  size_t pre_w, up_w[TTSGEN_MAX_UP], rw[TTSGEN_MAX_UP][TTSGEN_MAX_RES][6];
  size_t total;
};
}  // namespace

struct ttsgen_handle : HandleBase {
  ttsgen_dims d;
  GenBlob bl;
  GenPlanes pl;
};

namespace {

int chan(const ttsgen_dims& d, int i) { return d.upsample_initial_channel >> (i + 1); }  // channels after stage i

bool dil_ok(int C, int dil) { return dil == 1 || C % 32 == 0 || 32 % C == 0; }  // LoaderConvDil: a K tile is 32 fp32

bool dims_ok(const ttsgen_dims& d) {
  if (d.resblock != 1 || d.n_dil != 3) return false;  // ResBlock2 / other dilation counts: not built
  if (d.n_up < 1 || d.n_up > TTSGEN_MAX_UP || d.n_res < 1 || d.n_res > TTSGEN_MAX_RES) return false;
  if (d.initial_channel <= 0 || (d.initial_channel & 3) || d.initial_channel > 4096) return false;
  if (d.upsample_initial_channel <= 0 || (d.upsample_initial_channel & 3) || d.upsample_initial_channel > 4096) return false;
  if (d.gin_channels < 0 || d.gin_channels > 4096) return false;
  for (int i = 0; i < d.n_up; ++i) {
    const int C = chan(d, i), u = d.up_rates[i];
    if (C <= 0 || (C & 3) || (C << (i + 1)) != d.upsample_initial_channel) return false;
    if (u < 2 || (u & 1) || u > 64 || d.up_kernels[i] != 2 * u) return false;  // the polyphase packing covers k = 2u, even u
  }
  for (int j = 0; j < d.n_res; ++j) {
    const int k = d.res_kernels[j];
    if (k < 1 || !(k & 1) || k > 31) return false;
    for (int l = 0; l < 3; ++l) {
      const int dl = d.res_dilations[j][l];
      if (dl < 1 || dl > 16) return false;
      for (int i = 0; i < d.n_up; ++i)
        if (!dil_ok(chan(d, i), dl)) return false;
    }
  }
  return true;
}

GenBlob make_layout(const ttsgen_dims& d) {
  GenBlob L;
  memset(&L, 0, sizeof(L));
  Carver cv{nullptr};
  const size_t C0 = d.upsample_initial_channel;
  L.pre_w = cv.take_off(C0 * 7 * d.initial_channel);
  L.pre_b = cv.take_off(C0);
  for (int i = 0; i < d.n_up; ++i) {
    const size_t Ci = i == 0 ? C0 : chan(d, i - 1), Co = chan(d, i), u = d.up_rates[i];
    L.up_w[i] = cv.take_off(u * Co * 3 * Ci);
    L.up_b[i] = cv.take_off(u * Co);
  }
  for (int i = 0; i < d.n_up; ++i) {
    const size_t C = chan(d, i);
    for (int j = 0; j < d.n_res; ++j)
      for (int c = 0; c < 6; ++c) {
        L.rw[i][j][c] = cv.take_off(C * d.res_kernels[j] * C);
        L.rb[i][j][c] = cv.take_off(C);
      }
  }
  L.post_w = cv.take_off(7 * (size_t)chan(d, d.n_up - 1));
  if (d.gin_channels > 0) {
    L.cond_w = cv.take_off(C0 * d.gin_channels);
    L.cond_b = cv.take_off(C0);
  }
  L.total = cv.off;
  return L;
}

// A conv runs in split-fp16 when its rows are whole 16-byte columns of fp16 (Cin % 8) and, dilated, when its taps line up with the
// 64-k tiles of launch_gemm_dil_f16s (Cin | 64 or 64 | Cin; its 32-k tiles then line up too).  The resblocks of a stage
// share their buffers, so they switch together: one dilation that fails keeps the whole stage exact.
bool split_ok(int Cin, int dil) { return Cin % 8 == 0 && (dil == 1 || Cin % 64 == 0 || 64 % Cin == 0); }

GenPlanes make_planes(const ttsgen_dims& d) {
  GenPlanes P;
  memset(&P, 0, sizeof(P));
  Carver cv{nullptr};
  const size_t C0 = d.upsample_initial_channel;
  P.all = true;
  auto note = [&](bool ok) { P.all = P.all && ok; return ok; };
  if ((P.pre = note(split_ok(d.initial_channel, 1)))) P.pre_w = cv.take_off(C0 * 7 * d.initial_channel);
  for (int i = 0; i < d.n_up; ++i) {
    const size_t Ci = i == 0 ? C0 : chan(d, i - 1), Co = chan(d, i), u = d.up_rates[i];
    if ((P.up[i] = note(split_ok((int)Ci, 1)))) P.up_w[i] = cv.take_off(u * Co * 3 * Ci);
  }
  for (int i = 0; i < d.n_up; ++i) {
    const size_t C = chan(d, i);
    bool ok = true;
    for (int j = 0; j < d.n_res; ++j)
      for (int l = 0; l < 3; ++l) ok = ok && split_ok((int)C, d.res_dilations[j][l]);
    if (!(P.res[i] = note(ok))) continue;
    for (int j = 0; j < d.n_res; ++j)
      for (int c = 0; c < 6; ++c) P.rw[i][j][c] = cv.take_off(C * d.res_kernels[j] * C);
  }
  P.total = cv.off;
  return P;
}

int n_tensors(const ttsgen_dims& d) { return 2 + 2 * d.n_up + 12 * d.n_up * d.n_res + 1 + (d.gin_channels > 0 ? 2 : 0); }

// largest activation of one utterance, in floats (include/ttsdec.h)
size_t utt_floats(const ttsgen_dims& d, int T) {
  size_t f = (size_t)T * d.upsample_initial_channel, Ts = T;
  for (int i = 0; i < d.n_up; ++i) {
    Ts *= d.up_rates[i];
    const size_t a = Ts * chan(d, i);
    if (a > f) f = a;
  }
  return f;
}

// utterances per group: no activation buffer reaches 2 GiB, and no launch has more than 65535 row tiles of 64 rows (the grid's
// y extent).  TTSGEN_GROUP_FORCE=n (tests only) caps it lower.
constexpr size_t kMaxRows = (size_t)65535 * 64;
int group_size(const ttsgen_dims& d, int B, int T) {
  const size_t f = utt_floats(d, T);
  size_t rows = T;
  for (int i = 0; i < d.n_up; ++i) rows *= d.up_rates[i];
  size_t cap = (((size_t)1 << 31) - 4096) / (4 * f);
  if (kMaxRows / rows < cap) cap = kMaxRows / rows;
  int G = cap < (size_t)B ? (int)cap : B;
  if (const char* e = getenv("TTSGEN_GROUP_FORCE")) {
    const int n = atoi(e);
    if (n > 0 && n < G) G = n;
  }
  return G;
}

// The workspace of one group of G utterances (carved as layout.h's Carver comment says).  Y: a stage's activated input (conv_pre's
// output, then each stage's result; kept first: ttsgen_forward_stages reads it); X / LX: the upsampled x and lrelu(x); H: c1's
// output; R / LR: the branch's running x' and lrelu(x'); condv: [G, C0] cond(g)
//
// Split-fp16 (pl != nullptr: the handle's GenPlanes): the same six buffers - the two fp16 planes of an
// [M, N] activation take the bytes of its fp32 form, hi plane first - plus zp, the planes of z, and, when some layer stays exact,
// tmp: an exact layer cannot write planes, so where a split layer reads its result the fp32 form goes to tmp and launch_split
// makes the planes.  Planes do not sit at their fp32 element's bytes, so the last conv of a stage cannot turn the branch sum into
// the next stage's input in place as the exact path does (there each element is read and written by one thread): the planes go
// to LX, which no launch reads after the last branch's first conv, and Y and LX swap roles for the next stage.  A stage output
// that is wanted as fp32 (the last stage, for conv_post; a ttsgen_forward_stages read-back; an exact next layer) is written in
// place when Y is the first buffer and into LX, then the first buffer, otherwise: it always ends up at the start of the workspace.
struct GenWs { float *Y, *X, *LX, *H, *R, *LR, *condv, *zp, *tmp; };
GenWs carve_gen(Carver& cv, const ttsgen_dims& d, size_t G, int T, const GenPlanes* pl = nullptr) {
  const size_t F = G * utt_floats(d, T);
  GenWs w;
  w.Y = cv.take(F); w.X = cv.take(F); w.LX = cv.take(F); w.H = cv.take(F); w.R = cv.take(F); w.LR = cv.take(F);
  w.condv = cv.take(G * d.upsample_initial_channel);
  w.zp = pl != nullptr && pl->pre ? cv.take(G * T * d.initial_channel) : nullptr;
  w.tmp = pl != nullptr && !pl->all ? cv.take(F) : nullptr;
  return w;
}

// ===========================================================================
// kernels
// ===========================================================================
// ConvTranspose1d weight w [Cin, Cout, 2u] -> the polyphase 3-tap conv weight out [u * Cout, 3 * Cin]:
// out[r * Cout + co][tap * Cin + ci] = w[ci, co, j], j = u * (1 - tap) + r + u/2, zero where j is outside [0, 2u)
__global__ void pack_up_kernel(const float* w, float* out, int Cin, int Cout, int u) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t K = (size_t)3 * Cin;
  if (i >= (size_t)u * Cout * K) return;
  const int n = (int)(i / K), k = (int)(i % K);
  const int r = n / Cout, co = n % Cout, tap = k / Cin, ci = k % Cin;
  const int j = u * (1 - tap) + r + u / 2;
  out[i] = (j >= 0 && j < 2 * u) ? w[((size_t)ci * Cout + co) * 2 * u + j] : 0.f;
}
// bias [Cout] -> one copy per output phase [u * Cout]
__global__ void rep_bias_kernel(const float* b, float* out, int Cout, int u) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < u * Cout) out[i] = b[i % Cout];
}

// conv_post (Conv1d(C, 1, 7, padding 3, bias=False)) + tanh, models.py:964-965: one output sample per lane; x [M = G*T, C]
// channel-last (the activated last stage), w [7, C] tap-major; sum over taps, then channels, in order
__global__ __launch_bounds__(256) void conv_post_tanh_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ out,
                                                             int M, int T, int C) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int t = m % T;
  float acc = 0.f;
  for (int tap = 0; tap < 7; ++tap) {
    const int tt = t + tap - 3;
    if (tt < 0 || tt >= T) continue;
    const float4* xr = reinterpret_cast<const float4*>(x + (size_t)(m + tap - 3) * C);
    const float4* wr = reinterpret_cast<const float4*>(w + (size_t)tap * C);
    for (int c = 0; c < C / 4; ++c) {
      const float4 a = xr[c], b = wr[c];
      acc = fmaf(b.x, a.x, acc);
      acc = fmaf(b.y, a.y, acc);
      acc = fmaf(b.z, a.z, acc);
      acc = fmaf(b.w, a.w, acc);
    }
  }
  out[m] = tanhf(acc);
}

// one conv of the generator: x [M, Cin] channel-last in utterances of T frames, W [N, taps * Cin]
GemmArgs conv_args(const float* x, int M, int T, int Cin, int taps, int dil, const float* W, const float* bias, int N) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.a = make_seg1(x, Cin, taps * Cin);
  g.a_lo = g.a;
  g.T = T; g.Cin = Cin; g.taps = taps; g.dil = dil;
  g.W = W; g.W_lo = W; g.ldw = taps * Cin; g.prec = PREC_F32;
  g.M = M; g.N = N; g.K = taps * Cin;
  g.bias = bias;
  g.ldo = N;
  g.slope2 = kLrelu;
  return g;
}

// the planes of an n-element tensor held in n floats: hi, then lo
f16* plane_hi(const float* p) { return reinterpret_cast<f16*>(const_cast<float*>(p)); }
f16* plane_lo(const float* p, size_t n) { return plane_hi(p) + n; }

// the forward pass over one group of G utterances; n_stages < n_up stops early (ttsgen_forward_stages).  planes == nullptr: exact
// fp32; else the handle's split layers (GenPlanes) take their weights from it and their inputs as planes
void run_group(const ttsgen_handle* h, const float* planes, const float* z, const float* g, int G, int T, int n_stages, float* out, float* ws,
               hipStream_t st) {
  const ttsgen_dims& d = h->d;
  const GenBlob& L = h->bl;
  const GenPlanes none{};
  const GenPlanes& P = planes != nullptr ? h->pl : none;
  const float* b = h->blob;
  Carver cv{ws};  // (the layout of THIS group: the last one may hold fewer utterances than the reported size is for)
  const GenWs w = carve_gen(cv, d, G, T, planes != nullptr ? &h->pl : nullptr);
  float *Y = w.Y, *X = w.X, *LX = w.LX, *H = w.H, *R = w.R, *LR = w.LR, *condv = w.condv;
  const int C0 = d.upsample_initial_channel;
  // one conv: x as fp32, or (sp: a split layer) as the planes its producer left, with the weight planes at wp
  auto conv = [&](bool sp, const float* x, int M, int Tx, int Cin, int taps, int dil, size_t w_off, size_t wp, size_t b_off, int N) {
    GemmArgs a = conv_args(x, M, Tx, Cin, taps, dil, b + w_off, b + b_off, N);
    if (sp) {
      a.a = make_seg1(plane_hi(x), Cin, taps * Cin);
      a.a_lo = make_seg1(plane_lo(x, (size_t)M * Cin), Cin, taps * Cin);
      a.W = plane_hi(planes + wp);
      a.W_lo = plane_lo(planes + wp, (size_t)N * taps * Cin);
      a.prec = PREC_F16S;
    }
    return a;
  };
  // launches it with its activated output in dst: fp32, or the planes a split consumer reads (as_planes)
  auto launch = [&](GemmArgs& a, float* dst, bool as_planes) {
    const size_t n = (size_t)a.M * a.N;
    if (!as_planes) {
      a.out2 = dst;
    } else if (a.prec == PREC_F16S) {
      a.out_kind = 1;
      a.out_h = plane_hi(dst);
      a.out_l = plane_lo(dst, n);
    } else {
      a.out2 = w.tmp;  // (an exact layer in front of a split one)
    }
    launch_gemm(a, A_CONV_DIL, EPI_LRELU2, st);
    if (as_planes && a.prec != PREC_F16S) launch_split(w.tmp, plane_hi(dst), plane_lo(dst, n), n, st);
  };
  if (g != nullptr) launch_cond(g, b + L.cond_w, b + L.cond_b, condv, G, C0, d.gin_channels, st);
  // models.py:948-950: x = conv_pre(x) (+ cond(g)); the first stage reads lrelu(x, 0.1) (:953)
  {
    const size_t nz = (size_t)G * T * d.initial_channel;
    if (P.pre) launch_split(z, plane_hi(w.zp), plane_lo(w.zp, nz), nz, st);
    GemmArgs a = conv(P.pre, P.pre ? w.zp : z, G * T, T, d.initial_channel, 7, 1, L.pre_w, P.pre_w, L.pre_b, C0);
    a.rowvec = g != nullptr ? condv : nullptr;
    a.slope2 = n_stages == 0 && d.n_up == 0 ? kLreluLast : kLrelu;
    launch(a, Y, n_stages > 0 && P.up[0]);
  }
  int Ts = T, Cin = C0;
  for (int i = 0; i < n_stages; ++i) {
    const int u = d.up_rates[i], C = chan(d, i), Tin = Ts;
    Ts *= u;
    const int M = G * Ts;
    const float slope_out = i == d.n_up - 1 ? kLreluLast : kLrelu;
    const bool rs = P.res[i];
    // :954 x = ups[i](x): [G*Tin, u*C] = [G*Ts, C]; x and lrelu(x, 0.1) (the first layer of every branch, modules.py:298)
    {
      GemmArgs a = conv(P.up[i], Y, G * Tin, Tin, Cin, 3, 1, L.up_w[i], P.up_w[i], L.up_b[i], u * C);
      a.out = X;
      launch(a, LX, rs);
    }
    // :955-962 xs = sum_j resblocks[i * n_res + j](x); x = xs / n_res.  The sum lives in Y (the stage input, dead once ups[i] has
    // read it); the last branch turns it into the stage's activated output: in place, or - planes, and fp32 when Y is not the
    // first buffer - into LX, which then becomes Y (carve_gen)
    float* Ssum = Y;
    for (int j = 0; j < d.n_res; ++j) {
      const int k = d.res_kernels[j];
      for (int l = 0; l < 3; ++l) {
        // modules.py:298-301: xt = c1(lrelu(x)); xt = lrelu(xt)
        GemmArgs c1 = conv(rs, l == 0 ? LX : LR, M, Ts, C, k, d.res_dilations[j][l], L.rw[i][j][l], P.rw[i][j][l], L.rb[i][j][l], C);
        launch(c1, H, rs);
        // :304-305: x = c2(xt) + x
        GemmArgs c2 = conv(rs, H, M, Ts, C, k, 1, L.rw[i][j][3 + l], P.rw[i][j][3 + l], L.rb[i][j][3 + l], C);
        c2.resid = l == 0 ? X : R;
        if (l < 2) {
          c2.out = R;
          launch(c2, LR, rs);
        } else {
          if (j > 0) c2.sum = Ssum;  // xs += rb_j(x)
          if (j == d.n_res - 1) {
            c2.div = (float)d.n_res;  // x = xs / num_kernels; then lrelu for the next stage / conv_post
            c2.slope2 = slope_out;
            const bool as_planes = i + 1 < n_stages && P.up[i + 1];
            float* dst = !as_planes && Y == w.Y ? Ssum : LX;
            launch(c2, dst, as_planes);
            if (dst != Y) {
              LX = Y;
              Y = dst;
            }
          } else {
            c2.out = Ssum;
            c2.out2 = nullptr;
            launch_gemm(c2, A_CONV_DIL, EPI_LRELU2, st);
          }
        }
      }
    }
    Cin = C;
  }
  if (n_stages == d.n_up && out != nullptr)  // :964-965
    hipLaunchKernelGGL(conv_post_tanh_kernel, grid1((size_t)G * Ts), dim3(256), 0, st, Y, b + L.post_w, out, G * Ts, Ts, Cin);
}

}  // namespace

extern "C" {

int ttsgen_create(const ttsgen_dims* dims, ttsgen_handle** out) {
  if (!dims || !out) return TTSDEC_ERR_INVALID_ARG;
  *out = nullptr;
  if (!dims_ok(*dims)) return TTSDEC_ERR_DIMS;
  ttsgen_handle* h = new (std::nothrow) ttsgen_handle();
  if (!h) return TTSDEC_ERR_INVALID_ARG;
  h->d = *dims;
  h->bl = make_layout(*dims);
  h->pl = make_planes(*dims);
  h->device = current_device_or_minus1();
  *out = h;
  return TTSDEC_OK;
}
int ttsgen_destroy(ttsgen_handle* h) {
  delete h;
  return TTSDEC_OK;
}
const char* ttsgen_last_hip_error(const ttsgen_handle* h) { return last_hip_error(h); }
int ttsgen_num_weight_tensors(const ttsgen_handle* h) { return h ? n_tensors(h->d) : TTSDEC_ERR_INVALID_ARG; }
size_t ttsgen_packed_bytes(const ttsgen_handle* h) { return h ? h->bl.total * sizeof(float) : 0; }

int ttsgen_pack_weights(ttsgen_handle* h, const float* const* src, int n_src, void* blob, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = pack_begin(h, src, n_src, ttsgen_num_weight_tensors(h), false, blob, ttsgen_packed_bytes(h), st);
  if (rc != TTSDEC_OK) return rc;
  const ttsgen_dims& d = h->d;
  const GenBlob& L = h->bl;
  float* b = static_cast<float*>(blob);
  const int C0 = d.upsample_initial_channel;
  int k = 0;
  launch_conv_transpose(src[k++], b + L.pre_w, C0, d.initial_channel, 7, st);  // [Co, Ci, 7] -> [Co, 7, Ci]
  launch_copy(src[k++], b + L.pre_b, C0, st);
  for (int i = 0; i < d.n_up; ++i) {
    const int Ci = i == 0 ? C0 : chan(d, i - 1), Co = chan(d, i), u = d.up_rates[i];
    hipLaunchKernelGGL(pack_up_kernel, grid1((size_t)u * Co * 3 * Ci), dim3(256), 0, st, src[k++], b + L.up_w[i], Ci, Co, u);
    hipLaunchKernelGGL(rep_bias_kernel, grid1((size_t)u * Co), dim3(256), 0, st, src[k++], b + L.up_b[i], Co, u);
  }
  for (int i = 0; i < d.n_up; ++i) {
    const int C = chan(d, i);
    for (int j = 0; j < d.n_res; ++j)
      for (int c = 0; c < 6; ++c) {
        launch_conv_transpose(src[k++], b + L.rw[i][j][c], C, C, d.res_kernels[j], st);
        launch_copy(src[k++], b + L.rb[i][j][c], C, st);
      }
  }
  launch_conv_transpose(src[k++], b + L.post_w, 1, chan(d, d.n_up - 1), 7, st);  // [1, C, 7] -> [7, C]
  if (d.gin_channels > 0) {
    launch_copy(src[k++], b + L.cond_w, (size_t)C0 * d.gin_channels, st);
    launch_copy(src[k++], b + L.cond_b, C0, st);
  }
  return pack_end(h, b);
}

int ttsgen_bind_weights(ttsgen_handle* h, const void* blob) { return bind_blob(h, blob); }

// the workspace of a call: exact fp32 (pl = nullptr), or split-fp16 with the handle's planes
static size_t gen_ws_bytes(const ttsgen_handle* h, const GenPlanes* pl, int B, int T) {
  if (!h || B <= 0 || T <= 0) return 0;
  const int G = group_size(h->d, B, T);
  if (G < 1) return 0;
  Carver cv{nullptr};
  carve_gen(cv, h->d, G, T, pl);
  return cv.bytes();
}

// planes != nullptr: split-fp16 (the handle has split layers)
size_t ttsgen_workspace_bytes(const ttsgen_handle* h, int B, int T) { return gen_ws_bytes(h, nullptr, B, T); }

static int gen_call(ttsgen_handle* h, const float* planes, const float* z, const float* g, int B, int T, int n_stages, float* out,
                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !z || !workspace || B <= 0 || T <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (g != nullptr && h->d.gin_channels <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (!h->blob) return TTSDEC_ERR_NOT_BOUND;
  const int G = group_size(h->d, B, T);
  if (G < 1) return TTSDEC_ERR_DIMS;
  if (n_stages < h->d.n_up && G < B) return TTSDEC_ERR_INVALID_ARG;  // (the stage read-back holds one group)
  if (workspace_bytes < gen_ws_bytes(h, planes != nullptr ? &h->pl : nullptr, B, T) || (reinterpret_cast<uintptr_t>(workspace) & 255))
    return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(h->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  size_t up_all = 1;
  for (int i = 0; i < h->d.n_up; ++i) up_all *= h->d.up_rates[i];
  for (int b0 = 0; b0 < B; b0 += G) {
    const int n = B - b0 < G ? B - b0 : G;
    run_group(h, planes, z + (size_t)b0 * T * h->d.initial_channel, g != nullptr ? g + (size_t)b0 * h->d.gin_channels : nullptr, n, T, n_stages,
              out != nullptr ? out + (size_t)b0 * T * up_all : nullptr, static_cast<float*>(workspace), st);
  }
  return record_hip_error(h, "forward");
}

int ttsgen_forward(ttsgen_handle* h, const float* z, const float* g, int B, int T, float* out, void* workspace, size_t workspace_bytes,
                   void* stream) {
  if (!out) return TTSDEC_ERR_INVALID_ARG;
  return gen_call(h, nullptr, z, g, B, T, h ? h->d.n_up : 0, out, workspace, workspace_bytes, stream);
}

int ttsgen_forward_stages(ttsgen_handle* h, const float* z, const float* g, int B, int T, int n_stages, void* workspace, size_t workspace_bytes,
                          void* stream) {
  if (!h || n_stages < 0 || n_stages > h->d.n_up) return TTSDEC_ERR_INVALID_ARG;
  return gen_call(h, nullptr, z, g, B, T, n_stages, nullptr, workspace, workspace_bytes, stream);
}

// ---- the same forward with the arithmetic as a call argument (include/ttsdec.h) ----
size_t ttsvits_generator_planes_bytes(const ttsgen_handle* h) { return h ? h->pl.total * sizeof(float) : 0; }

int ttsvits_generator_pack_planes(ttsgen_handle* h, void* planes, void* stream) {
  if (!h) return TTSDEC_ERR_INVALID_ARG;
  if (!h->blob) return TTSDEC_ERR_NOT_BOUND;
  if (!planes) return TTSDEC_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(planes) & 255) return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(h->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ttsgen_dims& d = h->d;
  const GenBlob& L = h->bl;
  const GenPlanes& P = h->pl;
  const float* b = h->blob;
  float* p = static_cast<float*>(planes);
  auto split = [&](size_t src, size_t dst, size_t n) { launch_split(b + src, plane_hi(p + dst), plane_lo(p + dst, n), n, st); };
  const size_t C0 = d.upsample_initial_channel;
  if (P.pre) split(L.pre_w, P.pre_w, C0 * 7 * d.initial_channel);
  for (int i = 0; i < d.n_up; ++i) {
    const size_t Ci = i == 0 ? C0 : chan(d, i - 1), C = chan(d, i), u = d.up_rates[i];
    if (P.up[i]) split(L.up_w[i], P.up_w[i], u * C * 3 * Ci);
    for (int j = 0; j < d.n_res && P.res[i]; ++j)
      for (int c = 0; c < 6; ++c) split(L.rw[i][j][c], P.rw[i][j][c], C * d.res_kernels[j] * C);
  }
  return record_hip_error(h, "pack_planes");
}

size_t ttsvits_generator_workspace_bytes(const ttsgen_handle* h, int precision, int B, int T) {
  if (!h || (precision != TTSDEC_PREC_F32 && precision != TTSDEC_PREC_SPLIT_F16)) return 0;
  return gen_ws_bytes(h, precision == TTSDEC_PREC_SPLIT_F16 ? &h->pl : nullptr, B, T);
}

int ttsvits_generator_forward(ttsgen_handle* h, int precision, const void* planes, const float* z, const float* g, int B, int T, int n_stages,
                              float* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || (precision != TTSDEC_PREC_F32 && precision != TTSDEC_PREC_SPLIT_F16)) return TTSDEC_ERR_INVALID_ARG;
  if (n_stages < 0 || n_stages > h->d.n_up) return TTSDEC_ERR_INVALID_ARG;
  const bool split = precision == TTSDEC_PREC_SPLIT_F16;
  if (split && !planes) return TTSDEC_ERR_INVALID_ARG;
  if (split && (reinterpret_cast<uintptr_t>(planes) & 255)) return TTSDEC_ERR_WORKSPACE;
  // (out is only looked at by the full forward: with fewer stages, or with out == NULL, the call is the stage read-back)
  return gen_call(h, split ? static_cast<const float*>(planes) : nullptr, z, g, B, T, n_stages, n_stages == h->d.n_up ? out : nullptr, workspace,
                  workspace_bytes, stream);
}

}  // extern "C"
