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
// Every conv has one record (GConv: blob and planes offsets, whether it splits, N / Cin / taps, its source tensors, how it is
// packed), made by one walk at ttsgen_create; the two pack steps and the forward loop over the records and state no shape.
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

// One conv of the generator as the GEMM core reads it: packed weight [N, taps * Cin] and bias [N].  Made once by the walk at
// ttsgen_create; layout, pack, the planes, the tensor count and the forward's GEMM calls all read it.  Offsets in floats.
struct GConv {
  size_t w, b;  // in the blob (conv_post has no bias)
  size_t p;     // in the planes buffer (split): hi plane, then lo plane, n() floats in all, in the packed layout
  bool split;   // runs in split-fp16 in a ttsvits_generator_forward call that asks for it
  int N, Cin, taps;
  int src;      // its first source tensor: the weight, then the bias
  int u;        // ttsgen_pack_weights: 0, a Conv1d [N, Cin, taps] -> [N, taps, Cin]; else a ConvTranspose1d [Cin, N / u, 2u] packed
  bool bias;    // as the polyphase 3-tap conv, its bias once per phase.  bias: false for conv_post
  int K() const { return taps * Cin; }
  size_t n() const { return (size_t)N * K(); }
};
struct GenBlob {
  GConv pre;                                         // [C0, 7 * Cin] tap-major
  GConv up[TTSGEN_MAX_UP];                           // [u * Cout, 3 * Cin] polyphase, bias [u * Cout]
  GConv res[TTSGEN_MAX_UP][TTSGEN_MAX_RES][6];       // convs1.0-2, convs2.0-2: [C, k * C]
  GConv post;                                        // [1, 7 * C_last]
  Vec cond_w, cond_b;                                // [C0, gin], [C0], copied as given (no GEMM tile reads them)
  bool all;  // every conv does (never none: ups[0] reads upsample_initial_channel = 2 C_0 channels, a multiple of 8)
  size_t total, planes_total;  // floats: the blob; the second blob (ttsvits_generator_pack_planes)
  int n_src;                   // source tensors of ttsgen_pack_weights
};
}  // namespace

struct ttsgen_handle : HandleBase {
  ttsgen_dims d;
  GenBlob bl;
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

// A conv runs in split-fp16 when its rows are whole 16-byte columns of fp16 (Cin % 8) and, dilated, when its taps line up with the
// 64-k tiles of launch_gemm_dil_f16s (Cin | 64 or 64 | Cin; its 32-k tiles then line up too).  The resblocks of a stage
// share their buffers, so they switch together: one dilation that fails keeps the whole stage exact.
bool split_ok(int Cin, int dil) { return Cin % 8 == 0 && (dil == 1 || Cin % 64 == 0 || 64 % Cin == 0); }

// The one walk (at ttsgen_create): blob offsets in blob order, source indices in the order include/ttsdec.h documents (src ends as
// their count) and, for the convs that run in split-fp16, planes offsets in that order too: pre, the ups, the resblocks of split stages
struct Walk : BlobWalk {
  Carver pv{nullptr};  // the planes buffer
  GConv conv(int N, int Cin, int taps, bool split, int u = 0, bool bias = true) {
    GConv c{0, 0, 0, split, N, Cin, taps, src, u, bias};
    c.w = cv.take_off(c.n());
    if (bias) c.b = cv.take_off(N);
    if (split) c.p = pv.take_off(c.n());
    src += bias ? 2 : 1;
    return c;
  }
};

GenBlob make_layout(const ttsgen_dims& d) {
  GenBlob L;
  memset(&L, 0, sizeof(L));
  Walk w;
  const int C0 = d.upsample_initial_channel;
  L.pre = w.conv(C0, d.initial_channel, 7, split_ok(d.initial_channel, 1));
  L.all = L.pre.split;
  for (int i = 0; i < d.n_up; ++i) {
    const int Ci = i == 0 ? C0 : chan(d, i - 1), u = d.up_rates[i];
    L.up[i] = w.conv(u * chan(d, i), Ci, 3, split_ok(Ci, 1), u);
    L.all = L.all && L.up[i].split;
  }
  for (int i = 0; i < d.n_up; ++i) {
    const int C = chan(d, i);
    bool ok = true;
    for (int j = 0; j < d.n_res; ++j)
      for (int l = 0; l < 3; ++l) ok = ok && split_ok(C, d.res_dilations[j][l]);
    L.all = L.all && ok;
    for (int j = 0; j < d.n_res; ++j)
      for (int c = 0; c < 6; ++c) L.res[i][j][c] = w.conv(C, C, d.res_kernels[j], ok);
  }
  L.post = w.conv(1, chan(d, d.n_up - 1), 7, false, 0, false);
  if (d.gin_channels > 0) {
    L.cond_w = w.vec((size_t)C0 * d.gin_channels);
    L.cond_b = w.vec(C0);
  }
  L.total = w.cv.off;
  L.planes_total = w.pv.off;
  L.n_src = w.src;
  return L;
}

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
// Split-fp16 (pl != nullptr: the handle's records): the same six buffers - the two fp16 planes of an
// [M, N] activation take the bytes of its fp32 form, hi plane first - plus zp, the planes of z, and, when some layer stays exact,
// tmp: an exact layer cannot write planes, so where a split layer reads its result the fp32 form goes to tmp and launch_split
// makes the planes.  Planes do not sit at their fp32 element's bytes, so the last conv of a stage cannot turn the branch sum into
// the next stage's input in place as the exact path does (there each element is read and written by one thread): the planes go
// to LX, which no launch reads after the last branch's first conv, and Y and LX swap roles for the next stage.  A stage output
// that is wanted as fp32 (the last stage, for conv_post; a ttsgen_forward_stages read-back; an exact next layer) is written in
// place when Y is the first buffer and into LX, then the first buffer, otherwise: it always ends up at the start of the workspace.
struct GenWs { float *Y, *X, *LX, *H, *R, *LR, *condv, *zp, *tmp; };
GenWs carve_gen(Carver& cv, const ttsgen_dims& d, size_t G, int T, const GenBlob* pl = nullptr) {
  const size_t F = G * utt_floats(d, T);
  GenWs w;
  w.Y = cv.take(F); w.X = cv.take(F); w.LX = cv.take(F); w.H = cv.take(F); w.R = cv.take(F); w.LR = cv.take(F);
  w.condv = cv.take(G * d.upsample_initial_channel);
  w.zp = pl != nullptr && pl->pre.split ? cv.take(G * T * d.initial_channel) : nullptr;
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

// ttsgen_pack_weights' step for one conv: its weight and bias from src into the blob b
void pack_conv(const float* const* src, float* b, const GConv& c, hipStream_t st) {
  if (c.u > 0) {
    const int Cout = c.N / c.u;
    hipLaunchKernelGGL(pack_up_kernel, grid1(c.n()), dim3(256), 0, st, src[c.src], b + c.w, c.Cin, Cout, c.u);
    hipLaunchKernelGGL(rep_bias_kernel, grid1((size_t)c.N), dim3(256), 0, st, src[c.src + 1], b + c.b, Cout, c.u);
    return;
  }
  launch_conv_transpose(src[c.src], b + c.w, c.N, c.Cin, c.taps, st);  // [Co, Ci, k] -> [Co, k, Ci]
  if (c.bias) launch_copy(src[c.src + 1], b + c.b, c.N, st);
}
// ttsvits_generator_pack_planes' step: the planes of a split conv's packed weight, from the blob b into the planes buffer p
void split_conv(const float* b, float* p, const GConv& c, hipStream_t st) {
  if (c.split) planes_split(b + c.w, p + c.p, c.n(), st);
}

// the forward pass over one group of G utterances; n_stages < n_up stops early (ttsgen_forward_stages).  planes == nullptr: exact
// fp32; else the handle's split layers (GConv::split) take their weights from it and their inputs as planes
void run_group(const ttsgen_handle* h, const float* planes, const float* z, const float* g, int G, int T, int n_stages, float* out, float* ws,
               hipStream_t st) {
  const ttsgen_dims& d = h->d;
  const GenBlob& L = h->bl;
  const float* b = h->blob;
  Carver cv{ws};  // (the layout of THIS group: the last one may hold fewer utterances than the reported size is for)
  const GenWs w = carve_gen(cv, d, G, T, planes != nullptr ? &L : nullptr);
  float *Y = w.Y, *X = w.X, *LX = w.LX, *H = w.H, *R = w.R, *LR = w.LR, *condv = w.condv;
  const int C0 = d.upsample_initial_channel;
  auto split = [&](const GConv& c) { return planes != nullptr && c.split; };  // this call runs c in split-fp16
  // one conv of the generator (its record c): x [M, Cin] channel-last in utterances of Tx frames, W [N, taps * Cin] - x as fp32, or
  // (a split layer) as the planes its producer left, with the weight planes at c.p.  (The planes of an n-element tensor are held
  // in n floats: hi, then lo.)
  auto conv = [&](const GConv& c, const float* x, int M, int Tx, int dil) {
    const bool s = split(c);
    GemmArgs a = conv_gemm_args(s ? planes_at(x, (size_t)M * c.Cin) : planes_f32(x), s ? planes_at(planes + c.p, c.n()) : planes_f32(b + c.w),
                                s ? PREC_F16S : PREC_F32, M, Tx, c.Cin, c.taps, c.N, dil);
    a.bias = b + c.b;
    a.slope2 = kLrelu;
    return a;
  };
  // launches it with its activated output in dst: fp32, or the planes a split consumer reads (as_planes)
  auto launch = [&](GemmArgs& a, float* dst, bool as_planes) {
    const size_t n = (size_t)a.M * a.N;
    if (!as_planes) a.out2 = dst;
    else if (a.prec == PREC_F16S) set_output(a, PREC_F16S, dst, n);
    else a.out2 = w.tmp;  // (an exact layer in front of a split one)
    launch_gemm<A_CONV_DIL, EPI_LRELU2>(a, st);
    if (as_planes && a.prec != PREC_F16S) planes_split(w.tmp, dst, n, st);
  };
  if (g != nullptr) launch_cond(g, b + L.cond_w.off, b + L.cond_b.off, condv, G, C0, d.gin_channels, st);
  // models.py:948-950: x = conv_pre(x) (+ cond(g)); the first stage reads lrelu(x, 0.1) (:953)
  {
    const size_t nz = (size_t)G * T * d.initial_channel;
    if (split(L.pre)) planes_split(z, w.zp, nz, st);
    GemmArgs a = conv(L.pre, split(L.pre) ? w.zp : z, G * T, T, 1);
    a.rowvec = g != nullptr ? condv : nullptr;
    a.slope2 = n_stages == 0 && d.n_up == 0 ? kLreluLast : kLrelu;
    launch(a, Y, n_stages > 0 && split(L.up[0]));
  }
  int Ts = T;
  for (int i = 0; i < n_stages; ++i) {
    const int Tin = Ts;
    Ts *= d.up_rates[i];
    const int M = G * Ts;
    const float slope_out = i == d.n_up - 1 ? kLreluLast : kLrelu;
    const bool rs = split(L.res[i][0][0]);  // (the resblocks of a stage switch together)
    // :954 x = ups[i](x): [G*Tin, u*C] = [G*Ts, C]; x and lrelu(x, 0.1) (the first layer of every branch, modules.py:298)
    {
      GemmArgs a = conv(L.up[i], Y, G * Tin, Tin, 1);
      a.out = X;
      launch(a, LX, rs);
    }
    // :955-962 xs = sum_j resblocks[i * n_res + j](x); x = xs / n_res.  The sum lives in Y (the stage input, dead once ups[i] has
    // read it); the last branch turns it into the stage's activated output: in place, or - planes, and fp32 when Y is not the
    // first buffer - into LX, which then becomes Y (carve_gen)
    float* Ssum = Y;
    for (int j = 0; j < d.n_res; ++j) {
      for (int l = 0; l < 3; ++l) {
        // modules.py:298-301: xt = c1(lrelu(x)); xt = lrelu(xt)
        GemmArgs c1 = conv(L.res[i][j][l], l == 0 ? LX : LR, M, Ts, d.res_dilations[j][l]);
        launch(c1, H, rs);
        // :304-305: x = c2(xt) + x
        GemmArgs c2 = conv(L.res[i][j][3 + l], H, M, Ts, 1);
        c2.resid = l == 0 ? X : R;
        if (l < 2) {
          c2.out = R;
          launch(c2, LR, rs);
        } else {
          if (j > 0) c2.sum = Ssum;  // xs += rb_j(x)
          if (j == d.n_res - 1) {
            c2.div = (float)d.n_res;  // x = xs / num_kernels; then lrelu for the next stage / conv_post
            c2.slope2 = slope_out;
            const bool as_planes = i + 1 < n_stages && split(L.up[i + 1]);
            float* dst = !as_planes && Y == w.Y ? Ssum : LX;
            launch(c2, dst, as_planes);
            if (dst != Y) {
              LX = Y;
              Y = dst;
            }
          } else {
            c2.out = Ssum;
            c2.out2 = nullptr;
            launch_gemm<A_CONV_DIL, EPI_LRELU2>(c2, st);
          }
        }
      }
    }
  }
  if (n_stages == d.n_up && out != nullptr)  // :964-965
    hipLaunchKernelGGL(conv_post_tanh_kernel, grid1((size_t)G * Ts), dim3(256), 0, st, Y, b + L.post.w, out, G * Ts, Ts, L.post.Cin);
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
  h->device = current_device_or_minus1();
  *out = h;
  return TTSDEC_OK;
}
int ttsgen_destroy(ttsgen_handle* h) {
  delete h;
  return TTSDEC_OK;
}
const char* ttsgen_last_hip_error(const ttsgen_handle* h) { return last_hip_error(h); }
int ttsgen_num_weight_tensors(const ttsgen_handle* h) { return h ? h->bl.n_src : TTSDEC_ERR_INVALID_ARG; }
size_t ttsgen_packed_bytes(const ttsgen_handle* h) { return h ? h->bl.total * sizeof(float) : 0; }

int ttsgen_pack_weights(ttsgen_handle* h, const float* const* src, int n_src, void* blob, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = pack_begin(h, src, n_src, ttsgen_num_weight_tensors(h), false, blob, ttsgen_packed_bytes(h), st);
  if (rc != TTSDEC_OK) return rc;
  const ttsgen_dims& d = h->d;
  const GenBlob& L = h->bl;
  float* b = static_cast<float*>(blob);
  pack_conv(src, b, L.pre, st);
  for (int i = 0; i < d.n_up; ++i) pack_conv(src, b, L.up[i], st);
  for (int i = 0; i < d.n_up; ++i)
    for (int j = 0; j < d.n_res; ++j)
      for (int c = 0; c < 6; ++c) pack_conv(src, b, L.res[i][j][c], st);
  pack_conv(src, b, L.post, st);
  if (d.gin_channels > 0)
    for (const Vec& v : {L.cond_w, L.cond_b}) launch_copy(src[v.src], b + v.off, v.n, st);
  return pack_end(h, b);
}

int ttsgen_bind_weights(ttsgen_handle* h, const void* blob) { return bind_blob(h, blob); }

// the workspace of a call: exact fp32, or split-fp16 with the handle's split layers
static size_t gen_ws_bytes(const ttsgen_handle* h, bool split, int B, int T) {
  if (!h || B <= 0 || T <= 0) return 0;
  const int G = group_size(h->d, B, T);
  if (G < 1) return 0;
  Carver cv{nullptr};
  carve_gen(cv, h->d, G, T, split ? &h->bl : nullptr);
  return cv.bytes();
}

// planes != nullptr: split-fp16 (the handle has split layers)
size_t ttsgen_workspace_bytes(const ttsgen_handle* h, int B, int T) { return gen_ws_bytes(h, false, B, T); }

static int gen_call(ttsgen_handle* h, const float* planes, const float* z, const float* g, int B, int T, int n_stages, float* out,
                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !z || !workspace || B <= 0 || T <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (g != nullptr && h->d.gin_channels <= 0) return TTSDEC_ERR_INVALID_ARG;
  if (!h->blob) return TTSDEC_ERR_NOT_BOUND;
  const int G = group_size(h->d, B, T);
  if (G < 1) return TTSDEC_ERR_DIMS;
  if (n_stages < h->d.n_up && G < B) return TTSDEC_ERR_INVALID_ARG;  // (the stage read-back holds one group)
  if (workspace_bytes < gen_ws_bytes(h, planes != nullptr, B, T) || (reinterpret_cast<uintptr_t>(workspace) & 255))
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
size_t ttsvits_generator_planes_bytes(const ttsgen_handle* h) { return h ? h->bl.planes_total * sizeof(float) : 0; }

int ttsvits_generator_pack_planes(ttsgen_handle* h, void* planes, void* stream) {
  if (!h) return TTSDEC_ERR_INVALID_ARG;
  if (!h->blob) return TTSDEC_ERR_NOT_BOUND;
  if (!planes) return TTSDEC_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(planes) & 255) return TTSDEC_ERR_WORKSPACE;
  if (!device_is_current(h->device)) return TTSDEC_ERR_DEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ttsgen_dims& d = h->d;
  const GenBlob& L = h->bl;
  const float* b = h->blob;
  float* p = static_cast<float*>(planes);
  split_conv(b, p, L.pre, st);
  for (int i = 0; i < d.n_up; ++i) {
    split_conv(b, p, L.up[i], st);
    for (int j = 0; j < d.n_res; ++j)
      for (int c = 0; c < 6; ++c) split_conv(b, p, L.res[i][j][c], st);
  }
  return record_hip_error(h, "pack_planes");
}

size_t ttsvits_generator_workspace_bytes(const ttsgen_handle* h, int precision, int B, int T) {
  if (!h || (precision != TTSDEC_PREC_F32 && precision != TTSDEC_PREC_SPLIT_F16)) return 0;
  return gen_ws_bytes(h, precision == TTSDEC_PREC_SPLIT_F16, B, T);
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
