// The Transformer sequence encoder's layer stack and pool (src/encoders.py:99-111, 177-206):
//   post-norm nn.TransformerEncoderLayer (4 heads, ReLU, batch_first) x layers with the key padding
//   mask t >= lengths[b], then the mean over the valid steps -- forward and backward, fp32.
// Activations are (n = B*T, H) row-major.  The GEMMs (launch_gemm), the flash attention
// (launch_attn_fwd / _bwd on the (n, 3H) QKV buffer, ld = 3H) and the split-K weight gradients
// (plan_wgrad / launch_reduce) are the library's; this file adds the streaming kernels between them
// and the host code that chains a layer stack:
//
//  A  tr_mask_kernel          mask[b, t] = t < len_b (the attention's per-key mask) and the clamped lengths
//  B  add_layernorm_fwd       z = x + r, y = gamma (z - mean) rstd + beta; one row per wave, a float4 per
//                             lane (H <= 256): the mean, then the biased variance of the CENTRED values;
//                             z and (mean, rstd) are saved
//  C  masked_mean_pool_fwd / _bwd   pooled[b] = sum_{t < len_b} y[b, t] / max(len_b, 1); the backward
//                             broadcasts dpooled / len to the valid rows and writes zeros to the others
//  D  add_layernorm_bwd       dz = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma, xhat from the saved
//                             z, mean, rstd (never from y: gamma may be 0); dr = dz through the branch's
//                             dropout, the keep decision redrawn at the GEMM epilogue's site and index;
//                             per 32-row workgroup a partial of dgamma = sum dy xhat and dbeta = sum dy
//  E  ln_col_reduce           the partials summed in chunk order in two levels (groups of ~sqrt(chunks),
//                             then the groups), a kernel boundary between them
//
// Every cross-workgroup dependency is a kernel boundary: no atomics, no waits.  Two calls on the same
// inputs give the same bits.  fp32 MFMA at every matmul-precision setting (no MathScope: mode 0).
#include <cmath>

#include "capi_util.h"
#include "mmf_device.h"

namespace mmf {

namespace {

constexpr int NT = 256;
constexpr int TR_HEADS = 4;
constexpr int LN_ROWS = 32;   // rows per add_layernorm_bwd workgroup (8 per wave): one dgamma / dbeta partial
constexpr uint32_t SITE_TR = 0x500;   // + 4 * layer + {0 attention probabilities, 1 out_proj, 2 ffn, 3 linear2}
constexpr int TR_MAX_HIDDEN = 256, TR_MAX_FFN = 8192;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float hsum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }

// ------------------------------------------------------------------------------------------ A
__global__ __launch_bounds__(NT) void tr_mask_kernel(const int64_t* lengths, int B, int T, float* mask,
                                                     int32_t* lenc) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= (int64_t)B * T) return;
  const int b = (int)(i / T), t = (int)(i % T);
  int64_t L = lengths ? lengths[b] : (int64_t)T;
  L = L < 0 ? 0 : (L > T ? T : L);
  mask[i] = t < L ? 1.f : 0.f;
  if (t == 0) lenc[b] = (int32_t)L;
}

// ------------------------------------------------------------------------------------------ B
struct LnFwdArgs {
  const float* x;      // (n, H)
  const float* r;      // (n, H) the branch
  const float* gamma;  // (H)
  const float* beta;   // (H)
  float* z;            // (n, H) x + r (saved)
  float* stat;         // (n, 2) mean, rstd (saved)
  float* y;            // (n, H)
  int n, H;
  float eps;
};

__global__ __launch_bounds__(NT) void add_layernorm_fwd(LnFwdArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= a.n) return;   // (the whole wave: the cross-lane sums below see 64 active lanes)
  const int c = lane * 4;
  const bool on = c < a.H;
  const int64_t off = (int64_t)row * a.H + c;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (on) {
    const float4 x = ld4(a.x + off), r = ld4(a.r + off);
    v = make_float4(x.x + r.x, x.y + r.y, x.z + r.z, x.w + r.w);
  }
  const float inv_h = 1.f / (float)a.H;
  const float mean = sum64(hsum4(v)) * inv_h;
  const float4 d = on ? make_float4(v.x - mean, v.y - mean, v.z - mean, v.w - mean) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float var = sum64((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) * inv_h;
  const float rstd = 1.f / sqrtf(var + a.eps);
  if (on) {
    const float4 g = ld4(a.gamma + c), be = ld4(a.beta + c);
    st4(a.z + off, v);
    st4(a.y + off, make_float4(fmaf(d.x * rstd, g.x, be.x), fmaf(d.y * rstd, g.y, be.y), fmaf(d.z * rstd, g.z, be.z),
                               fmaf(d.w * rstd, g.w, be.w)));
  }
  if (lane == 0) {
    a.stat[2 * (int64_t)row] = mean;
    a.stat[2 * (int64_t)row + 1] = rstd;
  }
}

// ------------------------------------------------------------------------------------------ C
// One workgroup per sample: 64 float4 column lanes x 4 row lanes, each row lane taking every 4th
// valid step; the 4 partial sums are combined in a fixed order.
__global__ __launch_bounds__(NT) void masked_mean_pool_fwd(const float* y, const int32_t* lenc, int T, int H,
                                                           float* pooled) {
  __shared__ float4 red[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6, c = cx * 4;
  const int b = blockIdx.x;
  const int L = lenc[b];
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < H) {
    const float* yb = y + (int64_t)b * T * H + c;
#pragma unroll 4
    for (int t = ry; t < L; t += 4) {
      const float4 v = ld4(yb + (int64_t)t * H);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  red[ry][cx] = s;
  __syncthreads();
  if (ry == 0 && c < H) {
    const float4 p = red[0][cx], q = red[1][cx], u = red[2][cx], w = red[3][cx];
    const float dv = (float)(L > 1 ? L : 1);
    st4(pooled + (int64_t)b * H + c, make_float4(((p.x + q.x) + (u.x + w.x)) / dv, ((p.y + q.y) + (u.y + w.y)) / dv,
                                                 ((p.z + q.z) + (u.z + w.z)) / dv, ((p.w + q.w) + (u.w + w.w)) / dv));
  }
}

__global__ __launch_bounds__(NT) void masked_mean_pool_bwd(const float* dpooled, const int32_t* lenc, int B, int T,
                                                           int H, float* dy) {
  const int h4 = H / 4;
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= (int64_t)B * T * h4) return;
  const int64_t row = i / h4;
  const int c = (int)(i % h4) * 4;
  const int b = (int)(row / T), t = (int)(row % T);
  const int L = lenc[b];
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < L) {
    const float4 d = ld4(dpooled + (int64_t)b * H + c);
    const float dv = (float)L;
    g = make_float4(d.x / dv, d.y / dv, d.z / dv, d.w / dv);
  }
  st4(dy + row * H + c, g);
}

// ------------------------------------------------------------------------------------------ D
struct LnBwdArgs {
  const float* z;      // (n, H) saved
  const float* stat;   // (n, 2) saved
  const float* gamma;  // (H)
  const float* dy;     // (n, H)
  float* dz;           // (n, H) the gradient of z: the residual path's
  float* dr;           // (n, H) or null (no dropout: dr == dz): dz through the branch's dropout
  float* part;         // (chunks, 2, H): sum dy xhat | sum dy over the workgroup's rows
  int n, H;
  float p;
  uint32_t site;
  const RngSnap* rng;
};

__global__ __launch_bounds__(NT) void add_layernorm_bwd(LnBwdArgs a) {
  __shared__ float4 red[2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane * 4;
  const bool on = c < a.H;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 g = on ? ld4(a.gamma + c) : zero;
  const bool drop = a.dr != nullptr && a.p > 0.f;
  RngSnap rs{0, 0};
  if (drop) rs = *a.rng;
  const float inv_keep = drop ? 1.f / (1.f - a.p) : 1.f;
  const float inv_h = 1.f / (float)a.H;
  float4 sg = zero, sb = zero;
  const int r0 = blockIdx.x * LN_ROWS;
  for (int i = 0; i < LN_ROWS / 4; ++i) {
    const int row = r0 + i * 4 + wave;
    if (row >= a.n) break;   // (the whole wave)
    const int64_t off = (int64_t)row * a.H + c;
    const float mean = a.stat[2 * (int64_t)row], rstd = a.stat[2 * (int64_t)row + 1];
    float4 xh = zero, dy = zero;
    if (on) {
      const float4 z = ld4(a.z + off);
      dy = ld4(a.dy + off);
      xh = make_float4((z.x - mean) * rstd, (z.y - mean) * rstd, (z.z - mean) * rstd, (z.w - mean) * rstd);
    }
    const float4 gx = make_float4(dy.x * g.x, dy.y * g.y, dy.z * g.z, dy.w * g.w);
    const float m1 = sum64(hsum4(gx)) * inv_h;
    const float m2 = sum64((gx.x * xh.x + gx.y * xh.y) + (gx.z * xh.z + gx.w * xh.w)) * inv_h;
    if (on) {
      const float4 dz = make_float4(rstd * ((gx.x - m1) - xh.x * m2), rstd * ((gx.y - m1) - xh.y * m2),
                                    rstd * ((gx.z - m1) - xh.z * m2), rstd * ((gx.w - m1) - xh.w * m2));
      st4(a.dz + off, dz);
      if (drop) {
        // the GEMM epilogue's draw for this element: idx = row * N + column (N = H)
        const uint32_t bits = keep4(rs, a.site, (uint64_t)row * (uint64_t)a.H + (uint64_t)c, a.p);
        st4(a.dr + off, make_float4((bits & 1u) ? dz.x * inv_keep : 0.f, (bits & 2u) ? dz.y * inv_keep : 0.f,
                                    (bits & 4u) ? dz.z * inv_keep : 0.f, (bits & 8u) ? dz.w * inv_keep : 0.f));
      }
      sg.x = fmaf(dy.x, xh.x, sg.x); sg.y = fmaf(dy.y, xh.y, sg.y);
      sg.z = fmaf(dy.z, xh.z, sg.z); sg.w = fmaf(dy.w, xh.w, sg.w);
      sb.x += dy.x; sb.y += dy.y; sb.z += dy.z; sb.w += dy.w;
    }
  }
  red[0][wave][lane] = sg;
  red[1][wave][lane] = sb;
  __syncthreads();
  if (wave < 2 && on) {   // wave 0: dgamma's partial, wave 1: dbeta's
    const float4 p = red[wave][0][lane], q = red[wave][1][lane], u = red[wave][2][lane], w = red[wave][3][lane];
    st4(a.part + ((int64_t)blockIdx.x * 2 + wave) * a.H + c,
        make_float4((p.x + q.x) + (u.x + w.x), (p.y + q.y) + (u.y + w.y), (p.z + q.z) + (u.z + w.z),
                    (p.w + q.w) + (u.w + w.w)));
  }
}

// ------------------------------------------------------------------------------------------ E
// Group g sums the chunks [g * group, min(nchunk, (g + 1) * group)) of part (nchunk, 2, H) in chunk
// order: columns < H into out0[g * 2H + c], the others into out1[g * 2H + c - H].
__global__ __launch_bounds__(NT) void ln_col_reduce(const float* part, int nchunk, int group, int H, float* out0,
                                                    float* out1) {
  const int W = 2 * H;
  const int c = blockIdx.y * NT + threadIdx.x;
  if (c >= W) return;
  const int k0 = blockIdx.x * group, k1 = min(nchunk, k0 + group);
  float s = 0.f;
  for (int k = k0; k < k1; ++k) s += part[(int64_t)k * W + c];
  if (c < H) out0[(int64_t)blockIdx.x * W + c] = s;
  else out1[(int64_t)blockIdx.x * W + c - H] = s;
}

// ------------------------------------------------------------------------------------------ host
int tr_check(int B, int T, int H, int F, int NL) {
  if (H % 4 != 0 || H < 4 || H > TR_MAX_HIDDEN)
    return fail(MMF_ELIMIT, "transformer_encoder: hidden %d is not a multiple of 4 in 4..%d", H, TR_MAX_HIDDEN);
  if (F < 1 || F > TR_MAX_FFN) return fail(MMF_ELIMIT, "transformer_encoder: ffn %d outside 1..%d", F, TR_MAX_FFN);
  if (NL < 1 || NL > MMF_TRANSFORMER_MAX_LAYERS)
    return fail(MMF_ELIMIT, "transformer_encoder: layers %d outside 1..%d", NL, MMF_TRANSFORMER_MAX_LAYERS);
  if (B < 1 || T < 1) return fail(MMF_ELIMIT, "transformer_encoder: empty input (batch %d, steps %d)", B, T);
  if ((int64_t)B * T > (int64_t)1 << 24)
    return fail(MMF_ELIMIT, "transformer_encoder: batch * steps %lld > 2^24", (long long)B * T);
  return MMF_OK;
}

int tr_check(const mmf_transformer_desc* d) {
  if (!d) return fail(MMF_EINVAL, "transformer_encoder: null descriptor");
  if (int rc = tr_check(d->batch, d->steps, d->hidden, d->ffn, d->layers)) return rc;
  if (!(d->dropout >= 0.f && d->dropout < 1.f)) return fail(MMF_EINVAL, "transformer_encoder: dropout must be in [0, 1)");
  if (!(d->eps >= 0.f)) return fail(MMF_EINVAL, "transformer_encoder: negative eps");
  return MMF_OK;
}

inline int ln_chunks(int n) { return (n + LN_ROWS - 1) / LN_ROWS; }
inline int ln_group(int nchunk) {   // ~sqrt(nchunk) chunks per first-level group
  int g = 1;
  while (g * g < nchunk) ++g;
  return g;
}

// what the forward keeps for the backward, per layer
struct TrLayerSaved {
  float *qkv, *o, *lse;   // (n, 3H), (n, H), (B, heads, T)
  float *z1, *st1, *y1;   // x + Drop(attention), its (mean, rstd), LayerNorm1's output
  float *h;               // (n, F) Drop(ReLU(linear1))
  float *z2, *st2, *y2;   // y1 + Drop(ffn), its (mean, rstd), the layer's output
};
struct TrSaved {
  RngSnap* rng;
  TrLayerSaved l[MMF_TRANSFORMER_MAX_LAYERS];
  size_t bytes;
};

TrSaved tr_saved(void* base, int B, int T, int H, int F, int NL) {
  Bump bp(base);
  TrSaved s{};
  const size_t n = (size_t)B * T;
  s.rng = bp.take<RngSnap>(1);
  for (int k = 0; k < NL; ++k) {
    TrLayerSaved& l = s.l[k];
    l.qkv = bp.take<float>(n * 3 * H);
    l.o = bp.take<float>(n * H);
    l.lse = bp.take<float>(n * TR_HEADS);
    l.z1 = bp.take<float>(n * H);
    l.st1 = bp.take<float>(n * 2);
    l.y1 = bp.take<float>(n * H);
    l.h = bp.take<float>(n * F);
    l.z2 = bp.take<float>(n * H);
    l.st2 = bp.take<float>(n * 2);
    l.y2 = bp.take<float>(n * H);
  }
  s.bytes = bp.off + 256;
  return s;
}

// the split count of a weight gradient (M x N over `rows`): about 1024 workgroups over its 128 x 128
// output tiles and the splits, at most 64 splits (split_rows keeps >= 32 rows per split)
inline int wgrad_hint(int M, int N) {
  const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
  const int want = 1024 / tiles;
  return want < 1 ? 1 : (want > 64 ? 64 : want);
}

// one layer's four weight (and bias) gradients; with wp.size_only only the slabs are taken
struct TrWgradIn {
  const float *r2, *h, *dh, *y1, *r1, *o, *dqkv, *xin;
  const mmf_transformer_layer_grad* g;
};
void tr_plan_wgrads(WgradPlan& wp, Bump& ws, int n, int H, int F, const TrWgradIn& in) {
  const mmf_transformer_layer_grad none{};
  const mmf_transformer_layer_grad& g = in.g ? *in.g : none;
  wp.split_hint = wgrad_hint(H, F);
  plan_wgrad(wp, ws, H, F, n, opnd(in.r2, H), opnd(in.h, F), g.linear2_w, g.linear2_b);
  wp.split_hint = wgrad_hint(F, H);
  plan_wgrad(wp, ws, F, H, n, opnd(in.dh, F), opnd(in.y1, H), g.linear1_w, g.linear1_b);
  wp.split_hint = wgrad_hint(H, H);
  plan_wgrad(wp, ws, H, H, n, opnd(in.r1, H), opnd(in.o, H), g.out_proj_w, g.out_proj_b);
  wp.split_hint = wgrad_hint(3 * H, H);
  plan_wgrad(wp, ws, 3 * H, H, n, opnd(in.dqkv, 3 * H), opnd(in.xin, H), g.in_proj_w, g.in_proj_b);
}

struct TrWs {
  float* mask;     // (B, T)
  int32_t* lenc;   // (B)
  float* r;        // forward: (n, H) the branch before the residual add
  // backward
  float *dya, *dyb;             // (n, H) the gradient of a layer's output / input (ping-pong)
  float *dz2, *dr2, *dy1, *dz1, *dr1, *dO;   // (n, H)
  float *dh, *dqkv, *dsum;      // (n, F), (n, 3H), (B, heads, T)
  float *lnpart, *lnpart2;      // (chunks, 2, H), (groups, 2, H)
  size_t slab_off;              // the weight-gradient slabs (one layer's, reused by every layer)
  size_t bytes;
};

TrWs tr_carve(void* base, int B, int T, int H, int F, bool backward) {
  Bump bp(base);
  TrWs w{};
  const size_t n = (size_t)B * T;
  w.mask = bp.take<float>(n);
  w.lenc = bp.take<int32_t>((size_t)B);
  if (!backward) {
    w.r = bp.take<float>(n * H);
  } else {
    float** nh[] = {&w.dya, &w.dyb, &w.dz2, &w.dr2, &w.dy1, &w.dz1, &w.dr1, &w.dO};
    for (float** p : nh) *p = bp.take<float>(n * H);
    w.dh = bp.take<float>(n * F);
    w.dqkv = bp.take<float>(n * 3 * H);
    w.dsum = bp.take<float>(n * TR_HEADS);
    const int nchunk = ln_chunks((int)n), group = ln_group(nchunk);
    w.lnpart = bp.take<float>((size_t)nchunk * 2 * H);
    w.lnpart2 = bp.take<float>((size_t)((nchunk + group - 1) / group) * 2 * H);
    bp.off = (bp.off + 255) & ~size_t(255);
    w.slab_off = bp.off;
    WgradPlan wp;
    wp.size_only = true;
    tr_plan_wgrads(wp, bp, (int)n, H, F, TrWgradIn{});
  }
  w.bytes = bp.off + 256;
  return w;
}

AttnPair tr_pair(const TrLayerSaved& s, const float* mask, int T, int H, int layer) {
  AttnPair a;
  memset(&a, 0, sizeof(a));
  a.q = s.qkv; a.k = s.qkv + H; a.v = s.qkv + 2 * H;
  a.o = s.o; a.lse = s.lse;
  a.kmask = mask; a.kmask_mode = mask ? 2 : 0; a.kmask_ld = T;
  a.Lq = a.Lk = T;
  a.ldq = a.ldk = a.ldv = 3 * H;
  a.ldo = H;
  a.drop_site = SITE_TR + 4 * layer;
  return a;
}

hipError_t launch_ln_fwd(const float* x, const float* r, const float* gamma, const float* beta, float* z, float* stat,
                         float* y, int n, int H, float eps, hipStream_t st) {
  LnFwdArgs a{x, r, gamma, beta, z, stat, y, n, H, eps};
  ProfLaunch prof_(st, "add_layernorm_fwd", 10.0 * n * H, 16.0 * n * H);
  mmf_launch(add_layernorm_fwd, dim3((n + 3) / 4), dim3(NT), 0, st, a);
  return hipGetLastError();
}

// dz, dr and the LayerNorm's weight / bias gradients (two-level fixed-order reduce of the partials)
hipError_t launch_ln_bwd(LnBwdArgs a, float* part2, float* dgamma, float* dbeta, hipStream_t st) {
  const int nchunk = ln_chunks(a.n), group = ln_group(nchunk), ngroup = (nchunk + group - 1) / group;
  const int W = 2 * a.H;
  hipError_t e;
  {
    ProfLaunch prof_(st, "add_layernorm_bwd", 16.0 * a.n * a.H, (a.dr ? 16.0 : 12.0) * a.n * a.H);
    mmf_launch(add_layernorm_bwd, dim3(nchunk), dim3(NT), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  {
    ProfLaunch prof_(st, "ln_col_reduce", 1.0 * nchunk * W, 4.0 * nchunk * W);
    mmf_launch(ln_col_reduce, dim3(ngroup, (W + NT - 1) / NT), dim3(NT), 0, st, (const float*)a.part, nchunk, group,
               a.H, part2, part2 + a.H);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  ProfLaunch prof_(st, "ln_col_reduce", 1.0 * ngroup * W, 4.0 * ngroup * W);
  mmf_launch(ln_col_reduce, dim3(1, (W + NT - 1) / NT), dim3(NT), 0, st, (const float*)part2, ngroup, ngroup, a.H, dgamma,
             dbeta);
  return hipGetLastError();
}

hipError_t launch_tr_mask(const int64_t* lengths, int B, int T, const TrWs& w, hipStream_t st) {
  ProfLaunch prof_(st, "tr_mask_kernel", 0.0, 4.0 * B * T);
  mmf_launch(tr_mask_kernel, dim3((unsigned)(((int64_t)B * T + NT - 1) / NT)), dim3(NT), 0, st, lengths, B, T, w.mask,
             w.lenc);
  return hipGetLastError();
}

// C = epilogue(A W^T + bias): A (n, K) and W (N, K) both stored with the contraction contiguous
GemmJob tr_linear(int n, int N, int K, const float* a, const float* w, const float* bias, float* c, int epi,
                  uint32_t site) {
  GemmJob j = make_job(n, N, c, N, EPI_BIAS | epi);
  j.g.bias = bias;
  j.g.drop_site = site;
  add_src(j, opnd(a, K), opnd(w, K), K);
  return j;
}

// C (n, N) = G W (+ addm): G (n, K) against W (K, N) as stored (a linear layer's data gradient)
GemmJob tr_dgrad(int n, int N, int K, const float* g, const float* w, float* c, const float* addm) {
  GemmJob j = make_job(n, N, c, N, addm ? EPI_ADDMAT : 0);
  j.g.addm = addm;
  j.g.ld_addm = N;
  add_src(j, opnd(g, K), opnd(w, N), K);
  return j;
}

bool tr_null_layer(const mmf_transformer_layer& p) {
  return !p.in_proj_w || !p.in_proj_b || !p.out_proj_w || !p.out_proj_b || !p.linear1_w || !p.linear1_b ||
         !p.linear2_w || !p.linear2_b || !p.norm1_w || !p.norm1_b || !p.norm2_w || !p.norm2_b;
}
bool tr_null_layer(const mmf_transformer_layer_grad& p) {
  return !p.in_proj_w || !p.in_proj_b || !p.out_proj_w || !p.out_proj_b || !p.linear1_w || !p.linear1_b ||
         !p.linear2_w || !p.linear2_b || !p.norm1_w || !p.norm1_b || !p.norm2_w || !p.norm2_b;
}

}  // namespace

}  // namespace mmf

using namespace mmf;

extern "C" {

size_t mmf_transformer_encoder_saved_bytes(int32_t batch, int32_t steps, int32_t hidden, int32_t ffn,
                                           int32_t layers) {
  if (tr_check(batch, steps, hidden, ffn, layers) != MMF_OK) return 0;
  return tr_saved(nullptr, batch, steps, hidden, ffn, layers).bytes;
}

size_t mmf_transformer_encoder_workspace_bytes(int32_t batch, int32_t steps, int32_t hidden, int32_t ffn,
                                               int32_t layers, int32_t backward) {
  if (tr_check(batch, steps, hidden, ffn, layers) != MMF_OK) return 0;
  return tr_carve(nullptr, batch, steps, hidden, ffn, backward != 0).bytes;
}

int mmf_transformer_encoder_forward(const mmf_transformer_desc* d, const mmf_transformer_layer* params,
                                    const float* x, const int64_t* lengths, uint64_t* rng_state, void* saved,
                                    float* pooled, void* workspace, void* stream) {
  if (int rc = tr_check(d)) return rc;
  if (!params || !x || !saved || !pooled || !workspace) return fail(MMF_EINVAL, "transformer_encoder: null buffer");
  for (int k = 0; k < d->layers; ++k)
    if (tr_null_layer(params[k])) return fail(MMF_EINVAL, "transformer_encoder: null parameter in layer %d", k);
  const float p = (d->training && d->dropout > 0.f) ? d->dropout : 0.f;
  if (p > 0.f && !rng_state) return fail(MMF_EINVAL, "transformer_encoder: training with dropout needs rng_state");
  hipStream_t st = (hipStream_t)stream;
  const int B = d->batch, T = d->steps, H = d->hidden, F = d->ffn, n = B * T, hd = H / TR_HEADS;
  const float scale = 1.0f / std::sqrt((float)hd);
  TrSaved sv = tr_saved(saved, B, T, H, F, d->layers);
  TrWs ws = tr_carve(workspace, B, T, H, F, false);
  if (rng_state) STAGE_TRY("transformer.fwd.rng", launch_rng_snapshot(rng_state, sv.rng, st));
  const RngSnap* rng = rng_state ? sv.rng : nullptr;
  STAGE_TRY("transformer.fwd.mask", launch_tr_mask(lengths, B, T, ws, st));
  const float* xin = x;
  for (int k = 0; k < d->layers; ++k) {
    const mmf_transformer_layer& P = params[k];
    const TrLayerSaved& S = sv.l[k];
    const uint32_t site = SITE_TR + 4 * k;
    GemmJob j = tr_linear(n, 3 * H, H, xin, P.in_proj_w, P.in_proj_b, S.qkv, 0, 0);
    STAGE_TRY("transformer.fwd.qkv_gemm", launch_gemm(&j, 1, MODE_RK, MODE_RK, 0.f, rng, st));
    AttnPair a = tr_pair(S, lengths ? ws.mask : nullptr, T, H, k);
    STAGE_TRY("transformer.fwd.attn", launch_attn_fwd(&a, 1, B, TR_HEADS, hd, scale, p, rng, st));
    j = tr_linear(n, H, H, S.o, P.out_proj_w, P.out_proj_b, ws.r, EPI_DROP, site + 1);
    STAGE_TRY("transformer.fwd.out_gemm", launch_gemm(&j, 1, MODE_RK, MODE_RK, p, rng, st));
    STAGE_TRY("transformer.fwd.norm1", launch_ln_fwd(xin, ws.r, P.norm1_w, P.norm1_b, S.z1, S.st1, S.y1, n, H, d->eps, st));
    j = tr_linear(n, F, H, S.y1, P.linear1_w, P.linear1_b, S.h, EPI_RELU | EPI_DROP, site + 2);
    STAGE_TRY("transformer.fwd.linear1_gemm", launch_gemm(&j, 1, MODE_RK, MODE_RK, p, rng, st));
    j = tr_linear(n, H, F, S.h, P.linear2_w, P.linear2_b, ws.r, EPI_DROP, site + 3);
    STAGE_TRY("transformer.fwd.linear2_gemm", launch_gemm(&j, 1, MODE_RK, MODE_RK, p, rng, st));
    STAGE_TRY("transformer.fwd.norm2", launch_ln_fwd(S.y1, ws.r, P.norm2_w, P.norm2_b, S.z2, S.st2, S.y2, n, H, d->eps, st));
    xin = S.y2;
  }
  Stage stage_("transformer.fwd.pool", st);
  ProfLaunch prof_(st, "masked_mean_pool_fwd", 1.0 * n * H, 4.0 * n * H);
  mmf_launch(masked_mean_pool_fwd, dim3(B), dim3(NT), 0, st, xin, (const int32_t*)ws.lenc, T, H, pooled);
  HIP_TRY(hipGetLastError());
  return MMF_OK;
}

int mmf_transformer_encoder_backward(const mmf_transformer_desc* d, const mmf_transformer_layer* params,
                                     const float* x, const int64_t* lengths, const void* saved,
                                     const float* dpooled, void* workspace,
                                     const mmf_transformer_layer_grad* grads, float* dx, void* stream) {
  if (int rc = tr_check(d)) return rc;
  if (!params || !x || !saved || !dpooled || !workspace || !grads)
    return fail(MMF_EINVAL, "transformer_encoder: null buffer");
  for (int k = 0; k < d->layers; ++k)
    if (tr_null_layer(params[k]) || tr_null_layer(grads[k]))
      return fail(MMF_EINVAL, "transformer_encoder: null parameter or gradient in layer %d", k);
  hipStream_t st = (hipStream_t)stream;
  const int B = d->batch, T = d->steps, H = d->hidden, F = d->ffn, n = B * T, hd = H / TR_HEADS;
  const float p = (d->training && d->dropout > 0.f) ? d->dropout : 0.f;
  const float inv_keep = 1.f / (1.f - p);
  const float scale = 1.0f / std::sqrt((float)hd);
  TrSaved sv = tr_saved(const_cast<void*>(saved), B, T, H, F, d->layers);
  TrWs ws = tr_carve(workspace, B, T, H, F, true);
  const RngSnap* rng = p > 0.f ? sv.rng : nullptr;
  STAGE_TRY("transformer.bwd.mask", launch_tr_mask(lengths, B, T, ws, st));
  float* dy = ws.dya;      // the gradient of the current layer's output
  float* dnext = ws.dyb;   // ... of its input
  {
    Stage stage_("transformer.bwd.pool", st);
    ProfLaunch prof_(st, "masked_mean_pool_bwd", 1.0 * n * H, 4.0 * n * H);
    mmf_launch(masked_mean_pool_bwd, dim3((unsigned)(((int64_t)n * (H / 4) + NT - 1) / NT)), dim3(NT), 0, st, dpooled,
               (const int32_t*)ws.lenc, B, T, H, dy);
    HIP_TRY(hipGetLastError());
  }
  for (int k = d->layers - 1; k >= 0; --k) {
    const mmf_transformer_layer& P = params[k];
    const mmf_transformer_layer_grad& G = grads[k];
    const TrLayerSaved& S = sv.l[k];
    const float* xin = k == 0 ? x : sv.l[k - 1].y2;
    const uint32_t site = SITE_TR + 4 * k;
    // LayerNorm2 and the feed-forward branch
    LnBwdArgs n2{S.z2, S.st2, P.norm2_w, dy, ws.dz2, p > 0.f ? ws.dr2 : nullptr, ws.lnpart, n, H, p, site + 3, rng};
    STAGE_TRY("transformer.bwd.norm2", launch_ln_bwd(n2, ws.lnpart2, G.norm2_w, G.norm2_b, st));
    const float* r2 = p > 0.f ? ws.dr2 : ws.dz2;
    GemmJob j = tr_dgrad(n, F, H, r2, P.linear2_w, ws.dh, nullptr);
    j.g.epi |= EPI_GATE;   // through the saved Drop(ReLU(.)): its sign, and the keep scale
    j.g.gate = S.h;
    j.g.ld_gate = F;
    j.g.gate_scale = inv_keep;
    STAGE_TRY("transformer.bwd.dh_gemm", launch_gemm(&j, 1, MODE_RK, MODE_KR, 0.f, rng, st));
    j = tr_dgrad(n, H, F, ws.dh, P.linear1_w, ws.dy1, ws.dz2);   // + the residual path
    STAGE_TRY("transformer.bwd.dy1_gemm", launch_gemm(&j, 1, MODE_RK, MODE_KR, 0.f, rng, st));
    // LayerNorm1 and the attention branch
    LnBwdArgs n1{S.z1, S.st1, P.norm1_w, ws.dy1, ws.dz1, p > 0.f ? ws.dr1 : nullptr, ws.lnpart, n, H, p, site + 1, rng};
    STAGE_TRY("transformer.bwd.norm1", launch_ln_bwd(n1, ws.lnpart2, G.norm1_w, G.norm1_b, st));
    const float* r1 = p > 0.f ? ws.dr1 : ws.dz1;
    j = tr_dgrad(n, H, H, r1, P.out_proj_w, ws.dO, nullptr);
    STAGE_TRY("transformer.bwd.dO_gemm", launch_gemm(&j, 1, MODE_RK, MODE_KR, 0.f, rng, st));
    AttnPair a = tr_pair(S, lengths ? ws.mask : nullptr, T, H, k);
    a.dout = ws.dO; a.dsum = ws.dsum;
    a.dq = ws.dqkv; a.dk = ws.dqkv + H; a.dv = ws.dqkv + 2 * H;
    STAGE_TRY("transformer.bwd.attn", launch_attn_bwd(&a, 1, B, TR_HEADS, hd, scale, p, rng, st));
    float* dxin = k == 0 ? dx : dnext;
    if (dxin) {
      j = tr_dgrad(n, H, 3 * H, ws.dqkv, P.in_proj_w, dxin, ws.dz1);   // + the residual path
      STAGE_TRY("transformer.bwd.dx_gemm", launch_gemm(&j, 1, MODE_RK, MODE_KR, 0.f, rng, st));
    }
    // the layer's weight gradients (the slabs are reused by the next layer: same stream, in order)
    WgradPlan wp;
    Bump slabs(workspace);
    slabs.off = ws.slab_off;
    TrWgradIn in{r2, S.h, ws.dh, S.y1, r1, S.o, ws.dqkv, xin, &G};
    tr_plan_wgrads(wp, slabs, n, H, F, in);
    if (slabs.off + 256 > ws.bytes) return fail(MMF_EINVAL, "internal: workspace overflow");
    STAGE_TRY("transformer.bwd.wgrad_gemm", launch_gemm(wp.jobs.data(), (int)wp.jobs.size(), MODE_KR, MODE_KR, 0.f, rng, st));
    STAGE_TRY("transformer.bwd.wgrad_reduce", launch_reduce(wp.reds.data(), (int)wp.reds.size(), st));
    float* t = dy;
    dy = dnext;
    dnext = t;
  }
  return MMF_OK;
}

}  // extern "C"
