// The CNN sequence encoder's conv stack (src/encoders.py:87-97, 168-175):
//   Conv1d(k=3, pad=1) -> BatchNorm1d -> ReLU -> Conv1d(k=3, pad=1) -> BatchNorm1d -> ReLU -> mean over T
// forward and backward, fp32, channels-last: activations are (B, T, C) contiguous, i.e. (n = B*T, C)
// row-major, so the reference's transpose(1, 2) never materialises.  Conv weights arrive repacked
// as (Cout, 3, Cin).
//
//  A  conv3_gemm_kernel     implicit GEMM on v_mfma_f32_32x32x2_f32: y[r, :] = bias + sum_k a[r+k-1, :] W[:, k, :]^T,
//                           rows r+k-1 outside r's sample are zero.  `a` is the input itself, or
//                           relu(bn(a)) applied while the A tile is staged (normalise-on-load: the
//                           BatchNorm-1 output is never written); the zero padding applies AFTER that.
//                           The data gradient is the same kernel on the flipped, transposed weight.
//  B  bn_stats_partial / bn_stats_finalize   per-channel mean and biased variance over n: per 128-row
//                           chunk the mean and the CENTRED sum of squares (two passes over the chunk),
//                           merged over the chunks in chunk order by Chan's formula.
//  C  bn_relu_pool_kernel   pooled[b, c] = mean_t relu(bn(y2)), one pass over y2.
//  D  bn_bwd_partial / col_reduce / bn_bwd_apply   dz = da [bn(y) > 0]; dbeta = sum dz, dgamma = sum dz xhat
//                           (chunk partials, then a fixed-order reduce: two phases split by a kernel
//                           boundary); dy = gamma rstd (dz - dbeta/n - xhat dgamma/n) (training) or
//                           gamma rstd dz (eval); the conv bias gradient sum dy the same way.
//  E  conv3_wgrad_kernel / wgrad_reduce   dW[co, k, ci] = sum_r dy[r, co] a[r+k-1, ci] on the fp32
//                           matrix cores, split over row ranges into slabs summed in a fixed order.
//
// Every cross-workgroup dependency is a kernel boundary: no atomics, no waits.  Two calls on the
// same inputs give the same bits.  fp32 MFMA at every matmul-precision setting.
#include <cmath>

#include "capi_util.h"
#include "mmf_device.h"

namespace mmf {

namespace {

constexpr int NT = 256;
constexpr int BM = 128, BN = 128, KC = 16;   // conv tile: 128 rows x 128 outputs, 16 input channels per stage
constexpr int WT = 64, WR = 32;              // wgrad tile: 64 co x 64 ci x 3 taps, 32 rows per stage
constexpr int CH = 128;                      // rows per chunk of the column (per-channel) reductions
constexpr int CW = 64;                       // channels per workgroup of the column kernels
enum { ST_MEAN = 0, ST_VAR = 1, ST_RSTD = 2, ST_SCALE = 3, ST_BETA = 4, ST_MLO = 5 };   // rows of a (6, C) stat block

// gamma * (v - mean) * rstd + beta, in the centred form: at a conv bias of 100 the folded form
// v * scale + (beta - mean * scale) cancels two numbers 100 times the result
__device__ __forceinline__ float bn_apply(float v, float mean, float mlo, float scale, float beta) {
  return fmaf((v - mean) - mlo, scale, beta);
}

// ------------------------------------------------------------------------------------------ A
struct ConvArgs {
  const float* a;      // (n, Cin)
  const float* stat;   // null: a as it is; else the (6, Cin) statistics: a := relu(bn(a)) on load
  const float* w;      // (N, 3, Cin)
  const float* bias;   // (N) or null
  float* y;            // (n, N)
  int n, T, Cin, N;
};

__global__ __launch_bounds__(NT) void conv3_gemm_kernel(ConvArgs p) {
  __shared__ float As[BM + 2][KC + 1];   // rows r0 - 1 .. r0 + BM (the halo), activated
  __shared__ float Bs[3][BN][KC + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, half = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;   // the wave's 64 x 64 quadrant, 2 x 2 MFMA tiles
  const int r0 = blockIdx.x * BM;
  const int j0 = blockIdx.y * BN;
  // this lane's two A rows: which taps stay inside the row's own sample
  bool ok0[2], ok1[2], ok2[2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int r = r0 + wm * 64 + mi * 32 + li;
    const int t = r % p.T;
    ok1[mi] = r < p.n;
    ok0[mi] = ok1[mi] && t > 0;
    ok2[mi] = ok1[mi] && t + 1 < p.T;
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[mi][ni][g] = 0.f;

  for (int c0 = 0; c0 < p.Cin; c0 += KC) {
    __syncthreads();
    for (int e = tid; e < (BM + 2) * KC; e += NT) {
      const int rr = e / KC, cc = e % KC;
      const int gr = r0 - 1 + rr, gc = c0 + cc;
      float v = 0.f;
      if (gr >= 0 && gr < p.n && gc < p.Cin) {
        v = p.a[(int64_t)gr * p.Cin + gc];
        if (p.stat)
          v = fmaxf(bn_apply(v, p.stat[ST_MEAN * p.Cin + gc], p.stat[ST_MLO * p.Cin + gc],
                             p.stat[ST_SCALE * p.Cin + gc], p.stat[ST_BETA * p.Cin + gc]), 0.f);
      }
      As[rr][cc] = v;
    }
    for (int e = tid; e < 3 * BN * KC; e += NT) {
      const int cc = e % KC, jk = e / KC;   // jk = j * 3 + k: the weight's (N, 3) rows in order
      const int k = jk % 3, j = jk / 3;
      const int gj = j0 + j, gc = c0 + cc;
      float v = 0.f;
      if (gj < p.N && gc < p.Cin) v = p.w[((int64_t)gj * 3 + k) * p.Cin + gc];
      Bs[k][j][cc] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const bool v0 = k == 0 ? ok0[0] : (k == 1 ? ok1[0] : ok2[0]);
      const bool v1 = k == 0 ? ok0[1] : (k == 1 ? ok1[1] : ok2[1]);
#pragma unroll
      for (int s = 0; s < KC / 2; ++s) {
        const int kk = 2 * s + half;
        // output row i of the tile takes tap k from staged row i + k (= global row i + k - 1)
        float a0 = As[wm * 64 + li + k][kk];
        float a1 = As[wm * 64 + 32 + li + k][kk];
        a0 = v0 ? a0 : 0.f;
        a1 = v1 ? a1 : 0.f;
        const float b0 = Bs[k][wn * 64 + li][kk];
        const float b1 = Bs[k][wn * 64 + 32 + li][kk];
        acc[0][0] = mfma32(a0, b0, acc[0][0]);
        acc[0][1] = mfma32(a0, b1, acc[0][1]);
        acc[1][0] = mfma32(a1, b0, acc[1][0]);
        acc[1][1] = mfma32(a1, b1, acc[1][1]);
      }
    }
  }
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int col = j0 + wn * 64 + ni * 32 + li;
    if (col >= p.N) continue;
    const float bj = p.bias ? p.bias[col] : 0.f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int row = r0 + wm * 64 + mi * 32 + acc_row(g, half);
        if (row < p.n) p.y[(int64_t)row * p.N + col] = acc[mi][ni][g] + bj;
      }
    }
  }
}

// wT[ci][k][co] = w[co][2 - k][ci]: the weight of the data-gradient convolution
__global__ __launch_bounds__(NT) void conv3_flip_weight(const float* w, float* wT, int Cout, int Cin) {
  const int e = blockIdx.x * NT + threadIdx.x;
  if (e >= Cout * 3 * Cin) return;
  const int co = e % Cout, k = (e / Cout) % 3, ci = e / (3 * Cout);
  wT[e] = w[((int64_t)co * 3 + (2 - k)) * Cin + ci];
}

// ------------------------------------------------------------------------------------------ E
struct WgradArgs {
  const float* dy;     // (n, Cout)
  const float* a;      // (n, Cin)
  const float* stat;   // as ConvArgs::stat
  float* part;         // (nsplit, Cout, 3, Cin)
  int n, T, Cin, Cout, rows, tiles_ci;   // rows per split (a multiple of WR)
};

__global__ __launch_bounds__(NT) void conv3_wgrad_kernel(WgradArgs p) {
  __shared__ float Ds[WR][WT];
  __shared__ float Xs[WR + 2][WT];   // a rows rb - 1 .. rb + WR
  __shared__ int Fl[WR + 2];         // per a row q: bit 0 = a tap-0 source (t(q) != T-1), bit 1 = a tap-2 source (t(q) != 0)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, half = lane >> 5;
  const int wco = wave >> 1, wci = wave & 1;
  const int co0 = (blockIdx.x / p.tiles_ci) * WT, ci0 = (blockIdx.x % p.tiles_ci) * WT;
  const int split = blockIdx.y;
  const int rs = split * p.rows;
  const int re = min(p.n, rs + p.rows);
  f32x16 acc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[k][g] = 0.f;

  for (int rb = rs; rb < re; rb += WR) {
    __syncthreads();
    for (int e = tid; e < WR * WT; e += NT) {
      const int rr = e / WT, cc = e % WT;
      const int r = rb + rr, c = co0 + cc;
      Ds[rr][cc] = (r < re && c < p.Cout) ? p.dy[(int64_t)r * p.Cout + c] : 0.f;
    }
    for (int e = tid; e < (WR + 2) * WT; e += NT) {
      const int rr = e / WT, cc = e % WT;
      const int q = rb - 1 + rr, c = ci0 + cc;
      float v = 0.f;
      if (q >= 0 && q < p.n && c < p.Cin) {
        v = p.a[(int64_t)q * p.Cin + c];
        if (p.stat)
          v = fmaxf(bn_apply(v, p.stat[ST_MEAN * p.Cin + c], p.stat[ST_MLO * p.Cin + c], p.stat[ST_SCALE * p.Cin + c],
                             p.stat[ST_BETA * p.Cin + c]), 0.f);
      }
      Xs[rr][cc] = v;
    }
    if (tid < WR + 2) {
      const int q = rb - 1 + tid;
      int f = 0;
      if (q >= 0 && q < p.n) {
        const int t = q % p.T;
        f = (t != p.T - 1 ? 1 : 0) | (t != 0 ? 2 : 0);
      }
      Fl[tid] = f;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < WR / 2; ++s) {
      const int kk = 2 * s + half;   // row rb + kk; its tap k reads a row rb + kk + k - 1 = staged row kk + k
      const float d = Ds[kk][wco * 32 + li];
      float x0 = Xs[kk][wci * 32 + li];
      const float x1 = Xs[kk + 1][wci * 32 + li];
      float x2 = Xs[kk + 2][wci * 32 + li];
      x0 = (Fl[kk] & 1) ? x0 : 0.f;
      x2 = (Fl[kk + 2] & 2) ? x2 : 0.f;
      acc[0] = mfma32(d, x0, acc[0]);
      acc[1] = mfma32(d, x1, acc[1]);
      acc[2] = mfma32(d, x2, acc[2]);
    }
  }
  const int ci = ci0 + wci * 32 + li;
  if (ci < p.Cin) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int co = co0 + wco * 32 + acc_row(g, half);
        if (co < p.Cout) p.part[(((int64_t)split * p.Cout + co) * 3 + k) * p.Cin + ci] = acc[k][g];
      }
  }
}

// out[e] = sum_s part[s][e] in split order
__global__ __launch_bounds__(NT) void wgrad_reduce(const float* part, int nsplit, int64_t E, float* out) {
  const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (e >= E) return;
  float s = 0.f;
  for (int i = 0; i < nsplit; ++i) s += part[(int64_t)i * E + e];
  out[e] = s;
}

// --------------------------------------------------------------------------- column kernels
// A workgroup owns CW channels (lanes along the channels: coalesced rows) and the rows of one
// chunk, 4 row lanes each taking every 4th row; the 4 partial sums are combined in a fixed order.
__device__ __forceinline__ float rows4_sum(float v, float (*red)[CW], int ry, int cx) {
  __syncthreads();
  red[ry][cx] = v;
  __syncthreads();
  return (red[0][cx] + red[1][cx]) + (red[2][cx] + red[3][cx]);
}

// B: per chunk and channel, part[chunk][0] = a pivot p (the chunk's first value), [1] = sum (y - p)
// (small numbers whatever the channel's offset: the chunk mean p + sum / count is then good to the
// last bit, where a plain sum of values near 100 loses three digits of the mean), [2] = the sum of
// squares centred on that chunk mean
__global__ __launch_bounds__(NT) void bn_stats_partial(const float* y, int n, int C, float* part) {
  __shared__ float red[4][CW];
  const int cx = threadIdx.x & (CW - 1), ry = threadIdx.x / CW;
  const int c = blockIdx.y * CW + cx;
  const int rs = blockIdx.x * CH, re = min(n, rs + CH);
  const float piv = c < C ? y[(int64_t)rs * C + c] : 0.f;
  float s = 0.f;
  if (c < C)
    for (int r = rs + ry; r < re; r += 4) s += y[(int64_t)r * C + c] - piv;
  s = rows4_sum(s, red, ry, cx);
  const float dm = s / (float)(re - rs);   // chunk mean - pivot
  float m2 = 0.f;
  if (c < C)
    for (int r = rs + ry; r < re; r += 4) {
      const float d = (y[(int64_t)r * C + c] - piv) - dm;
      m2 = fmaf(d, d, m2);
    }
  m2 = rows4_sum(m2, red, ry, cx);
  if (ry == 0 && c < C) {
    part[((int64_t)blockIdx.x * 3 + 0) * C + c] = piv;
    part[((int64_t)blockIdx.x * 3 + 1) * C + c] = s;
    part[((int64_t)blockIdx.x * 3 + 2) * C + c] = m2;
  }
}

// Chan's merge of the chunks in chunk order, in double (training), or the running statistics (eval),
// and the BatchNorm coefficients: stat = (mean, biased var, rstd, gamma * rstd, beta, mean_lo), each
// (C).  mean + mean_lo is the mean to twice fp32's digits: xhat = ((y - mean) - mean_lo) rstd then
// sums to zero over the batch to rounding, and with it the conv bias gradient.
__global__ __launch_bounds__(NT) void bn_stats_finalize(const float* part, int nchunk, int n, int C, const float* rmean,
                                                        const float* rvar, const float* gamma, const float* beta,
                                                        float eps, float* stat) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= C) return;
  float mean, mlo = 0.f, var;
  if (part) {
    double cnt = 0.0, m2 = 0.0, mu = 0.0;
    for (int i = 0; i < nchunk; ++i) {
      const double nb = (double)min(CH, n - i * CH);
      const double mb = (double)part[((int64_t)i * 3 + 0) * C + c] + (double)part[((int64_t)i * 3 + 1) * C + c] / nb;
      const double qb = (double)part[((int64_t)i * 3 + 2) * C + c];
      const double tot = cnt + nb;
      const double delta = mb - mu;
      mu += delta * (nb / tot);
      m2 += qb + delta * delta * (cnt * nb / tot);
      cnt = tot;
    }
    mean = (float)mu;
    mlo = (float)(mu - (double)mean);
    var = (float)(m2 / (double)n);
  } else {
    mean = rmean[c];
    var = rvar[c];
  }
  const float rstd = 1.f / sqrtf(var + eps);
  stat[ST_MEAN * C + c] = mean;
  stat[ST_VAR * C + c] = var;
  stat[ST_RSTD * C + c] = rstd;
  stat[ST_SCALE * C + c] = gamma[c] * rstd;
  stat[ST_BETA * C + c] = beta[c];
  stat[ST_MLO * C + c] = mlo;
}

// C: pooled[b][c] = (1 / T) sum_t relu(bn(y[b, t, c]))
__global__ __launch_bounds__(NT) void bn_relu_pool_kernel(const float* y, const float* stat, int T, int C,
                                                          float* pooled) {
  __shared__ float red[4][CW];
  const int cx = threadIdx.x & (CW - 1), ry = threadIdx.x / CW;
  const int c = blockIdx.y * CW + cx;
  const int b = blockIdx.x;
  float s = 0.f;
  if (c < C) {
    const float mean = stat[ST_MEAN * C + c], mlo = stat[ST_MLO * C + c];
    const float scale = stat[ST_SCALE * C + c], beta = stat[ST_BETA * C + c];
    const float* yb = y + (int64_t)b * T * C + c;
    for (int t = ry; t < T; t += 4) s += fmaxf(bn_apply(yb[(int64_t)t * C], mean, mlo, scale, beta), 0.f);
  }
  s = rows4_sum(s, red, ry, cx);
  if (ry == 0 && c < C) pooled[(int64_t)b * C + c] = s / (float)T;
}

// D.  The upstream gradient of a layer's ReLU output: da (n, C), or dpooled (B, C) / T broadcast over t.
struct BnBwdArgs {
  const float* y;        // (n, C) the conv output the BatchNorm normalised
  const float* stat;     // (6, C)
  const float* da;       // (n, C) or null
  const float* dpooled;  // (B, C) (da null)
  float inv_T;
  int n, T, C, training;
  const float* dgamma;   // (C) reduced sums (bn_bwd_apply)
  const float* dbeta;    // (C)
  float* dy;             // (n, C) (bn_bwd_apply; may alias da)
  float* part;           // bn_bwd_partial: (nchunk, 2, C) sum dz | sum dz xhat;  bn_bwd_apply: (nchunk, 1, C) sum dy
};

struct BnCoef { float mean, mlo, rstd, scale, beta; };
__device__ __forceinline__ BnCoef bn_coef(const float* stat, int C, int c) {
  return BnCoef{stat[ST_MEAN * C + c], stat[ST_MLO * C + c], stat[ST_RSTD * C + c], stat[ST_SCALE * C + c],
                stat[ST_BETA * C + c]};
}

__device__ __forceinline__ float bn_bwd_dz(const BnBwdArgs& a, int r, int c, float v, const BnCoef& k) {
  const float g = a.da ? a.da[(int64_t)r * a.C + c] : a.dpooled[(int64_t)(r / a.T) * a.C + c] * a.inv_T;
  return bn_apply(v, k.mean, k.mlo, k.scale, k.beta) > 0.f ? g : 0.f;
}

__global__ __launch_bounds__(NT) void bn_bwd_partial(BnBwdArgs a) {
  __shared__ float red[4][CW];
  const int cx = threadIdx.x & (CW - 1), ry = threadIdx.x / CW;
  const int c = blockIdx.y * CW + cx;
  const int rs = blockIdx.x * CH, re = min(a.n, rs + CH);
  float s0 = 0.f, s1 = 0.f;
  if (c < a.C) {
    const BnCoef k = bn_coef(a.stat, a.C, c);
    for (int r = rs + ry; r < re; r += 4) {
      const float v = a.y[(int64_t)r * a.C + c];
      const float dz = bn_bwd_dz(a, r, c, v, k);
      s0 += dz;
      s1 = fmaf(dz, ((v - k.mean) - k.mlo) * k.rstd, s1);
    }
  }
  s0 = rows4_sum(s0, red, ry, cx);
  s1 = rows4_sum(s1, red, ry, cx);
  if (ry == 0 && c < a.C) {
    a.part[((int64_t)blockIdx.x * 2 + 0) * a.C + c] = s0;
    a.part[((int64_t)blockIdx.x * 2 + 1) * a.C + c] = s1;
  }
}

// out_k[c] = sum over the chunks of part[chunk][k][c], chunk order, k < K <= 2
__global__ __launch_bounds__(NT) void col_reduce(const float* part, int nchunk, int K, int C, float* out0,
                                                 float* out1) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= C) return;
  for (int k = 0; k < K; ++k) {
    float s = 0.f;
    for (int i = 0; i < nchunk; ++i) s += part[((int64_t)i * K + k) * C + c];
    (k == 0 ? out0 : out1)[c] = s;
  }
}

__global__ __launch_bounds__(NT) void bn_bwd_apply(BnBwdArgs a) {
  __shared__ float red[4][CW];
  const int cx = threadIdx.x & (CW - 1), ry = threadIdx.x / CW;
  const int c = blockIdx.y * CW + cx;
  const int rs = blockIdx.x * CH, re = min(a.n, rs + CH);
  float s = 0.f;
  if (c < a.C) {
    const BnCoef k = bn_coef(a.stat, a.C, c);
    const float mb = a.training ? a.dbeta[c] / (float)a.n : 0.f;
    const float mg = a.training ? a.dgamma[c] / (float)a.n : 0.f;
    for (int r = rs + ry; r < re; r += 4) {
      const float v = a.y[(int64_t)r * a.C + c];
      const float dz = bn_bwd_dz(a, r, c, v, k);
      const float xh = ((v - k.mean) - k.mlo) * k.rstd;
      const float d = k.scale * ((dz - mb) - xh * mg);
      a.dy[(int64_t)r * a.C + c] = d;
      s += d;
    }
  }
  s = rows4_sum(s, red, ry, cx);
  if (ry == 0 && c < a.C) a.part[(int64_t)blockIdx.x * a.C + c] = s;
}

// ------------------------------------------------------------------------------------------ host
constexpr int CONV_MAX_HIDDEN = 512, CONV_MAX_IN = 4096;

int conv_check(int batch, int steps, int in_dim, int hidden) {
  if (batch < 0 || steps < 0 || in_dim < 1 || hidden < 1) return fail(MMF_EINVAL, "conv_encoder: bad shape");
  if (batch == 0 || steps == 0) return fail(MMF_EINVAL, "conv_encoder: empty input (batch * steps == 0)");
  if (hidden % 32 != 0 || hidden > CONV_MAX_HIDDEN)
    return fail(MMF_ELIMIT, "conv_encoder: hidden %d is not a multiple of 32 up to %d", hidden, CONV_MAX_HIDDEN);
  if (in_dim > CONV_MAX_IN) return fail(MMF_ELIMIT, "conv_encoder: in_dim %d > %d", in_dim, CONV_MAX_IN);
  if ((int64_t)batch * steps > (int64_t)1 << 24)
    return fail(MMF_ELIMIT, "conv_encoder: batch * steps %lld > 2^24", (long long)batch * steps);
  return MMF_OK;
}

inline int nchunks(int n) { return (n + CH - 1) / CH; }

// the row split of a weight gradient: about 1024 workgroups over the (co, ci) tiles and splits,
// at most 32 splits, at least 4 stages per split
void wgrad_split(int n, int Cin, int Cout, int& nsplit, int& rows) {
  const int tiles = ((Cout + WT - 1) / WT) * ((Cin + WT - 1) / WT);
  int want = 1024 / tiles;
  want = want < 1 ? 1 : (want > 32 ? 32 : want);
  rows = (n + want - 1) / want;
  rows = (rows + WR - 1) / WR * WR;
  if (rows < 4 * WR) rows = 4 * WR;
  nsplit = (n + rows - 1) / rows;
}

struct ConvWs {
  float* bnpart;   // (nchunk, 3, C)
  float* dy2;      // (n, C)
  float* dy1;      // (n, C): the data gradient of conv 2, then dy1 in place
  float* wT;       // (max(C, Cin), 3, C)
  float* wpart;    // the larger of the two weight gradients' slabs
  size_t bytes;
};

ConvWs conv_carve(void* base, int n, int Cin, int C, bool backward) {
  Bump ws(base);
  ConvWs w{};
  w.bnpart = ws.take<float>((size_t)nchunks(n) * 3 * C);
  if (backward) {
    w.dy2 = ws.take<float>((size_t)n * C);
    w.dy1 = ws.take<float>((size_t)n * C);
    w.wT = ws.take<float>((size_t)3 * C * (C > Cin ? C : Cin));
    int s1, r1, s2, r2;
    wgrad_split(n, Cin, C, s1, r1);
    wgrad_split(n, C, C, s2, r2);
    const size_t e1 = (size_t)s1 * C * 3 * Cin, e2 = (size_t)s2 * C * 3 * C;
    w.wpart = ws.take<float>(e1 > e2 ? e1 : e2);
  }
  w.bytes = ws.off + 256;
  return w;
}

hipError_t launch_conv(const float* a, const float* stat, const float* w, const float* bias, float* y, int n, int T,
                       int Cin, int N, hipStream_t st) {
  ConvArgs p{a, stat, w, bias, y, n, T, Cin, N};
  ProfLaunch prof_(st, "conv3_gemm_kernel", 6.0 * n * Cin * N, 4.0 * ((double)n * (Cin + N) + 3.0 * Cin * N));
  mmf_launch(conv3_gemm_kernel, dim3((n + BM - 1) / BM, (N + BN - 1) / BN), dim3(NT), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_stats(const float* y, int n, int C, const float* rmean, const float* rvar, const float* gamma,
                        const float* beta, float eps, bool training, float* part, float* stat, hipStream_t st) {
  if (training) {
    ProfLaunch prof_(st, "bn_stats_partial", 4.0 * n * C, 4.0 * n * C);
    mmf_launch(bn_stats_partial, dim3(nchunks(n), (C + CW - 1) / CW), dim3(NT), 0, st, y, n, C, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  ProfLaunch prof_(st, "bn_stats_finalize", 8.0 * nchunks(n) * C, 8.0 * nchunks(n) * C);
  mmf_launch(bn_stats_finalize, dim3((C + NT - 1) / NT), dim3(NT), 0, st, training ? (const float*)part : nullptr,
             nchunks(n), n, C, rmean, rvar, gamma, beta, eps, stat);
  return hipGetLastError();
}

// dbeta, dgamma, dy and the conv bias gradient sum dy of one BatchNorm + ReLU
hipError_t launch_bn_bwd(BnBwdArgs a, float* dgamma, float* dbeta, float* dbias, float* part, hipStream_t st) {
  const dim3 grid(nchunks(a.n), (a.C + CW - 1) / CW), cgrid((a.C + NT - 1) / NT);
  const double elems = (double)a.n * a.C;
  hipError_t e;
  a.part = part;
  {
    ProfLaunch prof_(st, "bn_bwd_partial", 6.0 * elems, 8.0 * elems);
    mmf_launch(bn_bwd_partial, grid, dim3(NT), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  {
    ProfLaunch prof_(st, "col_reduce", 2.0 * grid.x * a.C, 8.0 * grid.x * a.C);
    mmf_launch(col_reduce, cgrid, dim3(NT), 0, st, (const float*)part, (int)grid.x, 2, a.C, dbeta, dgamma);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  a.dgamma = dgamma;
  a.dbeta = dbeta;
  {
    ProfLaunch prof_(st, "bn_bwd_apply", 8.0 * elems, 12.0 * elems);
    mmf_launch(bn_bwd_apply, grid, dim3(NT), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  ProfLaunch prof_(st, "col_reduce", 1.0 * grid.x * a.C, 4.0 * grid.x * a.C);
  mmf_launch(col_reduce, cgrid, dim3(NT), 0, st, (const float*)part, (int)grid.x, 1, a.C, dbias, (float*)nullptr);
  return hipGetLastError();
}

hipError_t launch_wgrad(const float* dy, const float* a, const float* stat, float* part, float* dw, int n, int T,
                        int Cin, int Cout, hipStream_t st) {
  int nsplit, rows;
  wgrad_split(n, Cin, Cout, nsplit, rows);
  const int tiles_ci = (Cin + WT - 1) / WT, tiles_co = (Cout + WT - 1) / WT;
  WgradArgs p{dy, a, stat, part, n, T, Cin, Cout, rows, tiles_ci};
  const int64_t E = (int64_t)Cout * 3 * Cin;
  {
    ProfLaunch prof_(st, "conv3_wgrad_kernel", 6.0 * n * Cin * Cout, 4.0 * ((double)n * (Cin + Cout) + 3.0 * Cin * Cout));
    mmf_launch(conv3_wgrad_kernel, dim3(tiles_co * tiles_ci, nsplit), dim3(NT), 0, st, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  ProfLaunch prof_(st, "wgrad_reduce", (double)nsplit * E, 4.0 * nsplit * E);
  mmf_launch(wgrad_reduce, dim3((unsigned)((E + NT - 1) / NT)), dim3(NT), 0, st, (const float*)part, nsplit, E, dw);
  return hipGetLastError();
}

// the data gradient (n, Cin) of a conv with weight w (Cout, 3, Cin) from dy (n, Cout)
hipError_t launch_dgrad(const float* dy, const float* w, float* wT, float* da, int n, int T, int Cin, int Cout,
                        hipStream_t st) {
  {
    const int E = Cout * 3 * Cin;
    ProfLaunch prof_(st, "conv3_flip_weight", 0.0, 8.0 * E);
    mmf_launch(conv3_flip_weight, dim3((E + NT - 1) / NT), dim3(NT), 0, st, w, wT, Cout, Cin);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return launch_conv(dy, nullptr, wT, nullptr, da, n, T, Cout, Cin, st);
}

}  // namespace

}  // namespace mmf

using namespace mmf;

extern "C" {

size_t mmf_conv_encoder_workspace_bytes(int32_t batch, int32_t steps, int32_t in_dim, int32_t hidden,
                                        int32_t backward) {
  if (conv_check(batch, steps, in_dim, hidden) != MMF_OK) return 0;
  return conv_carve(nullptr, batch * steps, in_dim, hidden, backward != 0).bytes;
}

int mmf_conv_encoder_forward(int32_t batch, int32_t steps, int32_t in_dim, int32_t hidden, int32_t training,
                             const float* x, const float* w1, const float* b1, const float* gamma1,
                             const float* beta1, const float* rmean1, const float* rvar1, float eps1,
                             const float* w2, const float* b2, const float* gamma2, const float* beta2,
                             const float* rmean2, const float* rvar2, float eps2, float* y1, float* y2,
                             float* stat1, float* stat2, float* pooled, void* workspace, void* stream) {
  if (int rc = conv_check(batch, steps, in_dim, hidden)) return rc;
  if (!(eps1 >= 0.f) || !(eps2 >= 0.f)) return fail(MMF_EINVAL, "conv_encoder: negative eps");
  if (!x || !w1 || !w2 || !y1 || !y2 || !stat1 || !stat2 || !pooled || !workspace)
    return fail(MMF_EINVAL, "conv_encoder: null buffer");
  hipStream_t st = (hipStream_t)stream;
  const int n = batch * steps, T = steps, C = hidden;
  const bool train = training != 0;
  ConvWs ws = conv_carve(workspace, n, in_dim, C, false);
  Stage stage_("conv_encoder.forward", st);
  HIP_TRY(launch_conv(x, nullptr, w1, b1, y1, n, T, in_dim, C, st));
  HIP_TRY(launch_stats(y1, n, C, rmean1, rvar1, gamma1, beta1, eps1, train, ws.bnpart, stat1, st));
  HIP_TRY(launch_conv(y1, stat1, w2, b2, y2, n, T, C, C, st));
  HIP_TRY(launch_stats(y2, n, C, rmean2, rvar2, gamma2, beta2, eps2, train, ws.bnpart, stat2, st));
  ProfLaunch prof_(st, "bn_relu_pool_kernel", 3.0 * n * C, 4.0 * n * C);
  mmf_launch(bn_relu_pool_kernel, dim3(batch, (C + CW - 1) / CW), dim3(NT), 0, st, (const float*)y2,
             (const float*)stat2, T, C, pooled);
  HIP_TRY(hipGetLastError());
  return MMF_OK;
}

int mmf_conv_encoder_backward(int32_t batch, int32_t steps, int32_t in_dim, int32_t hidden, int32_t training,
                              const float* x, const float* w1, const float* w2, const float* y1, const float* y2,
                              const float* stat1, const float* stat2, const float* dpooled, float* dx, float* dw1,
                              float* db1, float* dgamma1, float* dbeta1, float* dw2, float* db2, float* dgamma2,
                              float* dbeta2, void* workspace, void* stream) {
  if (int rc = conv_check(batch, steps, in_dim, hidden)) return rc;
  if (!x || !w1 || !w2 || !y1 || !y2 || !stat1 || !stat2 || !dpooled || !dw1 || !db1 || !dgamma1 || !dbeta1 || !dw2 ||
      !db2 || !dgamma2 || !dbeta2 || !workspace)
    return fail(MMF_EINVAL, "conv_encoder: null buffer");
  hipStream_t st = (hipStream_t)stream;
  const int n = batch * steps, T = steps, C = hidden;
  ConvWs ws = conv_carve(workspace, n, in_dim, C, true);
  Stage stage_("conv_encoder.backward", st);
  // layer 2: BatchNorm + ReLU under the mean over T
  BnBwdArgs a2{};
  a2.y = y2; a2.stat = stat2; a2.dpooled = dpooled; a2.inv_T = 1.f / (float)T;
  a2.n = n; a2.T = T; a2.C = C; a2.training = training != 0; a2.dy = ws.dy2;
  HIP_TRY(launch_bn_bwd(a2, dgamma2, dbeta2, db2, ws.bnpart, st));
  HIP_TRY(launch_wgrad(ws.dy2, y1, stat1, ws.wpart, dw2, n, T, C, C, st));   // a1 = relu(bn1(y1)) on load
  HIP_TRY(launch_dgrad(ws.dy2, w2, ws.wT, ws.dy1, n, T, C, C, st));
  // layer 1
  BnBwdArgs a1{};
  a1.y = y1; a1.stat = stat1; a1.da = ws.dy1; a1.inv_T = 0.f;
  a1.n = n; a1.T = T; a1.C = C; a1.training = training != 0; a1.dy = ws.dy1;
  HIP_TRY(launch_bn_bwd(a1, dgamma1, dbeta1, db1, ws.bnpart, st));
  HIP_TRY(launch_wgrad(ws.dy1, x, nullptr, ws.wpart, dw1, n, T, in_dim, C, st));
  if (dx) HIP_TRY(launch_dgrad(ws.dy1, w1, ws.wT, dx, n, T, in_dim, C, st));
  return MMF_OK;
}

}  // extern "C"
