// Uncertainty quantification kernels (src/uncertainty.py):
//
//  * mc_reduce_kernel: the reduction of MCDropoutUncertainty.forward (:58-66) and
//    EnsembleUncertainty.predict_with_uncertainty (:487-491) over a stack of S logit
//    samples (S, B, C): mean_s z, mean_s softmax(z) and mean_c var_s(softmax(z)) (population
//    variance).  One wave64 per batch row, four rows per workgroup; lane l owns classes
//    l, l + 64, ... (at most 16, C <= 1024) and keeps their running statistics in registers
//    across the S loop, so the stack is read exactly once, coalesced along C.  The variance is
//    accumulated in Welford's shifted form: the softmax outputs of a confident model differ
//    between dropout samples in the 3rd-5th digit, which E[p^2] - E[p]^2 cancels away in fp32.
//    With one sample the update is mean = p, M2 += p * (p - p): the variance is exactly 0.
//
//  * mmf_hybrid_mc_forward: S forwards of the HybridFusion plan the descriptor selects (each
//    advances the dropout offset by one on the device, so the samples draw distinct masks), every
//    sample's logits into its slot of the stack, then one mc_reduce_kernel launch.
//
//  * temperature_nll_kernel: TemperatureScaling.calibrate's closure (:431-435), the mean
//    cross-entropy of z / T and its derivative in T, T read from the device.  One wave per row in
//    a grid-stride loop, an online softmax (one pass over the logits); the per-workgroup partial
//    sums are reduced by a second one-workgroup launch in a fixed order (bit-identical reruns).
//
//  * uncertainty_fusion_fwd / _bwd: UncertaintyWeightedFusion.forward (:305-362),
//    w = mask / (u + eps) normalised by (sum + 1e-8) where the sum > 0, else the mask-uniform
//    fallback (1 / M where the mask is empty); the backward passes the selected branch's
//    gradient only, as autograd through torch.where does.
//
// All fp32; every entry point only enqueues on the caller's stream.
#include <cmath>

#include "capi_util.h"

namespace mmf {

namespace {

constexpr int NT = 256;
constexpr int ROWS_PER_BLOCK = NT / 64;
constexpr int MAX_CLASSES = 1024;   // 16 classes per lane of a wave64
constexpr int UF_MAX_M = 64;
constexpr int NLL_MAX_BLOCKS = 1024;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

struct McArgs {
  int S, B, C;
  const float* stack;   // (S, B, C)
  float* mean_logits;   // (B, C) or null
  float* mean_probs;    // (B, C) or null
  float* variance;      // (B) or null
};

// NJ = classes per lane (ceil(C / 64) rounded up to a power of two)
template <int NJ>
__global__ __launch_bounds__(NT) void mc_reduce_kernel(McArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (b >= a.B) return;   // (whole waves leave: no block-wide barrier below)
  float zsum[NJ], pmean[NJ], m2[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) zsum[j] = pmean[j] = m2[j] = 0.f;
  for (int s = 0; s < a.S; ++s) {
    const float* row = a.stack + ((int64_t)s * a.B + b) * a.C;
    float z[NJ];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      z[j] = c < a.C ? row[c] : -INFINITY;
      mx = fmaxf(mx, z[j]);
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      z[j] = c < a.C ? z[j] : 0.f;
      const float e = c < a.C ? expf(z[j] - mx) : 0.f;
      zsum[j] += z[j];
      z[j] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    const float inv_n = 1.f / (float)(s + 1);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const float p = z[j] / sum;
      const float delta = p - pmean[j];
      pmean[j] = fmaf(delta, inv_n, pmean[j]);
      m2[j] = fmaf(delta, p - pmean[j], m2[j]);
    }
  }
  const float inv_s = 1.f / (float)a.S;
  float vsum = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < a.C) {
      const int64_t o = (int64_t)b * a.C + c;
      if (a.mean_logits) a.mean_logits[o] = zsum[j] * inv_s;
      if (a.mean_probs) a.mean_probs[o] = pmean[j];
      vsum += m2[j];
    }
  }
  vsum = wave_sum(vsum);
  if (a.variance && lane == 0) a.variance[b] = a.S > 1 ? vsum * inv_s / (float)a.C : 0.f;
}

hipError_t launch_mc_reduce(const McArgs& a, hipStream_t st) {
  const dim3 grid((a.B + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), block(NT);
  ProfLaunch prof_(st, "mc_reduce_kernel", 12.0 * a.S * a.B * a.C,
                   4.0 * a.B * ((double)a.S * a.C + 2.0 * a.C + 1));
  const int nj = (a.C + 63) / 64;
  if (nj <= 1) mmf_launch(mc_reduce_kernel<1>, grid, block, 0, st, a);
  else if (nj <= 2) mmf_launch(mc_reduce_kernel<2>, grid, block, 0, st, a);
  else if (nj <= 4) mmf_launch(mc_reduce_kernel<4>, grid, block, 0, st, a);
  else if (nj <= 8) mmf_launch(mc_reduce_kernel<8>, grid, block, 0, st, a);
  else mmf_launch(mc_reduce_kernel<16>, grid, block, 0, st, a);
  return hipGetLastError();
}

int check_mc(int32_t samples, int32_t batch, int32_t classes) {
  if (samples < 1) return fail(MMF_EINVAL, "mc_reduce: samples must be >= 1, got %d", samples);
  if (batch < 0 || classes < 1) return fail(MMF_EINVAL, "mc_reduce: bad shape");
  if (classes > MAX_CLASSES) return fail(MMF_ELIMIT, "mc_reduce: %d classes > %d", classes, MAX_CLASSES);
  return MMF_OK;
}

struct NllArgs {
  int64_t n;
  int C;
  const float* logits;     // (n, C)
  const int64_t* labels;   // (n)
  const float* temp;       // (1) device
  float* part;             // (gridDim.x, 2): loss | sum_i (z_y - sum_c p_c z_c) partial sums
};

__global__ __launch_bounds__(NT) void temperature_nll_kernel(NllArgs a) {
  __shared__ float red[2 * ROWS_PER_BLOCK];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float inv_t = 1.f / a.temp[0];
  float loss = 0.f, dnum = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * ROWS_PER_BLOCK + w; i < a.n; i += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
    const float* row = a.logits + i * a.C;
    const int64_t y = a.labels[i];
    const bool ok = y >= 0 && y < a.C;   // (torch raises; never used as an index otherwise)
    const float zy = ok ? row[y] : NAN;
    const float ty = zy * inv_t;
    // Both sums are taken relative to the label's class, so a confidently right row loses no
    // digits: loss = log(1 + sum_{c != y} e^(t_c - t_y)), z_y - sum_c p_c z_c =
    // -sum_{c != y} p_c (z_c - z_y).  Online softmax of t = z / T over the classes c != y per
    // lane: running max m, sum of e^(t - m), sum of e^(t - m) (z - z_y).
    float m = -INFINITY, se = 0.f, sez = 0.f;
    for (int c = lane; c < a.C; c += 64) {
      if (c == y) continue;
      const float z = row[c], t = z * inv_t;
      if (t > m) {
        const float sc = expf(m - t);   // (e^-inf = 0 on the first class)
        se = fmaf(se, sc, 1.f);
        sez = fmaf(sez, sc, z - zy);
        m = t;
      } else {
        const float e = expf(t - m);
        se += e;
        sez = fmaf(e, z - zy, sez);
      }
    }
    const float mx = wave_max(m);   // (-inf when the label's class is the only one)
    const float f = m == -INFINITY ? 0.f : expf(m - mx);
    se = wave_sum(se * f);
    sez = wave_sum(sez * f);
    if (mx == -INFINITY) {
      loss += ok ? 0.f : NAN;
      dnum += ok ? 0.f : NAN;
    } else if (ty >= mx) {
      const float r = expf(mx - ty);            // the other classes' mass relative to the label's
      loss += log1pf(se * r);
      dnum -= sez * r / fmaf(se, r, 1.f);
    } else {
      const float ey = expf(ty - mx);           // (NaN for a label out of range: both sums NaN)
      loss += (mx - ty) + logf(se + ey);
      dnum -= sez / (se + ey);
    }
  }
  if (lane == 0) {
    red[2 * w] = loss;
    red[2 * w + 1] = dnum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.part[2 * blockIdx.x] = (red[0] + red[2]) + (red[4] + red[6]);
    a.part[2 * blockIdx.x + 1] = (red[1] + red[3]) + (red[5] + red[7]);
  }
}

// loss = sum(part[., 0]) / n, dT = sum(part[., 1]) / (n T^2): one workgroup, fixed order
__global__ __launch_bounds__(NT) void temperature_nll_finish(const float* part, int nblocks, int64_t n,
                                                             const float* temp, float* loss_out, float* dtemp_out) {
  __shared__ float red[2 * ROWS_PER_BLOCK];
  float l = 0.f, d = 0.f;
  for (int i = threadIdx.x; i < nblocks; i += NT) {
    l += part[2 * i];
    d += part[2 * i + 1];
  }
  l = wave_sum(l);
  d = wave_sum(d);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[2 * w] = l;
    red[2 * w + 1] = d;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = temp[0];
    const float inv_n = 1.f / (float)n;
    if (loss_out) loss_out[0] = ((red[0] + red[2]) + (red[4] + red[6])) * inv_n;
    if (dtemp_out) dtemp_out[0] = ((red[1] + red[3]) + (red[5] + red[7])) * inv_n / (t * t);
  }
}

inline int nll_blocks(int64_t n) {
  const int64_t nb = (n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  return (int)(nb < NLL_MAX_BLOCKS ? nb : NLL_MAX_BLOCKS);
}

struct UfArgs {
  int B, M, C;
  float eps;
  const float* logits;   // (B, M, C)
  const float* u;        // (B, M)
  const float* mask;     // (B, M)
  float* fused;          // (B, C)
  float* weights;        // (B, M)
  // backward
  const float* dfused;   // (B, C)
  float* dlogits;        // (B, M, C) or null
  float* du;             // (B, M) or null
};

// fw[m] of sample b into LDS (thread 0); returns through *inv: true when the inverse-uncertainty
// branch was taken (sum of the weighted terms > 0), false on the fallback
__device__ __forceinline__ void uf_weights(const UfArgs& a, int b, float* fw, float* wsum, int* inv) {
  if (threadIdx.x == 0) {
    float sw = 0.f, sm = 0.f;
    for (int m = 0; m < a.M; ++m) {
      const float mk = a.mask[(int64_t)b * a.M + m];
      const float wt = (1.f / (a.u[(int64_t)b * a.M + m] + a.eps)) * mk;
      fw[m] = wt;
      sw += wt;
      sm += mk;
    }
    const bool take = sw > 0.f;
    for (int m = 0; m < a.M; ++m) {
      const float mk = a.mask[(int64_t)b * a.M + m];
      const float fb = sm > 0.f ? mk / (sm + 1e-8f) : 1.f / (float)a.M;
      fw[m] = take ? fw[m] / (sw + 1e-8f) : fb;
    }
    *wsum = sw;
    *inv = take ? 1 : 0;
  }
}

__global__ __launch_bounds__(NT) void uncertainty_fusion_fwd(UfArgs a) {
  __shared__ float fw[UF_MAX_M];
  __shared__ float wsum;
  __shared__ int inv;
  const int b = blockIdx.x;
  uf_weights(a, b, fw, &wsum, &inv);
  __syncthreads();
  if (threadIdx.x < a.M) a.weights[(int64_t)b * a.M + threadIdx.x] = fw[threadIdx.x];
  for (int c = threadIdx.x; c < a.C; c += NT) {
    float acc = 0.f;
    for (int m = 0; m < a.M; ++m) acc = fmaf(a.logits[((int64_t)b * a.M + m) * a.C + c], fw[m], acc);
    a.fused[(int64_t)b * a.C + c] = acc;
  }
}

__global__ __launch_bounds__(NT) void uncertainty_fusion_bwd(UfArgs a) {
  __shared__ float fw[UF_MAX_M];
  __shared__ float dfw[UF_MAX_M];
  __shared__ float red[ROWS_PER_BLOCK];
  __shared__ float wsum;
  __shared__ int inv;
  const int b = blockIdx.x;
  uf_weights(a, b, fw, &wsum, &inv);
  __syncthreads();
  const float* gf = a.dfused + (int64_t)b * a.C;
  for (int m = 0; m < a.M; ++m) {
    float acc = 0.f;
    for (int c = threadIdx.x; c < a.C; c += NT) {
      const int64_t o = ((int64_t)b * a.M + m) * a.C + c;
      if (a.dlogits) a.dlogits[o] = gf[c] * fw[m];
      acc = fmaf(gf[c], a.logits[o], acc);
    }
    acc = wave_sum(acc);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) dfw[m] = (red[0] + red[1]) + (red[2] + red[3]);
  }
  __syncthreads();
  if (a.du && threadIdx.x == 0) {
    // fw = wt / (s + 1e-8), wt_j = mask_j r_j, r_j = 1 / (u_j + eps):
    // d wt_j = dfw_j / se - sum_m dfw_m wt_m / se^2, du_j = -d wt_j mask_j r_j^2; the fallback
    // branch does not depend on u
    const float se = wsum + 1e-8f;
    float dot = 0.f;
    for (int m = 0; m < a.M; ++m) dot = fmaf(dfw[m], fw[m], dot);   // sum_m dfw_m wt_m / se
    for (int m = 0; m < a.M; ++m) {
      float g = 0.f;
      if (inv) {
        const float mk = a.mask[(int64_t)b * a.M + m];
        const float r = 1.f / (a.u[(int64_t)b * a.M + m] + a.eps);
        g = -((dfw[m] - dot) / se) * mk * r * r;
      }
      a.du[(int64_t)b * a.M + m] = g;
    }
  }
}

int check_uf(int32_t batch, int32_t M, int32_t C) {
  if (batch < 0 || M < 1 || C < 1) return fail(MMF_EINVAL, "uncertainty fusion: bad shape");
  if (M > UF_MAX_M) return fail(MMF_ELIMIT, "uncertainty fusion: more than %d modalities", UF_MAX_M);
  return MMF_OK;
}

}  // namespace

}  // namespace mmf

using namespace mmf;

extern "C" {

int mmf_mc_reduce(int32_t samples, int32_t batch, int32_t classes, const float* logits_stack, float* mean_logits,
                  float* mean_probs, float* variance, void* stream) {
  int rc = check_mc(samples, batch, classes);
  if (rc) return rc;
  if (batch == 0) return MMF_OK;
  if (!logits_stack) return fail(MMF_EINVAL, "mc_reduce: null logits_stack");
  hipStream_t st = (hipStream_t)stream;
  McArgs a{samples, batch, classes, logits_stack, mean_logits, mean_probs, variance};
  HIP_TRY(launch_mc_reduce(a, st));
  return MMF_OK;
}

int mmf_hybrid_mc_forward(const mmf_hybrid_desc* d, const mmf_hybrid_params* params, const float* const* x,
                          const float* mask, uint64_t* rng_state, int32_t samples, void* saved,
                          float* logits_stack, float* fusion_weights, float* mean_logits, float* mean_probs,
                          float* variance, void* stream) {
  if (!d) return fail(MMF_EINVAL, "null descriptor");
  if (samples < 1) return fail(MMF_EINVAL, "hybrid_mc_forward: samples must be >= 1, got %d", samples);
  if (d->training != 1) return fail(MMF_EINVAL, "hybrid_mc_forward: MC dropout needs a training descriptor");
  if (d->return_attention != 0) return fail(MMF_EINVAL, "hybrid_mc_forward: return_attention is not supported");
  int rc = check_mc(samples, d->batch, d->num_classes);
  if (rc) return rc;
  if (!logits_stack) return fail(MMF_EINVAL, "null argument");
  hipStream_t st = (hipStream_t)stream;
  const int64_t slot = (int64_t)d->batch * d->num_classes;
  {
    // (the descriptor, the buffer contract and the remaining arguments are checked by the first
    // forward before its first launch)
    Stage stage_("mc.forward", st);
    for (int32_t s = 0; s < samples; ++s) {
      rc = mmf_hybrid_forward(d, params, x, mask, rng_state, saved, logits_stack + s * slot, fusion_weights,
                              nullptr, stream);
      if (rc) return rc;
    }
  }
  if (d->batch == 0) return MMF_OK;
  McArgs a{samples, d->batch, d->num_classes, logits_stack, mean_logits, mean_probs, variance};
  STAGE_TRY("mc.reduce", launch_mc_reduce(a, st));
  return MMF_OK;
}

size_t mmf_temperature_nll_workspace_bytes(int64_t n) {
  return (size_t)(n > 0 ? nll_blocks(n) : 1) * 2 * sizeof(float) + 256;
}

int mmf_temperature_nll(int64_t n, int32_t classes, const float* logits, const int64_t* labels,
                        const float* temperature_dev, float* loss_out, float* dtemp_out, void* workspace,
                        void* stream) {
  if (n < 1 || classes < 1) return fail(MMF_EINVAL, "temperature_nll: bad shape");
  if (classes > MAX_CLASSES) return fail(MMF_ELIMIT, "temperature_nll: %d classes > %d", classes, MAX_CLASSES);
  if (!logits || !labels || !temperature_dev || !workspace) return fail(MMF_EINVAL, "temperature_nll: null argument");
  hipStream_t st = (hipStream_t)stream;
  const int nb = nll_blocks(n);
  NllArgs a{n, classes, logits, labels, temperature_dev, (float*)workspace};
  {
    ProfLaunch prof_(st, "temperature_nll_kernel", 8.0 * n * classes, 4.0 * n * classes + 8.0 * n);
    mmf_launch(temperature_nll_kernel, dim3(nb), dim3(NT), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  ProfLaunch prof_(st, "temperature_nll_finish", 2.0 * nb, 8.0 * nb);
  mmf_launch(temperature_nll_finish, dim3(1), dim3(NT), 0, st, (const float*)a.part, nb, n, temperature_dev,
             loss_out, dtemp_out);
  HIP_TRY(hipGetLastError());
  return MMF_OK;
}

int mmf_uncertainty_fusion_forward(int32_t batch, int32_t num_modalities, int32_t num_classes, const float* logits,
                                   const float* uncertainty, const float* mask, float epsilon, float* fused,
                                   float* weights, void* stream) {
  int rc = check_uf(batch, num_modalities, num_classes);
  if (rc) return rc;
  if (batch == 0) return MMF_OK;
  if (!logits || !uncertainty || !mask || !fused || !weights)
    return fail(MMF_EINVAL, "uncertainty fusion: null argument");
  hipStream_t st = (hipStream_t)stream;
  UfArgs a;
  memset(&a, 0, sizeof(a));
  a.B = batch; a.M = num_modalities; a.C = num_classes; a.eps = epsilon;
  a.logits = logits; a.u = uncertainty; a.mask = mask; a.fused = fused; a.weights = weights;
  ProfLaunch prof_(st, "uncertainty_fusion_fwd", 2.0 * batch * num_modalities * num_classes,
                   4.0 * batch * num_modalities * (num_classes + 3));
  mmf_launch(uncertainty_fusion_fwd, dim3(batch), dim3(NT), 0, st, a);
  HIP_TRY(hipGetLastError());
  return MMF_OK;
}

int mmf_uncertainty_fusion_backward(int32_t batch, int32_t num_modalities, int32_t num_classes, const float* logits,
                                    const float* uncertainty, const float* mask, float epsilon, const float* dfused,
                                    float* dlogits, float* duncertainty, void* stream) {
  int rc = check_uf(batch, num_modalities, num_classes);
  if (rc) return rc;
  if (batch == 0 || (!dlogits && !duncertainty)) return MMF_OK;
  if (!logits || !uncertainty || !mask || !dfused) return fail(MMF_EINVAL, "uncertainty fusion: null argument");
  hipStream_t st = (hipStream_t)stream;
  UfArgs a;
  memset(&a, 0, sizeof(a));
  a.B = batch; a.M = num_modalities; a.C = num_classes; a.eps = epsilon;
  a.logits = logits; a.u = uncertainty; a.mask = mask; a.dfused = dfused; a.dlogits = dlogits; a.du = duncertainty;
  ProfLaunch prof_(st, "uncertainty_fusion_bwd", 4.0 * batch * num_modalities * num_classes,
                   4.0 * batch * num_modalities * (2 * num_classes + 3));
  mmf_launch(uncertainty_fusion_bwd, dim3(batch), dim3(NT), 0, st, a);
  HIP_TRY(hipGetLastError());
  return MMF_OK;
}

}  // extern "C"
