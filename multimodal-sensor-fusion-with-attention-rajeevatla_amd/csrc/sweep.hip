// Missing-modality robustness sweep (src/eval.py:312-458 evaluate_missing_modalities) kernels:
//
//  * sweep_prep_kernel: the all-present mask (B, M) the shared pass runs under, the patterns' bit
//    sets (host data, carried as kernel arguments) into the workspace, and one flag per (sample,
//    modality): the input holds a NaN.  The forward's ReLU kernels return 0 for a NaN
//    pre-activation, so the shared pass alone would turn a NaN input into finite logits; the tail
//    gives the rows whose pattern includes such a modality NaN logits, as the reference does.
//
//  * sweep_pool_kernel: the L-mean of a (B, L, H) activation of the shared pass, for the sources the
//    selected plan leaves unpooled (P_m of a sequence modality; the general plan's attended rows).
//    Four row lanes per column, combined in a fixed order.
//
//  * sweep_tail_kernel: one workgroup per tile of 32 (pattern, sample) rows.
//      1. every wave builds 8 rows' fused vectors in LDS: the aggregate of each present query by
//         selection (an absent modality's Pbar / Abar are never read; an absent key contributes the
//         pair's out_proj.bias), gating scores, the masked softmax with the reference's fallback
//         (src/fusion.py:462-478), the weighted sum;
//      2. classifier layer 1 on v_mfma_f32_32x32x2_f32: the tile's 32 rows against 32-column blocks
//         of W1, W1 streamed through LDS in 32-wide k chunks;
//      3. ReLU into LDS, then layer 2 as fp32 dot products in a fixed order (C is small);
//      4. logits (S, B, C) and, when asked, the fusion weights (S, B, M).
//    fp32 at every matmul-precision setting; no atomics: reruns are bit-identical.
//
//  * confusion_kernel: one wave per (stack, sample) row: argmax with torch.argmax's rule (lowest
//    index among equal maxima, NaN counts as the maximum), counts[s, label, pred] += 1 (64-bit
//    integer atomics: the order cannot change the result); a label outside [0, C) is never used as
//    an index and bumps bad_labels.
#include <cmath>

#include "capi_util.h"
#include "mmf_device.h"

namespace mmf {

namespace {

constexpr int NT = 256;
constexpr int TR = 32;    // (pattern, sample) rows per tail tile: one MFMA row block
constexpr int KC = 32;    // k chunk of W1 staged in LDS
constexpr int LDW = KC + 1;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// blocks [0, B M): does sample b's input of modality m hold a NaN; the blocks after them: the
// all-present mask and the pattern words
__global__ __launch_bounds__(NT) void sweep_prep_kernel(SweepPrepArgs a) {
  const int nscan = a.B * a.M;
  if ((int)blockIdx.x < nscan) {
    const int b = blockIdx.x / a.M, m = blockIdx.x % a.M;
    const int64_t n = a.xn[m];
    const float* p = a.x[m] + (int64_t)b * n;
    int bad = 0;
    for (int64_t i = threadIdx.x; i < n; i += NT) bad |= p[i] != p[i];
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) a.nan_out[blockIdx.x] = bad ? 1u : 0u;
    return;
  }
  const int i = ((int)blockIdx.x - nscan) * NT + threadIdx.x;
  if (i < a.n_ones) a.ones[i] = 1.f;
  if (i < a.n_words) a.bits_out[i] = a.words[i];
}

__global__ __launch_bounds__(NT) void sweep_pool_kernel(SweepPoolArgs a) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = blockIdx.y * 64 + lane, b = blockIdx.x, si = blockIdx.z;   // (the batch on grid.x: no 65 535 cap)
  const int L = a.L[si], H = a.H;
  float acc = 0.f;
  if (col < H) {
    const float* p = a.src[si] + (int64_t)b * L * H + col;
    for (int r = rl; r < L; r += 4) acc += p[(int64_t)r * H];
  }
  red[rl][lane] = acc;
  __syncthreads();
  if (rl == 0 && col < H)
    a.dst[si][(int64_t)b * H + col] = ((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])) * a.scale[si];
}

// NC = columns per lane of the row phase (H <= 64 NC); the tile's H is padded to HP = 32-multiples
template <int NC>
__global__ __launch_bounds__(NT) void sweep_tail_kernel(SweepTailArgs a) {
  constexpr int HMAX = 64 * NC;
  constexpr int LDF = HMAX + 1;
  constexpr int NBW = NC >= 2 ? NC / 2 : 1;   // 32-column blocks of the hidden layer per wave
  __shared__ float Fs[TR * LDF];              // fused rows, then the hidden layer
  __shared__ float Wt[HMAX * LDW];            // W1[:, k0 : k0 + KC]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int M = a.M, H = a.H, C = a.C, B = a.B;
  const int64_t R = (int64_t)a.S * B;
  const int64_t row0 = (int64_t)blockIdx.x * TR;
  const int HP = (H + 31) & ~31;

  // ---- 1. fused rows
  for (int rr = 0; rr < TR / 4; ++rr) {
    const int lr = w * (TR / 4) + rr;
    const int64_t r = row0 + lr;
    float fused[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) fused[j] = 0.f;
    if (r < R) {   // (wave-uniform)
      const int s = (int)(r / B), b = (int)(r % B);
      const uint32_t bits = a.bits[s];
      float agg[8][NC], score[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        score[q] = 0.f;
#pragma unroll
        for (int j = 0; j < NC; ++j) agg[q][j] = 0.f;
        if (q < M && ((bits >> q) & 1u)) {
          float dot = 0.f;
#pragma unroll
          for (int j = 0; j < NC; ++j) {
            const int col = lane + 64 * j;
            if (col < H) {
              float v = a.Pbar[q][(int64_t)b * H + col];
              for (int g = 0; g < a.npairs; ++g) {
                if (a.pq[g] != q) continue;
                v += ((bits >> a.pk[g]) & 1u) ? a.Abar[g][(int64_t)b * H + col] : a.bo[g][col];
              }
              v *= a.inv_cnt[q];
              agg[q][j] = v;
              dot = fmaf(v, a.gate_w[q][col], dot);
            }
          }
          score[q] = wave_sum(dot) + a.gate_b[q][0];
        }
      }
      // masked softmax over the present modalities, renormalisation / fallback (src/fusion.py:462-478)
      float mx = -INFINITY;
      int cnt = 0;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (q < M && ((bits >> q) & 1u)) {
          mx = fmaxf(mx, score[q]);
          ++cnt;
        }
      float wq[8], z = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        wq[q] = (q < M && ((bits >> q) & 1u)) ? __expf(score[q] - mx) : 0.f;
        z += wq[q];
      }
      float sw = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        wq[q] = (mx == -INFINITY) ? 0.f : wq[q] / z;   // nan_to_num of an all -inf row
        sw += wq[q];
      }
      const bool take = sw > 0.f;   // (false for a NaN score: the reference's nan_to_num, then its fallback)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const bool present = q < M && ((bits >> q) & 1u);
        const float fb = cnt > 0 ? (present ? 1.f / ((float)cnt + 1e-8f) : 0.f) : 1.f / (float)M;
        wq[q] = take ? wq[q] / (sw + 1e-8f) : fb;
        if (present) {
#pragma unroll
          for (int j = 0; j < NC; ++j) fused[j] = fmaf(wq[q], agg[q][j], fused[j]);
        }
        if (a.weights && lane == q && q < M) a.weights[r * M + q] = wq[q];
      }
      // a NaN in the input of a PRESENT modality: NaN logits, as the reference gives (the shared
      // pass's ReLUs returned 0 for it); an absent modality's flag is not read
      bool poisoned = false;
      for (int q = 0; q < M; ++q)
        if (((bits >> q) & 1u) && a.nan_in[(int64_t)b * M + q]) poisoned = true;
      if (poisoned) {
#pragma unroll
        for (int j = 0; j < NC; ++j) fused[j] = NAN;
      }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) Fs[lr * LDF + lane + 64 * j] = fused[j];
  }

  // ---- 2. hidden = fused W1^T on the matrix cores, W1 streamed through LDS
  f32x16 acc[NBW];
#pragma unroll
  for (int i = 0; i < NBW; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  const int mi = lane & 31, half = lane >> 5;
  for (int k0 = 0; k0 < HP; k0 += KC) {
    __syncthreads();   // (first pass: the fused rows are complete; later: the last chunk is consumed)
    for (int idx = t; idx < HP * (KC / 4); idx += NT) {
      const int n = idx / (KC / 4), kq = idx % (KC / 4);
      const int k = k0 + 4 * kq;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n < H && k < H) {   // (H % 4 == 0: the four never straddle the row's end; W1 need not be 16-byte aligned)
        const float* p = a.W1 + (int64_t)n * H + k;
        v = make_float4(p[0], p[1], p[2], p[3]);
      }
      float* o = Wt + n * LDW + 4 * kq;
      o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < KC; kk += 2) {
      const float av = Fs[mi * LDF + k0 + kk + half];
#pragma unroll
      for (int i = 0; i < NBW; ++i) {
        const int n0 = (w + 4 * i) * 32;
        if (n0 < HP) acc[i] = mfma32(av, Wt[(n0 + mi) * LDW + kk + half], acc[i]);   // (wave-uniform)
      }
    }
  }
  __syncthreads();   // every wave has read the fused rows: the hidden layer takes their place
  // ---- 3. ReLU(. + b1) into LDS
#pragma unroll
  for (int i = 0; i < NBW; ++i) {
    const int n = (w + 4 * i) * 32 + mi;
    if ((w + 4 * i) * 32 < HP) {
      const float bias = n < H ? a.b1[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float z = acc[i][r] + bias;
        Fs[acc_row(r, half) * LDF + n] = n < H ? (z < 0.f ? 0.f : z) : 0.f;   // (torch.relu: a NaN stays)
      }
    }
  }
  __syncthreads();
  // ---- 4. logits = hidden W2^T + b2 (32 rows x C outputs; the 32 lanes of one class share W2's row)
  for (int idx = t; idx < TR * C; idx += NT) {
    const int lr = idx & (TR - 1), c = idx / TR;
    const int64_t r = row0 + lr;
    if (r >= R) continue;
    const float* w2 = a.W2 + (int64_t)c * H;
    const float* h = Fs + lr * LDF;
    float s = 0.f;
    for (int k = 0; k < H; ++k) s = fmaf(h[k], w2[k], s);
    a.logits[r * C + c] = s + a.b2[c];
  }
}

struct ConfArgs {
  int32_t S, B, C;
  const float* logits;     // (S, B, C)
  const int64_t* labels;   // (B)
  int64_t* counts;         // (S, C, C)
  int64_t* bad;            // (1)
};

// (v1, i1) beats (v2, i2) under torch.argmax's order
__device__ __forceinline__ bool arg_better(float v1, int i1, float v2, int i2) {
  const bool n1 = v1 != v1, n2 = v2 != v2;
  if (n1 != n2) return n1;
  if (n1 || v1 == v2) return i1 < i2;
  return v1 > v2;
}

__global__ __launch_bounds__(NT) void confusion_kernel(ConfArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (r >= (int64_t)a.S * a.B) return;   // (whole waves leave; no barrier below)
  const int s = (int)(r / a.B), b = (int)(r % a.B);
  const float* row = a.logits + r * a.C;
  float bv = -INFINITY;
  int bi = 0x7fffffff;   // (no class yet: any real class wins the index tie)
  for (int c = lane; c < a.C; c += 64) {
    const float v = row[c];
    if (arg_better(v, c, bv, bi)) {
      bv = v;
      bi = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (arg_better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    const int64_t y = a.labels[b];
    if (y >= 0 && y < a.C)
      atomicAdd(reinterpret_cast<unsigned long long*>(a.counts + ((int64_t)s * a.C + y) * a.C + bi), 1ull);
    else
      atomicAdd(reinterpret_cast<unsigned long long*>(a.bad), 1ull);
  }
}

}  // namespace

hipError_t launch_sweep_prep(const SweepPrepArgs& a, hipStream_t st) {
  const int n = a.n_ones > a.n_words ? a.n_ones : a.n_words;
  double xbytes = 0;
  for (int m = 0; m < a.M; ++m) xbytes += 4.0 * a.B * a.xn[m];
  ProfLaunch prof_(st, "sweep_prep_kernel", 0.0, xbytes + 4.0 * (a.n_ones + a.n_words));
  mmf_launch(sweep_prep_kernel, dim3(a.B * a.M + (n + NT - 1) / NT), dim3(NT), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_sweep_pool(const SweepPoolArgs& a, hipStream_t st) {
  if (a.nsrc == 0) return hipSuccess;
  double rows = 0;
  for (int i = 0; i < a.nsrc; ++i) rows += a.L[i] + 1;
  ProfLaunch prof_(st, "sweep_pool_kernel", rows * a.B * a.H, 4.0 * rows * a.B * a.H);
  mmf_launch(sweep_pool_kernel, dim3(a.B, (a.H + 63) / 64, a.nsrc), dim3(NT), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_sweep_tail(const SweepTailArgs& a, hipStream_t st) {
  const int64_t R = (int64_t)a.S * a.B;
  const dim3 grid((unsigned)((R + TR - 1) / TR)), block(NT);
  ProfLaunch prof_(st, "sweep_tail_kernel", 2.0 * R * a.H * (a.H + a.C + 2.0 * a.M),
                   4.0 * (R * (a.C + a.M) + (double)a.B * a.H * (a.M + a.npairs) + (double)a.H * (a.H + a.C)));
  if (a.H <= 64) mmf_launch(sweep_tail_kernel<1>, grid, block, 0, st, a);
  else if (a.H <= 128) mmf_launch(sweep_tail_kernel<2>, grid, block, 0, st, a);
  else mmf_launch(sweep_tail_kernel<4>, grid, block, 0, st, a);
  return hipGetLastError();
}

}  // namespace mmf

using namespace mmf;

extern "C" {

int mmf_confusion_accumulate(int32_t stacks, int32_t batch, int32_t classes, const float* logits_stack,
                             const int64_t* labels, int64_t* counts, int64_t* bad_labels, void* stream) {
  if (stacks < 1 || batch < 0 || classes < 1)
    return fail(MMF_EINVAL, "confusion_accumulate: bad shape (stacks %d, batch %d, classes %d)", stacks, batch,
                classes);
  if (batch == 0) return MMF_OK;
  if (!logits_stack || !labels || !counts || !bad_labels) return fail(MMF_EINVAL, "confusion_accumulate: null argument");
  hipStream_t st = (hipStream_t)stream;
  const int64_t R = (int64_t)stacks * batch;
  if ((R + 3) / 4 > 0x7fffffff) return fail(MMF_ELIMIT, "confusion_accumulate: %lld rows", (long long)R);
  ConfArgs a{stacks, batch, classes, logits_stack, labels, counts, bad_labels};
  ProfLaunch prof_(st, "confusion_kernel", (double)R * classes, 4.0 * R * classes + 16.0 * R);
  mmf_launch(confusion_kernel, dim3((unsigned)((R + 3) / 4)), dim3(NT), 0, st, a);
  HIP_TRY(hipGetLastError());
  return MMF_OK;
}

}  // extern "C"
