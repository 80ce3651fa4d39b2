// Standard evaluation (src/eval.py:39-130 evaluate_model, src/uncertainty.py:84-192
// CalibrationMetrics): one batch of logits and labels into every statistic the metrics need, on the
// device, into a state that is read back once after the last batch.
//
//  * eval_rows_kernel: one wave per row.  z = logit / T; argmax with confusion_kernel's rule
//    (lowest index among equal maxima, a NaN counts as the maximum); s = sum exp(z - max z) over
//    the lanes' strided partial sums, combined by an xor butterfly (every lane ends with the same
//    bits); confidence = 1 / s with the correctly rounded division; cross-entropy = max z + log s -
//    z[label]; the bin by the float32 edges.  It writes the row's prediction and confidence where
//    asked, the row's record {cross-entropy, confidence, code} into the workspace, and adds 1 to
//    confusion[label, pred] (a 64-bit integer atomic: the order cannot change the result).  A label
//    outside [0, C) is never used as an index: the row's record says "bad label" and nothing else.
//
//  * eval_reduce_kernel: workgroup b < bins folds the records of bin b (count, correct count, sum
//    of confidences), workgroup `bins` the batch's totals (samples, correct, bad labels, NaN rows,
//    sum of cross-entropies).  Each thread takes the rows t, t + 256, ... in order into a float64 /
//    int64 partial, the partials are combined by a fixed butterfly and then wave by wave, and the
//    workgroup adds the result to the state words it alone owns: no float atomics, no
//    inter-workgroup waits, and a rerun leaves the same bytes.
#include <cmath>

#include "capi_util.h"

namespace mmf {

namespace {

constexpr int NT = 256;
constexpr int EVAL_MAX_CLASSES = 1024, EVAL_MAX_BINS = 256, EVAL_MAX_BATCH = 1 << 24;
constexpr int HEAD_WORDS = 8;   // include/mmfusion.h: the state's first 8 words

// a row's code: bits 0..8 = bin + 1 (0: in no bin), then the flags
constexpr int CODE_BIN_MASK = 0x1ff, CODE_CORRECT = 1 << 9, CODE_VALID = 1 << 10, CODE_NAN = 1 << 11;

struct EvalRowsArgs {
  int32_t B, C, bins;
  const float* logits;      // (B, C)
  const int64_t* labels;    // (B)
  const float* edges;       // (bins + 1)
  const float* temperature; // device scalar or null
  int64_t* confusion;       // (C, C) inside the state
  int64_t* preds_out;       // (B) or null
  float* conf_out;          // (B) or null
  float* row_ce;            // (B) workspace
  float* row_conf;          // (B) workspace
  int32_t* row_code;        // (B) workspace
};

struct EvalReduceArgs {
  int32_t B, C, bins;
  const float* row_ce;
  const float* row_conf;
  const int32_t* row_code;
  int64_t* state;
};

// (v1, i1) beats (v2, i2) under torch.argmax's order
__device__ __forceinline__ bool arg_better(float v1, int i1, float v2, int i2) {
  const bool n1 = v1 != v1, n2 = v2 != v2;
  if (n1 != n2) return n1;
  if (n1 || v1 == v2) return i1 < i2;
  return v1 > v2;
}

__global__ __launch_bounds__(NT) void eval_rows_kernel(EvalRowsArgs a) {
  const int lane = threadIdx.x & 63;
  const int r = (int)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (r >= a.B) return;   // (whole waves leave; no barrier below)
  const float* row = a.logits + (int64_t)r * a.C;
  const bool scaled = a.temperature != nullptr;
  const float T = scaled ? a.temperature[0] : 1.f;

  float bv = -INFINITY;
  int bi = 0x7fffffff;   // (no class yet: any real class wins the index tie)
  for (int c = lane; c < a.C; c += 64) {
    const float v = scaled ? __fdiv_rn(row[c], T) : row[c];
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
  // every lane now holds the row's (max, argmax).  A NaN maximum, +inf (inf - inf) and an all -inf
  // row (-inf + inf) make the sum NaN below, as they make torch's softmax NaN.
  float s = 0.f;
  for (int c = lane; c < a.C; c += 64) {
    const float v = scaled ? __fdiv_rn(row[c], T) : row[c];
    s += expf(v - bv);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);   // (a + b == b + a: the same bits in every lane)
  const float conf = __fdiv_rn(1.f, s);

  // the bin: edges[b] <= conf < edges[b + 1], the last bin closed; the edges rise, so at most one matches
  int bin1 = 0;
  for (int b = lane; b < a.bins; b += 64) {
    const float lo = a.edges[b], hi = a.edges[b + 1];
    if (conf >= lo && (conf < hi || (b == a.bins - 1 && conf <= hi))) bin1 = b + 1;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int ob = __shfl_xor(bin1, o);
    bin1 = ob > bin1 ? ob : bin1;
  }

  if (lane == 0) {
    if (a.preds_out) a.preds_out[r] = bi;
    if (a.conf_out) a.conf_out[r] = conf;
    const int64_t y = a.labels[r];
    float ce = 0.f;
    int code = 0;
    if (y >= 0 && y < a.C) {
      const float zy = scaled ? __fdiv_rn(row[y], T) : row[y];
      ce = (bv + logf(s)) - zy;
      code = bin1 | CODE_VALID | (bi == (int)y ? CODE_CORRECT : 0) | (conf != conf ? CODE_NAN : 0);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.confusion + y * a.C + bi), 1ull);
    }
    a.row_ce[r] = ce;
    a.row_conf[r] = conf;
    a.row_code[r] = code;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// grid bins + 1
__global__ __launch_bounds__(NT) void eval_reduce_kernel(EvalReduceArgs a) {
  __shared__ double fs[NT / 64];
  __shared__ long long is[4][NT / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int job = blockIdx.x;
  double f = 0.0;
  long long n0 = 0, n1 = 0, n2 = 0, n3 = 0;
  if (job < a.bins) {   // bin `job`: count, correct count, sum of confidences
    for (int r = t; r < a.B; r += NT) {
      const int code = a.row_code[r];
      if ((code & CODE_BIN_MASK) == job + 1) {
        n0 += 1;
        n1 += (code & CODE_CORRECT) ? 1 : 0;
        f += (double)a.row_conf[r];
      }
    }
  } else {   // the batch: samples, correct, bad labels, NaN rows, sum of cross-entropies
    for (int r = t; r < a.B; r += NT) {
      const int code = a.row_code[r];
      if (code & CODE_VALID) {
        n0 += 1;
        n1 += (code & CODE_CORRECT) ? 1 : 0;
        n3 += (code & CODE_NAN) ? 1 : 0;
        f += (double)a.row_ce[r];
      } else {
        n2 += 1;
      }
    }
  }
  f = wave_sum(f);
  n0 = wave_sum(n0);
  n1 = wave_sum(n1);
  n2 = wave_sum(n2);
  n3 = wave_sum(n3);
  if (lane == 0) {
    fs[w] = f;
    is[0][w] = n0;
    is[1][w] = n1;
    is[2][w] = n2;
    is[3][w] = n3;
  }
  __syncthreads();
  if (t != 0) return;
  double ft = 0.0;
  long long nt[4] = {0, 0, 0, 0};
  for (int i = 0; i < NT / 64; ++i) {   // the waves in index order
    ft += fs[i];
    for (int k = 0; k < 4; ++k) nt[k] += is[k][i];
  }
  int64_t* st = a.state;
  double* sd = reinterpret_cast<double*>(a.state);
  if (job < a.bins) {
    int64_t* bin = st + HEAD_WORDS + (int64_t)a.C * a.C;
    bin[job] += nt[0];
    bin[a.bins + job] += nt[1];
    reinterpret_cast<double*>(bin)[2 * a.bins + job] += ft;
  } else {
    st[0] += nt[0];
    st[1] += nt[1];
    st[2] += nt[2];
    st[3] += 1;
    st[4] += nt[3];
    sd[5] += ft / (double)a.B;   // the call's mean cross-entropy (F.cross_entropy's default reduction)
    sd[6] += ft;
  }
}

bool eval_shape_ok(int32_t batch, int32_t classes, int32_t bins) {
  return classes >= 1 && classes <= EVAL_MAX_CLASSES && bins >= 1 && bins <= EVAL_MAX_BINS && batch >= 0 &&
         batch <= EVAL_MAX_BATCH;
}

size_t round256(size_t n) { return (n + 255) & ~size_t(255); }

}  // namespace

}  // namespace mmf

using namespace mmf;

extern "C" {

size_t mmf_eval_state_bytes(int32_t classes, int32_t bins) {
  if (!eval_shape_ok(0, classes, bins)) {
    fail(MMF_ELIMIT, "eval_state_bytes: classes %d outside 1..%d or bins %d outside 1..%d", classes, EVAL_MAX_CLASSES,
         bins, EVAL_MAX_BINS);
    return 0;
  }
  return 8 * ((size_t)HEAD_WORDS + (size_t)classes * classes + 3 * (size_t)bins);
}

size_t mmf_eval_workspace_bytes(int32_t batch, int32_t classes, int32_t bins) {
  if (!eval_shape_ok(batch, classes, bins)) {
    fail(MMF_ELIMIT, "eval_workspace_bytes: batch %d, classes %d, bins %d outside the limits (2^24, %d, %d)", batch,
         classes, bins, EVAL_MAX_CLASSES, EVAL_MAX_BINS);
    return 0;
  }
  return 3 * round256(4 * (size_t)batch) + 256;
}

int mmf_eval_accumulate(int32_t batch, int32_t classes, int32_t bins, const float* logits, const int64_t* labels,
                        const float* edges, const float* temperature, void* state, int64_t* preds_out,
                        float* conf_out, void* workspace, void* stream) {
  if (!eval_shape_ok(batch, classes, bins))
    return fail(MMF_ELIMIT, "eval_accumulate: batch %d, classes %d, bins %d outside the limits (2^24, %d, %d)", batch,
                classes, bins, EVAL_MAX_CLASSES, EVAL_MAX_BINS);
  if (batch == 0) return MMF_OK;   // an empty batch: nothing to do (it is no call of the loss either)
  if (!logits || !labels || !edges || !state || !workspace) return fail(MMF_EINVAL, "eval_accumulate: null argument");
  hipStream_t st = (hipStream_t)stream;
  Bump ws(workspace);
  float* row_ce = ws.take<float>(batch);
  float* row_conf = ws.take<float>(batch);
  int32_t* row_code = ws.take<int32_t>(batch);
  int64_t* words = (int64_t*)state;
  EvalRowsArgs ra{batch, classes, bins, logits, labels, edges, temperature, words + HEAD_WORDS, preds_out, conf_out,
                  row_ce, row_conf, row_code};
  {
    ProfLaunch prof_(st, "eval_rows_kernel", 4.0 * batch * classes, 4.0 * batch * classes + 36.0 * batch);
    mmf_launch(eval_rows_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(NT), 0, st, ra);
    HIP_TRY(hipGetLastError());
  }
  EvalReduceArgs rr{batch, classes, bins, row_ce, row_conf, row_code, words};
  {
    ProfLaunch prof_(st, "eval_reduce_kernel", (double)batch * (bins + 1), 8.0 * batch * (bins + 1));
    mmf_launch(eval_reduce_kernel, dim3((unsigned)(bins + 1)), dim3(NT), 0, st, rr);
    HIP_TRY(hipGetLastError());
  }
  return MMF_OK;
}

}  // extern "C"
