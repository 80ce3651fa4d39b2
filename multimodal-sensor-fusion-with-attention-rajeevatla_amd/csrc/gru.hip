// Persistent GRU recurrence (SequenceEncoder 'gru', src/encoders.py:77-85, 135-166; PyTorch
// nn.GRU semantics, gate order r, z, n, zero initial state):
//   a_t = W_hh h_{t-1}             (xproj = x W_ih^T + b_ih + [b_hr, b_hz, 0], precomputed)
//   r = sigmoid(xproj_r + a_r);  z = sigmoid(xproj_z + a_z)
//   q = a_n + b_hn;  n = tanh(xproj_n + r q);  h_t = (1 - z) n + z h_{t-1}
// The LSTM's sibling (lstm.hip) on the same plan and the same exchange (recurrence.h): G = H / 64
// workgroups of 1024 threads per (GRU, <= 4 batch rows) instance keep their 64 units' 3 x 64 rows
// of W_hh in VGPRs (48 floats per thread at H = 256, loaded once) and exchange h_t every step
// through tagged granules, double-buffered by step parity; every spin is bounded, a wait that gives
// up sets the call's timeout word and poisons the missing values with NaN.  One barrier per step.
//
// The cell is not the LSTM's: three gate rows sit in the four-slot transpose-reduce (the fourth
// slot idle), and n needs r.  After the one cross-lane reduce every lane of a unit's 16-lane row
// takes r, z (row_newbcast of the sigmoids), a_n and xproj_n (row_newbcast of the reduce's output
// and of the input) and computes n itself: the dependent step costs one more activation in the
// chain and four DPP moves, no second barrier and no LDS round trip.  b_hn cannot be folded into
// xproj (it is multiplied by r), so it rides in a register.  The owner lane keeps h_{t-1} in a
// register (there is no cell state).  The backward's carry is d z + W_hh^T [dr, dz, dn r]: the
// owner keeps d z in a register and the workgroups exchange their partials of the matvec over
// 3 x 64 local rows.
#include "recurrence.h"

namespace mmf {

namespace {

struct GruArgs {
  int T, H, G, ninst;
  int8_t gru_of[LMAX_I];           // instance -> GRU
  int16_t b0[LMAX_I];              // instance -> first batch row
  int8_t nb[LMAX_I];               // instance -> batch rows (<= 4)
  const float* xproj[LMAX_N];      // (B, T, 3H)
  const float* w_hh[LMAX_N];       // (3H, H)
  const float* b_hn[LMAX_N];       // (H)
  float* h[LMAX_N];                // (B, T, H)
  float* gates[LMAX_N];            // (B, T, 4H): r, z, n, q = a_n + b_hn
  // backward
  const float* dh[LMAX_N];         // (B, T, H) upstream gradient of every h_t (may be null)
  float* dgates[LMAX_N];           // (B, T, 4H): dr_pre, dz_pre, dn_pre, dn_pre * r
  gu64* gran[LMAX_N];              // 2 x G x B x H granules (the forward uses 2 x B x H)
  unsigned* timeout;
};

constexpr int GROWS = 3 * LU;      // local rows of W_hh per workgroup
constexpr int GRP = GROWS / 16;    // rows per matvec lane of the backward (12)

// Backward: lane u of wave b polls the G partials of (W_hh^T dgh)[b][unit u] with independent
// loads and runs the cell backward directly; dg_s is double-buffered: one barrier per step.
__global__ __launch_bounds__(LNT) void gru_bwd_kernel(const GruArgs a) {
  __shared__ __attribute__((aligned(16))) float dg_s[2][LMAX_B][GROWS];
  const int inst = blockIdx.x / a.G, j = blockIdx.x - inst * a.G;
  if (inst >= a.ninst) return;
  const int li = a.gru_of[inst], b0 = a.b0[inst];
  const int t0 = threadIdx.x;
  const int H = a.H, B = a.nb[inst], G = a.G, H4X = 4 * H;
  const float* hin = a.h[li] + (int64_t)b0 * a.T * H;
  const float* gin = a.gates[li] + (int64_t)b0 * a.T * H4X;
  const float* dhin = a.dh[li] ? a.dh[li] + (int64_t)b0 * a.T * H : nullptr;
  float* dgout = a.dgates[li] + (int64_t)b0 * a.T * H4X;
  gu64* gr = a.gran[li] + (int64_t)2 * G * b0 * H;
  // matvec lanes: wave w, lane l -> local rows (l & 15) * 12 .. + 12 (row = gate * 64 + unit),
  // hidden columns kc .. kc + 3 with kc = 4 (4 w + (l >> 4)); the butterfly leaves column
  // kc + ((l >> 2) & 3) in lane l
  const int l = t0 & 63, rp = l & 15;
  const int kc = ((t0 >> 6) * 4 + (l >> 4)) * 4;
  const int k = kc + ((l >> 2) & 3);
  const bool kthread = kc < H;
  f2v w[4][GRP / 2];   // w[c][i / 2] = W_hh[grow(rp * 12 + i)][kc + c]
#pragma unroll
  for (int i = 0; i < GRP; i += 2) {
    float4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if (kthread) {
      const int r0 = rp * GRP + i, r1 = r0 + 1;
      v0 = *reinterpret_cast<const float4*>(a.w_hh[li] + (int64_t)((r0 >> 6) * H + j * LU + (r0 & 63)) * H + kc);
      v1 = *reinterpret_cast<const float4*>(a.w_hh[li] + (int64_t)((r1 >> 6) * H + j * LU + (r1 & 63)) * H + kc);
    }
    w[0][i / 2] = f2v{v0.x, v1.x};
    w[1][i / 2] = f2v{v0.y, v1.y};
    w[2][i / 2] = f2v{v0.z, v1.z};
    w[3][i / 2] = f2v{v0.w, v1.w};
  }
  const int ub = t0 / LU, lu = t0 - ub * LU;
  const bool unit_thread = ub < B;
  const int unit = j * LU + lu;
  float dz = 0.f;   // d_{t+1} z_{t+1}: the local term of the carry
  const int64_t par = (int64_t)G * B * H;
  for (int s = 0; s < a.T; ++s) {
    const int t = a.T - 1 - s;
    float (*db)[GROWS] = dg_s[s & 1];
    if (unit_thread) {
      const int64_t bt = (int64_t)ub * a.T + t;
      const float* gp = gin + bt * H4X;
      const float rg = gp[unit], zg = gp[H + unit], ng = gp[2 * H + unit], qg = gp[3 * H + unit];
      const float hp = t > 0 ? hin[(bt - 1) * H + unit] : 0.f;
      float d = (dhin ? dhin[bt * H + unit] : 0.f) + dz;
      if (s > 0) {
        gu64* g0 = gr + (s & 1) * par + (int64_t)ub * H + unit;
        float v[LMAX_H / LU];
        unsigned ready = 0, spins = 0;
        const unsigned all = (1u << G) - 1;
        while (ready != all) {
#pragma unroll
          for (int q = 0; q < LMAX_H / LU; ++q) {
            if (q < G && !(ready >> q & 1)) {
              const unsigned long long x =
                  __hip_atomic_load(g0 + (int64_t)q * B * H, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              if ((unsigned)(x >> 32) == (unsigned)s) { v[q] = __uint_as_float((unsigned)x); ready |= 1u << q; }
            }
          }
          if (ready == all) break;
          if (timed_out(++spins, a.timeout)) {
            atomicOr(a.timeout, 1u);
            // poison what never arrived: the gradients become NaN, never silently wrong
            for (int q = 0; q < LMAX_H / LU; ++q) if (!(ready >> q & 1)) v[q] = __builtin_nanf("");
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
#pragma unroll
        for (int q = 0; q < LMAX_H / LU; ++q) if (q < G) d += v[q];
      }
      const float d_n = d * (1.f - zg) * (1.f - ng * ng);
      const float d_z = d * (hp - ng) * zg * (1.f - zg);
      const float d_r = d_n * qg * rg * (1.f - rg);
      const float d_q = d_n * rg;
      dz = d * zg;
      float* dp = dgout + bt * H4X;
      dp[unit] = d_r;
      dp[H + unit] = d_z;
      dp[2 * H + unit] = d_n;
      dp[3 * H + unit] = d_q;
      db[ub][lu] = d_r;
      db[ub][LU + lu] = d_z;
      db[ub][2 * LU + lu] = d_q;
    }
    __syncthreads();
    if (t > 0) {
#pragma unroll
      for (int b = 0; b < LMAX_B; ++b) {
        if (b >= B) break;
        const float4* dr = reinterpret_cast<const float4*>(&db[b][rp * GRP]);
        f2v acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = f2v{0.f, 0.f};
#pragma unroll
        for (int i = 0; i < GRP / 4; ++i) {
          const float4 d4 = dr[i];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            acc[c] = __builtin_elementwise_fma(w[c][2 * i], f2v{d4.x, d4.y}, acc[c]);
            acc[c] = __builtin_elementwise_fma(w[c][2 * i + 1], f2v{d4.z, d4.w}, acc[c]);
          }
        }
        const float acc1 = transpose_reduce4(acc[0].x + acc[0].y, acc[1].x + acc[1].y, acc[2].x + acc[2].y,
                                             acc[3].x + acc[3].y, l);
        if ((l & 3) == 0 && k < H)
          put(gr + ((s + 1) & 1) * par + ((int64_t)j * B + b) * H + k, (unsigned)(s + 1), acc1);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Forward: wave b (< B) sweeps batch row b's H granules of h_{t-1} into LDS; lane l of wave w
// owns unit 4 w + (l >> 4) and the k slice (l & 15) * H / 16 of its 3 gate rows; after the
// transpose-reduce lane l holds a_gate with gate = (l >> 2) & 3 (gate 3: the idle slot, 0);
// every lane of the row then forms r, z, q, n; lane b updates row b's h.
// ---------------------------------------------------------------------------
constexpr int SWEEP_MAX = LMAX_H / 64;   // granules per lane

template <int HH>
__global__ __launch_bounds__(LNT) void gru_fwd_kernel(const GruArgs a) {
  __shared__ __attribute__((aligned(16))) float h_s[2][LMAX_B * LMAX_H];
  const int inst = blockIdx.x / a.G, j = blockIdx.x - inst * a.G;
  if (inst >= a.ninst) return;
  const int li = a.gru_of[inst], b0 = a.b0[inst];
  const int t0 = threadIdx.x;
  constexpr int H = HH, H3X = 3 * H, H4X = 4 * H;
  const int B = a.nb[inst];
  const float* xproj = a.xproj[li] + (int64_t)b0 * a.T * H3X;
  float* hout = a.h[li] + (int64_t)b0 * a.T * H;
  float* gout = a.gates[li] + (int64_t)b0 * a.T * H4X;
  gu64* gr = a.gran[li] + (int64_t)2 * a.G * b0 * H;
  const int l = t0 & 63;
  const int pb = t0 >> 6;   // poller wave of batch row pb
  const bool poller = pb < B;
  const int unit = j * LU + (t0 >> 6) * 4 + (l >> 4);
  // lane l of wave w: unit 4 w + (l >> 4); k slice (l & 15) * KP .. + KP of the 3 gate rows
  const int kp = l & 15, gate = (l >> 2) & 3, mb = l & 15;
  constexpr int KP = H / 16;
  const int grow = gate * H + unit;   // the slot of xproj (gate < 3) and of gates this lane serves
  const int nbh = B * H;
  f2v w[3][KP / 2];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    const float4* wr = reinterpret_cast<const float4*>(a.w_hh[li] + (int64_t)(g * H + unit) * H + kp * KP);
#pragma unroll
    for (int i = 0; i < KP / 4; ++i) {
      const float4 v = wr[i];
      w[g][2 * i] = f2v{v.x, v.y};
      w[g][2 * i + 1] = f2v{v.z, v.w};
    }
  }
  const float bhn = a.b_hn[li][unit];
  float hprev = 0.f;
  for (int t = 0; t < a.T; ++t) {
    float xv[LMAX_B];
#pragma unroll
    for (int b = 0; b < LMAX_B; ++b) xv[b] = (b < B && gate < 3) ? xproj[((int64_t)b * a.T + t) * H3X + grow] : 0.f;
    float* hb = h_s[t & 1];   // [b * H + k]
    if (poller) {
      float* dst = hb + pb * H;
      if (t == 0) {
        for (int k = l; k < H; k += 64) dst[k] = 0.f;
      } else {
        const gu64* src = gr + (int64_t)(t & 1) * nbh + pb * H;
        unsigned long long x[SWEEP_MAX];
        unsigned pending = 0;
#pragma unroll
        for (int p = 0; p < SWEEP_MAX; ++p)
          if (64 * p < H) {  // compile-time
            x[p] = __hip_atomic_load(src + l + 64 * p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            pending |= 1u << p;
          }
        for (unsigned spins = 0;; ++spins) {
#pragma unroll
          for (int p = 0; p < SWEEP_MAX; ++p)
            if ((pending >> p & 1) && (unsigned)(x[p] >> 32) == (unsigned)t) {
              dst[l + 64 * p] = __uint_as_float((unsigned)x[p]);
              pending &= ~(1u << p);
            }
          if (!pending) break;
          if (timed_out(spins, a.timeout)) {
            atomicOr(a.timeout, 1u);
#pragma unroll
            for (int p = 0; p < SWEEP_MAX; ++p)
              if (pending >> p & 1) dst[l + 64 * p] = __builtin_nanf("");   // poison: outputs become NaN
            break;
          }
          __builtin_amdgcn_s_sleep(1);
#pragma unroll
          for (int p = 0; p < SWEEP_MAX; ++p)
            if (pending >> p & 1)
              x[p] = __hip_atomic_load(src + l + 64 * p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    __syncthreads();
    float zg = 0.f, ng = 0.f;
#pragma unroll
    for (int b = 0; b < LMAX_B; ++b) {
      if (b >= B) break;
      const float4* hr = reinterpret_cast<const float4*>(hb + b * H + kp * KP);
      f2v acc[3];
#pragma unroll
      for (int g = 0; g < 3; ++g) acc[g] = f2v{0.f, 0.f};
#pragma unroll
      for (int i = 0; i < KP / 4; ++i) {
        const float4 h4 = hr[i];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          acc[g] = __builtin_elementwise_fma(w[g][2 * i], f2v{h4.x, h4.y}, acc[g]);
          acc[g] = __builtin_elementwise_fma(w[g][2 * i + 1], f2v{h4.z, h4.w}, acc[g]);
        }
      }
      // lane l ends with a_gate, gate = (l >> 2) & 3 (the fourth slot is idle: 0)
      const float acc1 = transpose_reduce4(acc[0].x + acc[0].y, acc[1].x + acc[1].y, acc[2].x + acc[2].y, 0.f, l);
      const float sg = fsigm(acc1 + xv[b]);                 // r in the gate-0 lanes, z in the gate-1 lanes
      const float vq = dpp<0x158>(acc1) + bhn;              // q = a_n + b_hn, in every lane of the row
      const float vx = dpp<0x158>(xv[b]);                   // xproj_n
      const float vr = dpp<0x150>(sg), vz = dpp<0x154>(sg);
      const float vn = ftanh(vx + vr * vq);                 // the dependent step: n needs r
      if ((l & 3) == 0)
        gout[((int64_t)b * a.T + t) * H4X + grow] = gate == 0 ? vr : gate == 1 ? vz : gate == 2 ? vn : vq;
      if (mb == b) { zg = vz; ng = vn; }
    }
    if (mb < B) {
      const float hv = ng + zg * (hprev - ng);   // (1 - z) n + z h_{t-1}
      hprev = hv;
      hout[((int64_t)mb * a.T + t) * H + unit] = hv;
      put(gr + (int64_t)((t + 1) & 1) * nbh + mb * H + unit, (unsigned)(t + 1), hv);
    }
  }
}

// split every GRU's batch into instances of <= LMAX_B rows (recurrence.h)
int gru_plan(GruArgs& a, int num_gru, int batch, int steps, int hidden, unsigned* timeout) {
  return recurrence_plan(a, a.gru_of, "gru", "GRUs", num_gru, batch, steps, hidden, timeout);
}

}  // namespace

}  // namespace mmf

using namespace mmf;

extern "C" {

size_t mmf_gru_sync_bytes(int32_t batch, int32_t hidden) { return recurrence_sync_bytes(batch, hidden); }

int mmf_gru_forward(int32_t num_gru, int32_t batch, int32_t steps, int32_t hidden, const float* const* xproj,
                    const float* const* w_hh, const float* const* b_hn, float* const* h, float* const* gates,
                    void* const* sync, uint32_t* timeout, void* stream) {
  GruArgs a;
  if (int rc = gru_plan(a, num_gru, batch, steps, hidden, timeout)) return rc;
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < num_gru; ++i)
    if (reinterpret_cast<uintptr_t>(w_hh[i]) & 15) return fail(MMF_EINVAL, "gru: w_hh must be 16-byte aligned");
  for (int i = 0; i < num_gru; ++i) {
    a.xproj[i] = xproj[i]; a.w_hh[i] = w_hh[i]; a.b_hn[i] = b_hn[i]; a.h[i] = h[i]; a.gates[i] = gates[i];
    a.gran[i] = (gu64*)sync[i];
  }
  // every polled word is zeroed before the launch (epochs start at 1); the timeout word per
  // call (a stale flag never aborts waits); one zero-fill kernel (graph-capturable)
  if (int rc = zero_sync(num_gru, batch, hidden, sync, timeout, st)) return rc;
  const int grid = a.G * a.ninst;
  void (*kern)(const GruArgs) = hidden == 64    ? gru_fwd_kernel<64>
                                : hidden == 128 ? gru_fwd_kernel<128>
                                : hidden == 192 ? gru_fwd_kernel<192>
                                                : gru_fwd_kernel<256>;
  if (int rc = check_coresident(kern, grid, "gru forward")) return rc;
  ProfLaunch prof_(st, "gru_fwd_kernel", 6.0 * num_gru * batch * steps * hidden * hidden,
                   4.0 * num_gru * ((double)3 * hidden * hidden + (double)batch * steps * 8 * hidden));
  mmf_launch(kern, dim3(grid), dim3(LNT), 0, st, a);
  HIP_TRY(hipGetLastError());
  return MMF_OK;
}

int mmf_gru_backward(int32_t num_gru, int32_t batch, int32_t steps, int32_t hidden, const float* const* w_hh,
                     const float* const* h, const float* const* gates, const float* const* dh,
                     float* const* dgates, void* const* sync, uint32_t* timeout, void* stream) {
  GruArgs a;
  if (int rc = gru_plan(a, num_gru, batch, steps, hidden, timeout)) return rc;
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < num_gru; ++i)
    if (reinterpret_cast<uintptr_t>(w_hh[i]) & 15) return fail(MMF_EINVAL, "gru: w_hh must be 16-byte aligned");
  for (int i = 0; i < num_gru; ++i) {
    a.w_hh[i] = w_hh[i]; a.h[i] = (float*)h[i]; a.gates[i] = (float*)gates[i]; a.dh[i] = dh[i];
    a.dgates[i] = dgates[i]; a.gran[i] = (gu64*)sync[i];
  }
  if (int rc = zero_sync(num_gru, batch, hidden, sync, timeout, st)) return rc;
  if (int rc = check_coresident(gru_bwd_kernel, a.G * a.ninst, "gru backward")) return rc;
  ProfLaunch prof_(st, "gru_bwd_kernel", 6.0 * num_gru * batch * steps * hidden * hidden,
                   4.0 * num_gru * ((double)3 * hidden * hidden + (double)batch * steps * 11 * hidden));
  mmf_launch(gru_bwd_kernel, dim3(a.G * a.ninst), dim3(LNT), 0, st, a);
  HIP_TRY(hipGetLastError());
  return MMF_OK;
}

}  // extern "C"
