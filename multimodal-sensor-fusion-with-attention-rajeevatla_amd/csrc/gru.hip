// Persistent GRU recurrence (SequenceEncoder 'gru', src/encoders.py:77-85, 135-166; PyTorch
// nn.GRU semantics, gate order r, z, n, zero initial state):
//   a_t = W_hh h_{t-1}             (xproj = x W_ih^T + b_ih + [b_hr, b_hz, 0], precomputed)
//   r = sigmoid(xproj_r + a_r);  z = sigmoid(xproj_z + a_z)
//   q = a_n + b_hn;  n = tanh(xproj_n + r q);  h_t = (1 - z) n + z h_{t-1}
// The LSTM's sibling (lstm.hip) on the plan and the inter-workgroup exchange of recurrence.h, with
// 3 gate rows per unit (48 weight floats per thread at H = 256).  This file is the cell.
//
// It is not the LSTM's: three gate rows sit in the four-slot transpose-reduce (the fourth slot
// idle), and n needs r.  After the one cross-lane reduce every lane of a unit's 16-lane row
// takes r, z (row_newbcast of the sigmoids), a_n and xproj_n (row_newbcast of the reduce's output
// and of the input) and computes n itself: the dependent step costs one more activation in the
// chain and four DPP moves, no second barrier and no LDS round trip.  b_hn cannot be folded into
// xproj (it is multiplied by r), so it rides in a register.  The owner lane keeps h_{t-1} in a
// register (there is no cell state).  The backward's carry is d z + W_hh^T [dr, dz, dn r]: the
// owner keeps d z in a register and the workgroups exchange their partials of the matvec over
// 3 x 64 local rows.  gates = r, z, n, q; dgates = dr_pre, dz_pre, dn_pre, dn_pre * r.
#include "recurrence.h"

namespace mmf {

namespace {

// Backward: lane u of wave b runs the cell backward of unit u, row b, straight after its gather;
// dg_s is double-buffered: one barrier per step.
__global__ __launch_bounds__(LNT) void gru_bwd_kernel(const RecArgs a) {
  __shared__ __attribute__((aligned(16))) float dg_s[2][LMAX_B][3 * LU];
  Instance in;
  if (!find_instance(a, in)) return;
  const int j = in.j, li = in.net, b0 = in.b0, B = in.B;
  const int t0 = threadIdx.x;
  const int H = a.H, G = a.G, H4X = 4 * H;
  const float* hin = a.h[li] + (int64_t)b0 * a.T * H;
  const float* gin = a.gates[li] + (int64_t)b0 * a.T * H4X;
  const float* dhin = a.dh[li] ? a.dh[li] + (int64_t)b0 * a.T * H : nullptr;
  float* dgout = a.dgates[li] + (int64_t)b0 * a.T * H4X;
  gu64* gr = a.gran[li] + (int64_t)2 * G * b0 * H;
  const int l = t0 & 63;
  const int kc = ((t0 >> 6) * 4 + (l >> 4)) * 4;
  const int k = kc + ((l >> 2) & 3);
  f2v w[4][6];
  bwd_load_w<3>(w, a.w_hh[li], H, j, l & 15, kc);
  const int ub = t0 / LU, lu = t0 - ub * LU;
  const bool unit_thread = ub < B;
  const int unit = j * LU + lu;
  float dz = 0.f;   // d_{t+1} z_{t+1}: the local term of the carry
  const int64_t par = (int64_t)G * B * H;
  for (int s = 0; s < a.T; ++s) {
    const int t = a.T - 1 - s;
    float (*db)[3 * LU] = dg_s[s & 1];
    if (unit_thread) {
      const int64_t bt = (int64_t)ub * a.T + t;
      const float* gp = gin + bt * H4X;
      const float rg = gp[unit], zg = gp[H + unit], ng = gp[2 * H + unit], qg = gp[3 * H + unit];
      const float hp = t > 0 ? hin[(bt - 1) * H + unit] : 0.f;
      float d = (dhin ? dhin[bt * H + unit] : 0.f) + dz;
      float v[LMAX_H / LU];
      if (s > 0)
        d = gather_partials(v, d, gr + (s & 1) * par + (int64_t)ub * H + unit, B, H, G, s, a.timeout);
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
    if (t > 0) bwd_matvec_put<3>(w, db, B, H, l, j, k, gr + ((s + 1) & 1) * par, (unsigned)(s + 1));
  }
}

// Forward: after the transpose-reduce lane l holds a_gate with gate = (l >> 2) & 3 (gate 3: the
// idle slot, 0); every lane of the unit's row then forms r, z, q, n; lane b updates row b's h.
template <int HH>
__global__ __launch_bounds__(LNT) void gru_fwd_kernel(const RecArgs a) {
  __shared__ __attribute__((aligned(16))) float h_s[2][LMAX_B * LMAX_H];
  Instance in;
  if (!find_instance(a, in)) return;
  const int j = in.j, li = in.net, b0 = in.b0, B = in.B;
  const int t0 = threadIdx.x;
  constexpr int H = HH, H3X = 3 * H, H4X = 4 * H, KP = H / 16;
  const float* xproj = a.xproj[li] + (int64_t)b0 * a.T * H3X;
  float* hout = a.h[li] + (int64_t)b0 * a.T * H;
  float* gout = a.gates[li] + (int64_t)b0 * a.T * H4X;
  gu64* gr = a.gran[li] + (int64_t)2 * a.G * b0 * H;
  const int l = t0 & 63;
  const int pb = t0 >> 6;   // poller wave of batch row pb
  const bool poller = pb < B;
  const int unit = j * LU + (t0 >> 6) * 4 + (l >> 4);
  const int kp = l & 15, gate = (l >> 2) & 3, mb = l & 15;
  const int grow = gate * H + unit;   // the slot of xproj (gate < 3) and of gates this lane serves
  const int nbh = B * H;
  f2v w[3][KP / 2];
  fwd_load_w<3, H>(w, a.w_hh[li], unit, kp);
  const float bhn = a.b_hn[li][unit];
  float hprev = 0.f;
  for (int t = 0; t < a.T; ++t) {
    float xv[LMAX_B];
#pragma unroll
    for (int b = 0; b < LMAX_B; ++b) xv[b] = (b < B && gate < 3) ? xproj[((int64_t)b * a.T + t) * H3X + grow] : 0.f;
    float* hb = h_s[t & 1];   // [b * H + k]
    if (poller) sweep_row<H>(hb + pb * H, gr + (int64_t)(t & 1) * nbh + pb * H, t, l, a.timeout);
    __syncthreads();
    float zg = 0.f, ng = 0.f;
#pragma unroll
    for (int b = 0; b < LMAX_B; ++b) {
      if (b >= B) break;
      const float acc1 = fwd_matvec<3, H>(w, hb + b * H + kp * KP, l);
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

}  // namespace

}  // namespace mmf

using namespace mmf;

extern "C" {

size_t mmf_gru_sync_bytes(int32_t batch, int32_t hidden) { return recurrence_sync_bytes(batch, hidden); }

int mmf_gru_forward(int32_t num_gru, int32_t batch, int32_t steps, int32_t hidden, const float* const* xproj,
                    const float* const* w_hh, const float* const* b_hn, float* const* h, float* const* gates,
                    void* const* sync, uint32_t* timeout, void* stream) {
  RecArgs a;
  if (int rc = recurrence_plan(a, "gru", "GRUs", num_gru, batch, steps, hidden, timeout)) return rc;
  for (int i = 0; i < num_gru; ++i) {
    a.xproj[i] = xproj[i]; a.w_hh[i] = w_hh[i]; a.b_hn[i] = b_hn[i]; a.h[i] = h[i]; a.gates[i] = gates[i];
    a.gran[i] = (gu64*)sync[i];
  }
  void (*kern)(const RecArgs) = hidden == 64    ? gru_fwd_kernel<64>
                                : hidden == 128 ? gru_fwd_kernel<128>
                                : hidden == 192 ? gru_fwd_kernel<192>
                                                : gru_fwd_kernel<256>;
  return recurrence_launch(a, kern, "gru", "gru forward", "gru_fwd_kernel", num_gru, batch,
                           6.0 * num_gru * batch * steps * hidden * hidden,
                           4.0 * num_gru * ((double)3 * hidden * hidden + (double)batch * steps * 8 * hidden), stream);
}

int mmf_gru_backward(int32_t num_gru, int32_t batch, int32_t steps, int32_t hidden, const float* const* w_hh,
                     const float* const* h, const float* const* gates, const float* const* dh,
                     float* const* dgates, void* const* sync, uint32_t* timeout, void* stream) {
  RecArgs a;
  if (int rc = recurrence_plan(a, "gru", "GRUs", num_gru, batch, steps, hidden, timeout)) return rc;
  for (int i = 0; i < num_gru; ++i) {
    a.w_hh[i] = w_hh[i]; a.h[i] = (float*)h[i]; a.gates[i] = (float*)gates[i]; a.dh[i] = dh[i];
    a.dgates[i] = dgates[i]; a.gran[i] = (gu64*)sync[i];
  }
  return recurrence_launch(a, gru_bwd_kernel, "gru", "gru backward", "gru_bwd_kernel", num_gru, batch,
                           6.0 * num_gru * batch * steps * hidden * hidden,
                           4.0 * num_gru * ((double)3 * hidden * hidden + (double)batch * steps * 11 * hidden), stream);
}

}  // extern "C"
