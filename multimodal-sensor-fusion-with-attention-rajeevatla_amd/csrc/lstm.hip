// Persistent LSTM recurrence (SequenceEncoder, src/encoders.py:67-75,
// 135-166; PyTorch nn.LSTM semantics, gate order i, f, g, o):
//   pre_t = xproj_t + W_hh h_{t-1}          (xproj = x W_ih^T + b_ih + b_hh, precomputed)
//   c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g);  h_t = sigmoid(o) tanh(c_t)
// C3 spent 98 % of a step in MIOpen's LSTM: 1024 sequential steps of a
// 1024 x 256 recurrent matvec.  Here one launch runs the whole recurrence on the plan and the
// inter-workgroup exchange of recurrence.h, with 4 gate rows per unit (64 weight floats per
// thread at H = 256).  This file is the cell: after the forward's transpose-reduce lane l holds
// gate (l >> 2) & 3 of its unit, row_newbcast gathers the unit's 4 activations and lane b of the
// unit's 16-lane row updates batch row b's cell state, which it keeps in a register; the
// backward's owner lane keeps dc.  gates = the activated i, f, g, o; dgates = the gradient of
// the PRE-activation gates.
#include "recurrence.h"

namespace mmf {

namespace {

// Backward: lane u of wave b runs the cell backward of unit u, row b, straight after its gather
// (no barrier in between); dg_s is double-buffered, so one barrier per step remains.
__global__ __launch_bounds__(LNT) void lstm_bwd_kernel(const RecArgs a) {
  __shared__ __attribute__((aligned(16))) float dg_s[2][LMAX_B][4 * LU];
  Instance in;
  if (!find_instance(a, in)) return;
  const int j = in.j, li = in.net, b0 = in.b0, B = in.B;
  const int t0 = threadIdx.x;
  const int H = a.H, G = a.G, H4X = 4 * H;
  const float* cin = a.c[li] + (int64_t)b0 * a.T * H;
  const float* gin = a.gates[li] + (int64_t)b0 * a.T * H4X;
  const float* dhin = a.dh[li] ? a.dh[li] + (int64_t)b0 * a.T * H : nullptr;
  float* dgout = a.dgates[li] + (int64_t)b0 * a.T * H4X;
  gu64* gr = a.gran[li] + (int64_t)2 * G * b0 * H;
  const int l = t0 & 63;
  const int kc = ((t0 >> 6) * 4 + (l >> 4)) * 4;
  const int k = kc + ((l >> 2) & 3);
  f2v w[4][8];
  bwd_load_w<4>(w, a.w_hh[li], H, j, l & 15, kc);
  const int ub = t0 / LU, lu = t0 - ub * LU;
  const bool unit_thread = ub < B;
  const int unit = j * LU + lu;
  float dc = 0.f;
  const int64_t par = (int64_t)G * B * H;
  for (int s = 0; s < a.T; ++s) {
    const int t = a.T - 1 - s;
    float (*db)[4 * LU] = dg_s[s & 1];
    if (unit_thread) {
      const int64_t bt = (int64_t)ub * a.T + t;
      const float* gp = gin + bt * H4X;
      const float ig = gp[unit], fg = gp[H + unit], gg = gp[2 * H + unit], og = gp[3 * H + unit];
      const float ct = cin[bt * H + unit];
      const float cp = t > 0 ? cin[(bt - 1) * H + unit] : 0.f;
      float dh = dhin ? dhin[bt * H + unit] : 0.f;
      float v[LMAX_H / LU];
      if (s > 0)
        dh = gather_partials(v, dh, gr + (s & 1) * par + (int64_t)ub * H + unit, B, H, G, s, a.timeout);
      const float tc = ftanh(ct);
      dc += dh * og * (1.f - tc * tc);
      const float d_o = dh * tc * og * (1.f - og);
      const float d_i = dc * gg * ig * (1.f - ig);
      const float d_g = dc * ig * (1.f - gg * gg);
      const float d_f = dc * cp * fg * (1.f - fg);
      dc *= fg;
      float* dp = dgout + bt * H4X;
      dp[unit] = d_i;
      dp[H + unit] = d_f;
      dp[2 * H + unit] = d_g;
      dp[3 * H + unit] = d_o;
      db[ub][lu] = d_i;
      db[ub][LU + lu] = d_f;
      db[ub][2 * LU + lu] = d_g;
      db[ub][3 * LU + lu] = d_o;
    }
    __syncthreads();
    if (t > 0) bwd_matvec_put<4>(w, db, B, H, l, j, k, gr + ((s + 1) & 1) * par, (unsigned)(s + 1));
  }
}

#ifdef MMF_LSTM_PROBE
__device__ unsigned long long g_lstm_probe[2][8];
#define PROBE_DECL unsigned long long pr_acc[6] = {0, 0, 0, 0, 0, 0}; unsigned long long pr_t = __builtin_amdgcn_s_memtime();
#define PROBE(i) { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); pr_acc[i] += n_ - pr_t; pr_t = n_; }
#define PROBE_END                                                                         \
  if (blockIdx.x == 0 && (t0 == 0 || t0 == LNT - 64))                                     \
    for (int i = 0; i < 6; ++i) g_lstm_probe[t0 == 0 ? 0 : 1][i] = pr_acc[i];
#else
#define PROBE_DECL
#define PROBE(i)
#define PROBE_END
#endif

// Forward.  PROBE(0..4): the phase stamps of the diagnostic build (-DMMF_LSTM_PROBE).
template <int HH>
__global__ __launch_bounds__(LNT) void lstm_fwd_kernel(const RecArgs a) {
  __shared__ __attribute__((aligned(16))) float h_s[2][LMAX_B * LMAX_H];
  Instance in;
  if (!find_instance(a, in)) return;
  const int j = in.j, li = in.net, b0 = in.b0, B = in.B;
  const int t0 = threadIdx.x;
  constexpr int H = HH, H4X = 4 * H, KP = H / 16;
  const float* xproj = a.xproj[li] + (int64_t)b0 * a.T * H4X;
  float* hout = a.h[li] + (int64_t)b0 * a.T * H;
  float* cout = a.c[li] + (int64_t)b0 * a.T * H;
  float* gout = a.gates[li] + (int64_t)b0 * a.T * H4X;
  gu64* gr = a.gran[li] + (int64_t)2 * a.G * b0 * H;
  const int l = t0 & 63;
  const int pb = t0 >> 6;   // poller wave of batch row pb
  const bool poller = pb < B;
  const int unit = j * LU + (t0 >> 6) * 4 + (l >> 4);
  const int kp = l & 15, gate = (l >> 2) & 3, mb = l & 15;
  const int grow = gate * H + unit;   // the gate row this lane finishes (after the butterfly)
  const int nbh = B * H;
  f2v w[4][KP / 2];
  fwd_load_w<4, H>(w, a.w_hh[li], unit, kp);
  float c = 0.f;
  PROBE_DECL
  for (int t = 0; t < a.T; ++t) {
    float xv[LMAX_B];
#pragma unroll
    for (int b = 0; b < LMAX_B; ++b) xv[b] = b < B ? xproj[((int64_t)b * a.T + t) * H4X + grow] : 0.f;
    float* hb = h_s[t & 1];   // [b * H + k]
    PROBE(0)
    if (poller) sweep_row<H>(hb + pb * H, gr + (int64_t)(t & 1) * nbh + pb * H, t, l, a.timeout);
    PROBE(1)
    __syncthreads();
    PROBE(2)
    float ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f;
#pragma unroll
    for (int b = 0; b < LMAX_B; ++b) {
      if (b >= B) break;
      const float pre = fwd_matvec<4, H>(w, hb + b * H + kp * KP, l) + xv[b];
      const float act = gate == 2 ? ftanh(pre) : fsigm(pre);
      if ((l & 3) == 0) gout[((int64_t)b * a.T + t) * H4X + grow] = act;
      const float vi = dpp<0x150>(act), vf = dpp<0x154>(act);
      const float vg = dpp<0x158>(act), vo = dpp<0x15C>(act);
      if (mb == b) { ig = vi; fg = vf; gg = vg; og = vo; }
    }
    PROBE(3)
    if (mb < B) {
      c = fg * c + ig * gg;
      const float hv = og * ftanh(c);
      const int64_t bt = (int64_t)mb * a.T + t;
      hout[bt * H + unit] = hv;
      cout[bt * H + unit] = c;
      put(gr + (int64_t)((t + 1) & 1) * nbh + mb * H + unit, (unsigned)(t + 1), hv);
    }
    PROBE(4)
  }
  PROBE_END
}

}  // namespace

}  // namespace mmf

using namespace mmf;

extern "C" {

size_t mmf_lstm_sync_bytes(int32_t batch, int32_t hidden) { return recurrence_sync_bytes(batch, hidden); }

int mmf_lstm_forward(int32_t num_lstm, int32_t batch, int32_t steps, int32_t hidden, const float* const* xproj,
                     const float* const* w_hh, float* const* h, float* const* c, float* const* gates,
                     void* const* sync, uint32_t* timeout, void* stream) {
  RecArgs a;
  if (int rc = recurrence_plan(a, "lstm", "LSTMs", num_lstm, batch, steps, hidden, timeout)) return rc;
  for (int i = 0; i < num_lstm; ++i) {
    a.xproj[i] = xproj[i]; a.w_hh[i] = w_hh[i]; a.h[i] = h[i]; a.c[i] = c[i]; a.gates[i] = gates[i];
    a.gran[i] = (gu64*)sync[i];
  }
  void (*kern)(const RecArgs) = hidden == 64    ? lstm_fwd_kernel<64>
                                : hidden == 128 ? lstm_fwd_kernel<128>
                                : hidden == 192 ? lstm_fwd_kernel<192>
                                                : lstm_fwd_kernel<256>;
  return recurrence_launch(a, kern, "lstm", "lstm forward", "lstm_fwd_kernel", num_lstm, batch,
                           8.0 * num_lstm * batch * steps * hidden * hidden,
                           4.0 * num_lstm * ((double)4 * hidden * hidden + (double)batch * steps * 10 * hidden), stream);
}

int mmf_lstm_backward(int32_t num_lstm, int32_t batch, int32_t steps, int32_t hidden,
                      const float* const* w_hh, const float* const* c, const float* const* gates,
                      const float* const* dh, float* const* dgates, void* const* sync, uint32_t* timeout,
                      void* stream) {
  RecArgs a;
  if (int rc = recurrence_plan(a, "lstm", "LSTMs", num_lstm, batch, steps, hidden, timeout)) return rc;
  for (int i = 0; i < num_lstm; ++i) {
    a.w_hh[i] = w_hh[i]; a.c[i] = (float*)c[i]; a.gates[i] = (float*)gates[i]; a.dh[i] = dh[i];
    a.dgates[i] = dgates[i]; a.gran[i] = (gu64*)sync[i];
  }
  return recurrence_launch(a, lstm_bwd_kernel, "lstm", "lstm backward", "lstm_bwd_kernel", num_lstm, batch,
                           8.0 * num_lstm * batch * steps * hidden * hidden,
                           4.0 * num_lstm * ((double)4 * hidden * hidden + (double)batch * steps * 14 * hidden), stream);
}

#ifdef MMF_LSTM_PROBE
int mmf_lstm_probe_read(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lstm_probe), sizeof(g_lstm_probe)) == hipSuccess ? 0 : 3;
}
#endif

}  // extern "C"
