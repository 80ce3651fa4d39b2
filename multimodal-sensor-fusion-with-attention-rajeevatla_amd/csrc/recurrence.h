// The persistent recurrence that lstm.hip and gru.hip share; each of them adds only its cell.
//
// One launch runs a whole layer of up to 8 networks: every network's batch is split into instances
// of <= 4 rows, and G = H / 64 workgroups of 1024 threads per instance each keep their 64 hidden
// units' NG x 64 rows of W_hh in VGPRs (NG gate rows per unit: 4 for the LSTM, 3 for the GRU; loaded
// once) and exchange h_t every step through tagged 8-byte granules {epoch, value}: agent-scope
// relaxed atomic stores and polls, double-buffered by step parity, the data is its own flag (CDNA
// guide §6 Guideline 16, R2).  Nothing is ordered by dispatch or placement.  Every spin is bounded:
// a wait that gives up sets the call's timeout word and poisons the missing values with NaN, so the
// results can never be silently wrong.  The granules and the timeout word are zeroed before every
// launch (epochs start at 1).
//
// Forward, per step and workgroup: wave b (< B) sweeps batch row b's H granules of h_{t-1} into LDS
// (sweep_row: one wave per row polls, MI355X_MICROARCH.md handoff-1to1: the price of a hand-off sits
// in the consumer CU's memory queue); one barrier; lane l of wave w owns unit 4 w + (l >> 4) and the
// k slice (l & 15) * H / 16 of its NG gate rows and runs the matvec as packed FMAs on the
// register-resident weights against LDS-broadcast operands (16 lanes share an NG x 16 weight block
// per row so each lane reads 16 operands, not 64: the LDS read rate, not the FMA rate, bounded the
// first version); the partial sums are transpose-reduced across the 16 lanes with DPP moves (no LDS
// round trip), which leaves gate (l >> 2) & 3 in lane l (fwd_matvec).  The cell follows and
// publishes h_t with `put`.
//
// Backward, the same in reverse: lane u of wave b gathers the G partials of (W_hh^T dgates)[b][unit
// u] with independent loads, sums them in a fixed order (gather_partials) and runs the cell backward
// directly into a double-buffered LDS block of NG x 64 local rows (row = gate * 64 + unit); one
// barrier; every workgroup publishes its partial of the transposed matvec for every hidden unit
// (bwd_matvec_put).  The time-parallel GEMMs (input projection, weight gradients) are the caller's.
#pragma once

#include <cmath>

#include "capi_util.h"

namespace mmf {

namespace {

typedef __attribute__((address_space(1))) unsigned long long gu64;
constexpr int LNT = 1024;          // threads per workgroup
constexpr int LU = 64;             // hidden units per workgroup
constexpr int LMAX_B = 4;          // batch rows per instance (one workgroup group)
constexpr int LMAX_H = 256;
constexpr int LMAX_N = 8;          // networks per launch (one per modality)
constexpr int LMAX_I = 32;         // instances per launch: (network, <= 4 batch rows) pairs
constexpr unsigned SPIN_LIMIT = 1u << 20;   // ~1 s of polling
constexpr int SWEEP_MAX = LMAX_H / 64;      // granules per lane of the forward's sweep

// The kernels' argument, for both cells and both directions; what a kernel does not use stays null.
struct RecArgs {
  int T, H, G, ninst;
  int8_t net_of[LMAX_I];           // instance -> network
  int16_t b0[LMAX_I];              // instance -> first batch row
  int8_t nb[LMAX_I];               // instance -> batch rows (<= 4)
  const float* xproj[LMAX_N];      // (B, T, NG H)
  const float* w_hh[LMAX_N];       // (NG H, H)
  const float* b_hn[LMAX_N];       // (H), GRU
  float* h[LMAX_N];                // (B, T, H)
  float* c[LMAX_N];                // (B, T, H), LSTM
  float* gates[LMAX_N];            // (B, T, 4H) what the cell saves for its backward
  // backward
  const float* dh[LMAX_N];         // (B, T, H) upstream gradient of every h_t (may be null)
  float* dgates[LMAX_N];           // (B, T, 4H)
  gu64* gran[LMAX_N];              // 2 x G x B x H granules (the forward uses 2 x B x H)
  unsigned* timeout;
};

// fast activations for the recurrences: v_exp_f32 + v_rcp_f32 (a few ulp; parity is 1e-3 relative)
__device__ __forceinline__ float fsigm(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float ftanh(float x) { return 2.f * __builtin_amdgcn_rcpf(1.f + __expf(-2.f * x)) - 1.f; }

// DPP lane moves (no LDS round trip): quad_perm xor 1 / xor 2, row_newbcast:n (lane n of each 16-lane row)
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float quad_sum(float v) {
  v += dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  return v + dpp<0x4E>(v);   // quad_perm [2,3,0,1]
}

typedef float f2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void put(gu64* g, unsigned epoch, float v) {
  __hip_atomic_store(g, ((unsigned long long)epoch << 32) | __float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool timed_out(unsigned spins, unsigned* tmo) {
  return (spins & 255) == 255 && tmo &&
         (spins > SPIN_LIMIT || __hip_atomic_load(tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// lane l (of a 16-lane row) holds partials P0..P3 of four outputs; returns, in lane l, the
// row-wide total of output (l >> 2) & 3
__device__ __forceinline__ float transpose_reduce4(float P0, float P1, float P2, float P3, int l) {
  const bool b3 = (l >> 3) & 1, b2 = (l >> 2) & 1;
  const float r0 = (b3 ? P2 : P0) + dpp<0x128>(b3 ? P0 : P2);   // row_ror:8 (lane l ^ 8)
  const float r1 = (b3 ? P3 : P1) + dpp<0x128>(b3 ? P1 : P3);
  const float snd = b2 ? r0 : r1;
  const float from_lo = dpp<0x124>(snd), from_hi = dpp<0x12C>(snd);   // row_ror:4 / :12 (lanes l - 4, l + 4)
  return quad_sum((b2 ? r1 : r0) + (b2 ? from_lo : from_hi));
}
// the same for the column sums of NG (3 or 4) packed accumulators; an idle fourth slot is 0
template <int NG>
__device__ __forceinline__ float transpose_reduce(const f2v (&acc)[NG], int l) {
  return transpose_reduce4(acc[0].x + acc[0].y, acc[1].x + acc[1].y, acc[2].x + acc[2].y,
                           NG > 3 ? acc[NG - 1].x + acc[NG - 1].y : 0.f, l);
}

// The matvec loop of both directions: acc[r] = the two interleaved halves of w[r] . x, for R rows
// of 2 N2 register-resident weights (packed in pairs along x) against 2 N2 floats of an LDS row
template <int R, int N2>
__device__ __forceinline__ void packed_dot(f2v (&acc)[R], const f2v (&w)[R][N2], const float4* x) {
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = f2v{0.f, 0.f};
#pragma unroll
  for (int i = 0; i < N2 / 2; ++i) {
    const float4 x4 = x[i];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      acc[r] = __builtin_elementwise_fma(w[r][2 * i], f2v{x4.x, x4.y}, acc[r]);
      acc[r] = __builtin_elementwise_fma(w[r][2 * i + 1], f2v{x4.z, x4.w}, acc[r]);
    }
  }
}

// The workgroup's place in the plan (recurrence_plan): workgroup j of the G of its instance, the
// instance's network, first batch row and row count.  False for a workgroup past the last instance.
struct Instance { int j, net, b0, B; };
__device__ __forceinline__ bool find_instance(const RecArgs& a, Instance& in) {
  const int inst = blockIdx.x / a.G;
  if (inst >= a.ninst) return false;
  in = Instance{(int)blockIdx.x - inst * a.G, a.net_of[inst], a.b0[inst], a.nb[inst]};
  return true;
}

// ---------------------------------------------------------------------------
// Forward.  KP = H / 16 is a lane's k slice.
// ---------------------------------------------------------------------------
// w[g][.] = W_hh[g * H + unit][kp * KP .. + KP]
template <int NG, int H>
__device__ __forceinline__ void fwd_load_w(f2v (&w)[NG][H / 32], const float* w_hh, int unit, int kp) {
  constexpr int KP = H / 16;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const float4* wr = reinterpret_cast<const float4*>(w_hh + (int64_t)(g * H + unit) * H + kp * KP);
#pragma unroll
    for (int i = 0; i < KP / 4; ++i) {
      const float4 v = wr[i];
      w[g][2 * i] = f2v{v.x, v.y};
      w[g][2 * i + 1] = f2v{v.z, v.w};
    }
  }
}

// One wave: the H values of h_{t-1} of one batch row (zeros at t = 0) from the granules `src` of
// step t's parity into the LDS row `dst`: H / 64 loads per lane in flight at once, then only the
// missing ones are polled again.
template <int H>
__device__ __forceinline__ void sweep_row(float* dst, const gu64* src, int t, int l, unsigned* tmo) {
  if (t == 0) {
    for (int k = l; k < H; k += 64) dst[k] = 0.f;
    return;
  }
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
    if (timed_out(spins, tmo)) {
      atomicOr(tmo, 1u);
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

// (W_hh h_{t-1}) of one batch row: `hk` is the lane's k slice of the row in LDS; lane l ends with the
// total of gate row (l >> 2) & 3 of its unit
template <int NG, int H>
__device__ __forceinline__ float fwd_matvec(const f2v (&w)[NG][H / 32], const float* hk, int l) {
  f2v acc[NG];
  packed_dot(acc, w, reinterpret_cast<const float4*>(hk));
  return transpose_reduce(acc, l);
}

// ---------------------------------------------------------------------------
// Backward.  Matvec lanes: wave w, lane l -> local rows rp * RP .. + RP with rp = l & 15 and
// RP = NG * 64 / 16 (a lane's rows may straddle a gate boundary: the row index is split per row),
// hidden columns kc .. kc + 3 with kc = 4 (4 w + (l >> 4)); the butterfly leaves column
// kc + ((l >> 2) & 3) in lane l.
// ---------------------------------------------------------------------------
// w[c][i / 2] = W_hh[grow(rp * RP + i)][kc + c] (zeros in the lanes with kc >= H)
template <int NG>
__device__ __forceinline__ void bwd_load_w(f2v (&w)[4][2 * NG], const float* w_hh, int H, int j, int rp, int kc) {
  constexpr int RP = 4 * NG;
#pragma unroll
  for (int i = 0; i < RP; i += 2) {
    float4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if (kc < H) {
      const int r0 = rp * RP + i, r1 = r0 + 1;
      v0 = *reinterpret_cast<const float4*>(w_hh + (int64_t)((r0 >> 6) * H + j * LU + (r0 & 63)) * H + kc);
      v1 = *reinterpret_cast<const float4*>(w_hh + (int64_t)((r1 >> 6) * H + j * LU + (r1 & 63)) * H + kc);
    }
    w[0][i / 2] = f2v{v0.x, v1.x};
    w[1][i / 2] = f2v{v0.y, v1.y};
    w[2][i / 2] = f2v{v0.z, v1.z};
    w[3][i / 2] = f2v{v0.w, v1.w};
  }
}

// d + the G partials of step s that the workgroups published for one (row, unit): granules g0,
// g0 + B H, ...; independent loads, only the missing ones polled again, summed for q ascending.
// `v` is scratch registers of the caller's (declared in its step body, as before the kernels shared
// this code: with the array local to this function gru_bwd_kernel is allocated differently)
__device__ __forceinline__ float gather_partials(float (&v)[LMAX_H / LU], float d, gu64* g0, int B, int H, int G,
                                                 int s, unsigned* tmo) {
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
    if (timed_out(++spins, tmo)) {
      atomicOr(tmo, 1u);
      // poison what never arrived: the gradients become NaN, never silently wrong
      for (int q = 0; q < LMAX_H / LU; ++q) if (!(ready >> q & 1)) v[q] = __builtin_nanf("");
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
#pragma unroll
  for (int q = 0; q < LMAX_H / LU; ++q) if (q < G) d += v[q];
  return d;
}

// The workgroup's partial of W_hh^T dg for every batch row, over its NG x 64 local rows `db` (LDS),
// published into the G x B x H granules `out` with tag `epoch`; the lane ends with column k
template <int NG>
__device__ __forceinline__ void bwd_matvec_put(const f2v (&w)[4][2 * NG], const float (*db)[NG * LU], int B, int H,
                                               int l, int j, int k, gu64* out, unsigned epoch) {
#pragma unroll
  for (int b = 0; b < LMAX_B; ++b) {
    if (b >= B) break;
    f2v acc[4];
    packed_dot(acc, w, reinterpret_cast<const float4*>(&db[b][(l & 15) * 4 * NG]));
    const float acc1 = transpose_reduce(acc, l);
    if ((l & 3) == 0 && k < H) put(out + ((int64_t)j * B + b) * H + k, epoch, acc1);
  }
}

// ---------------------------------------------------------------------------
// Host
// ---------------------------------------------------------------------------
// The recurrence needs every workgroup of the grid resident at once (they wait on
// each other's granules).  Refuse a grid the device cannot hold even when idle;
// residency under concurrent kernels (e.g. RCCL under DDP) is not guaranteed, which
// the bounded spins + NaN poisoning + per-call timeout word make loud, not silent.
template <typename K>
int check_coresident(K kernel, int grid, const char* what) {
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, LNT, 0) != hipSuccess)
    return fail(MMF_EHIP, "%s: occupancy query failed", what);
  if ((int64_t)per_cu * cus < grid)
    return fail(MMF_ELIMIT, "%s: %d workgroups of %d threads cannot be co-resident (%d per CU x %d CUs)", what,
                grid, LNT, per_cu, cus);
  return MMF_OK;
}

// Split every network's batch into instances of <= LMAX_B rows; the pointers of `a` stay null for
// the caller to fill.  `what` / `many` name the cell in the messages ("lstm" / "LSTMs").
inline int recurrence_plan(RecArgs& a, const char* what, const char* many, int num, int batch, int steps, int hidden,
                           unsigned* timeout) {
  if (num < 1 || num > LMAX_N || batch < 1 || steps < 1 || hidden < LU || hidden > LMAX_H || hidden % LU != 0)
    return fail(MMF_ELIMIT, "%s: 1..%d %s, hidden a multiple of %d up to %d (got n=%d B=%d T=%d H=%d)", what,
                LMAX_N, many, LU, LMAX_H, num, batch, steps, hidden);
  const int per = (batch + LMAX_B - 1) / LMAX_B;
  if (per * num > LMAX_I)
    return fail(MMF_ELIMIT, "%s: num_%s x ceil(batch / %d) = %d instances (max %d)", what, what, LMAX_B, per * num,
                LMAX_I);
  if (!timeout) return fail(MMF_EINVAL, "%s: a device timeout word is required", what);
  memset(&a, 0, sizeof(a));
  a.T = steps; a.H = hidden; a.G = hidden / LU; a.timeout = timeout;
  for (int i = 0; i < num; ++i)
    for (int b = 0; b < batch; b += LMAX_B) {
      a.net_of[a.ninst] = (int8_t)i;
      a.b0[a.ninst] = (int16_t)b;
      a.nb[a.ninst] = (int8_t)(batch - b < LMAX_B ? batch - b : LMAX_B);
      ++a.ninst;
    }
  return MMF_OK;
}

// 2 parities x G x B x H granules (the backward's partial sums; >= the forward's 2 x B x H)
inline size_t recurrence_sync_bytes(int32_t batch, int32_t hidden) {
  if (batch < 1 || hidden < 1) return 0;
  const size_t G = (size_t)(hidden + LU - 1) / LU;
  return 2 * G * (size_t)batch * hidden * sizeof(unsigned long long);
}

// the sync granules of every network and the timeout word, zeroed by one kernel
inline int zero_sync(const RecArgs& a, int num, int batch, hipStream_t st) {
  float* ptrs[LMAX_N + 1];
  int64_t counts[LMAX_N + 1];
  int n = 0;
  for (int i = 0; i < num; ++i) {
    ptrs[n] = (float*)a.gran[i];
    counts[n++] = (int64_t)(recurrence_sync_bytes(batch, a.H) / 4);
  }
  ptrs[n] = (float*)a.timeout;
  counts[n++] = 1;
  HIP_TRY(launch_zero_fill(ptrs, counts, n, st));
  return MMF_OK;
}

// One planned and filled recurrence launch.  `what` names the cell ("lstm"), `which` the launch
// ("lstm forward"), `kname` the kernel for the profile; flops / bytes are the launch's algorithmic
// work for the profile.
template <typename K>
int recurrence_launch(const RecArgs& a, K kernel, const char* what, const char* which, const char* kname, int num,
                      int batch, double flops, double bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < num; ++i)
    if (reinterpret_cast<uintptr_t>(a.w_hh[i]) & 15) return fail(MMF_EINVAL, "%s: w_hh must be 16-byte aligned", what);
  // every polled word is zeroed before the launch (epochs start at 1); the timeout word per
  // call (a stale flag never aborts waits); one zero-fill kernel (graph-capturable)
  if (int rc = zero_sync(a, num, batch, st)) return rc;
  const int grid = a.G * a.ninst;
  if (int rc = check_coresident(kernel, grid, which)) return rc;
  ProfLaunch prof_(st, kname, flops, bytes);
  mmf_launch(kernel, dim3(grid), dim3(LNT), 0, st, a);
  HIP_TRY(hipGetLastError());
  return MMF_OK;
}

}  // namespace

}  // namespace mmf
