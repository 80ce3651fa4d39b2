// What the persistent recurrences (lstm.hip, gru.hip) share: the limits, the tagged-granule
// exchange between the H / 64 workgroups of an instance ({epoch, value} 8-byte granules,
// agent-scope relaxed atomic stores and polls, double-buffered by step parity: the data is
// its own flag -- CDNA guide §6 Guideline 16, R2), the bound of every spin and the timeout
// word, the DPP transpose-reduce, the fast activations, the co-residency check, the split
// of every network's batch into instances of <= 4 rows, and the zero-fill of the granules
// and the timeout word before every launch.  One protocol, two cells.
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

// Split every network's batch into instances of <= LMAX_B rows.  `a` is the kernel's argument
// struct (T, H, G, ninst, b0, nb, timeout; `net_of` its instance -> network table); `what` /
// `many` name the cell in the messages ("lstm" / "LSTMs").
template <class A>
int recurrence_plan(A& a, int8_t (&net_of)[LMAX_I], const char* what, const char* many, int num, int batch,
                    int steps, int hidden, unsigned* timeout) {
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
      net_of[a.ninst] = (int8_t)i;
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
inline int zero_sync(int num, int batch, int hidden, void* const* sync, uint32_t* timeout, hipStream_t st) {
  float* ptrs[LMAX_N + 1];
  int64_t counts[LMAX_N + 1];
  int n = 0;
  for (int i = 0; i < num; ++i) {
    ptrs[n] = (float*)sync[i];
    counts[n++] = (int64_t)(recurrence_sync_bytes(batch, hidden) / 4);
  }
  ptrs[n] = (float*)timeout;
  counts[n++] = 1;
  HIP_TRY(launch_zero_fill(ptrs, counts, n, st));
  return MMF_OK;
}

}  // namespace

}  // namespace mmf
