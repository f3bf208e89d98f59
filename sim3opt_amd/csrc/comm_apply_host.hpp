// comm_apply_host.hpp -- the host half of the transport's diagnostic read-outs (sim3opt_comm_apply_*, capi.cpp): what is
// decided about the arguments and the plans for ALL ranks before any rank enters a collective.  Each check returns the
// message of the refusal (SIM3OPT_ERR_ARG), or an empty string.  Plain C++, no HIP: tests/cxx/comm_apply_host_driver.cpp
// runs it under AddressSanitizer + UndefinedBehaviorSanitizer.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace sim3opt {

// offs[0 .. world]: never decreasing from offs[0] >= 0
inline bool comm_offsets_ok(const int64_t* offs, int32_t world) {
  if (offs[0] < 0) return false;
  for (int32_t r = 0; r < world; ++r)
    if (offs[r + 1] < offs[r]) return false;
  return true;
}

inline bool comm_phase_ok(int32_t phase) { return phase == 0 || phase == 1; }

// (k_comm_reduce counts in int: n stays well inside it)
inline std::string comm_check_allreduce(int64_t n, int32_t op, int32_t phase, const void* in, const void* out) {
  if (!in || !out) return "comm_apply_allreduce: null argument";
  if (n < 0 || n > ((int64_t)1 << 30)) return "comm_apply_allreduce: n must be in 0 .. 2^30";
  if (op != 0 && op != 1) return "comm_apply_allreduce: op is 0 (sum) or 1 (max)";
  if (!comm_phase_ok(phase)) return "comm_apply_allreduce: phase is 0 or 1";
  return "";
}

inline std::string comm_check_allgatherv(const int64_t* offs, int32_t world, int32_t phase, const void* in,
                                         const void* out) {
  if (!offs || !in || !out) return "comm_apply_allgatherv: null argument";
  if (!comm_phase_ok(phase)) return "comm_apply_allgatherv: phase is 0 or 1";
  if (offs[0] != 0 || !comm_offsets_ok(offs, world)) return "comm_apply_allgatherv: offsets start at 0 and never decrease";
  return "";
}

// soffs, roffs: world rows of world + 1 offsets.  On success sbase / rbase [0 .. world] are where rank r's buffers start
// in the concatenated send / receive arrays.
inline std::string comm_check_exchange(const int64_t* soffs, const int64_t* roffs, int32_t world, int32_t send_phase,
                                       int32_t recv_phase, const void* send, const void* recv,
                                       std::vector<int64_t>& sbase, std::vector<int64_t>& rbase) {
  if (!soffs || !roffs || !send || !recv) return "comm_apply_exchange: null argument";
  if (!comm_phase_ok(send_phase) || !comm_phase_ok(recv_phase)) return "comm_apply_exchange: a phase is 0 or 1";
  const int64_t w1 = (int64_t)world + 1;
  sbase.assign((size_t)w1, 0);
  rbase.assign((size_t)w1, 0);
  for (int32_t r = 0; r < world; ++r) {
    if (!comm_offsets_ok(soffs + r * w1, world) || !comm_offsets_ok(roffs + r * w1, world))
      return "comm_apply_exchange: rank " + std::to_string(r) + ": offsets must start at 0 or above and never decrease";
    sbase[r + 1] = sbase[r] + soffs[r * w1 + world];
    rbase[r + 1] = rbase[r] + roffs[r * w1 + world];
  }
  for (int32_t p = 0; p < world; ++p)
    for (int32_t q = 0; q < world; ++q) {
      const int64_t ns = soffs[p * w1 + q + 1] - soffs[p * w1 + q], nr = roffs[q * w1 + p + 1] - roffs[q * w1 + p];
      if (ns != nr)
        return "comm_apply_exchange: the plans disagree: rank " + std::to_string(p) + " sends " + std::to_string(ns) +
               " doubles to rank " + std::to_string(q) + ", which receives " + std::to_string(nr) + " from it";
    }
  return "";
}

}  // namespace sim3opt
