// The account table's predecessor search on the host (gpu_accounts.hip: a batch whose per-address list is longer than the chain cap; DESIGN.md "Account table").
// Plain C++ without HIP, so tests/accounts_finish_driver.cpp builds it under the sanitizers.
// addrs: n x 20 bytes in record order.  pred[i] = 1 + the closest j < i with the same address, or 0; succ[i] = 1 if some j > i has the same address, else 0.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <unordered_map>

namespace zk {

struct AcctAddrHash {
  size_t operator()(const std::array<uint8_t, 20> &a) const { uint64_t h = 0xcbf29ce484222325ull; for (uint8_t b : a) h = (h ^ b) * 0x100000001b3ull; return (size_t)h; }
};
inline void acct_pred_host(const uint8_t *addrs, size_t n, uint32_t *pred, uint32_t *succ) {
  std::unordered_map<std::array<uint8_t, 20>, uint32_t, AcctAddrHash> last;   // address -> 1 + its latest record so far
  last.reserve(n);
  for (size_t i = 0; i < n; i++) {
    std::array<uint8_t, 20> a; memcpy(a.data(), addrs + 20 * i, 20);
    uint32_t &l = last[a]; pred[i] = l; succ[i] = 0;
    if (l) succ[l - 1] = 1;
    l = (uint32_t)i + 1;
  }
}

}  // namespace zk
