// The host half of the account table's predecessor search (blockmaze_amd/csrc/acct_pred_host.hpp) as a program of its own, for the sanitizer build that
// tests/test_accounts_cpu.py makes: seeded batches — all addresses distinct, drawn from a few, all equal, and an empty one — against the plain O(n^2) search.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "acct_pred_host.hpp"

static uint64_t splitmix(uint64_t &s) { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

static int check(size_t n, uint64_t pool, uint64_t seed) {
  std::vector<uint8_t> addrs(20 * n + 1); std::vector<uint32_t> pred(n + 1, 0xDEADBEEFu), succ(n + 1, 0xDEADBEEFu); uint64_t s = seed;
  for (size_t i = 0; i < n; i++) { uint64_t who = pool ? splitmix(s) % pool : i, t = who * 0x100000001B3ull + seed; for (int b = 0; b < 20; b++) addrs[20 * i + b] = (uint8_t)(splitmix(t) >> 11); }
  zk::acct_pred_host(addrs.data(), n, pred.data(), succ.data());
  if (pred[n] != 0xDEADBEEFu || succ[n] != 0xDEADBEEFu) { printf("wrote past the end at n = %zu\n", n); return 1; }
  for (size_t i = 0; i < n; i++) {
    uint32_t want_pred = 0, want_succ = 0;
    for (size_t j = 0; j < n; j++) { if (j == i || memcmp(&addrs[20 * i], &addrs[20 * j], 20)) continue; if (j < i) want_pred = (uint32_t)j + 1; else want_succ = 1; }
    if (pred[i] != want_pred || succ[i] != want_succ) { printf("n = %zu pool = %llu record %zu: pred %u want %u, succ %u want %u\n", n, (unsigned long long)pool, i, pred[i], want_pred, succ[i], want_succ); return 1; }
  }
  return 0;
}

int main() {
  const size_t sizes[] = {0, 1, 2, 3, 63, 64, 65, 257, 1000, 3000};
  for (size_t n : sizes) for (uint64_t pool : {0ull, 1ull, 3ull, 40ull}) if (check(n, pool, 77 + n + pool)) return 1;
  printf("ACCOUNTS FINISH OK\n");
  return 0;
}
