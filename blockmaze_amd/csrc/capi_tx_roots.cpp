// extern "C" surface of the trie roots (include/zk_tx_roots.h, include/zkgpu.h "trie roots of many lists"): the arguments are checked here, before
// anything is queued; the device work is gpu_txs.hip's.  verifyChainBodiesRoots stands beside verifyChainBodies in capi_bodies.cpp.  Every C++ exception ends at this
// boundary.
#include <cstdio>
#include <cstring>
#include "../../include/zk_tx_roots.h"
#include "txs_host.hpp"
using namespace zk;

namespace {
// every output as a failure leaves it: nothing is written through a null pointer or for a negative count
void roots_zero(int n_lists, uint8_t *roots, uint8_t *defined) {
  if (n_lists <= 0) return;
  if (roots) memset(roots, 0, 32 * (size_t)n_lists);
  if (defined) memset(defined, 0, (size_t)n_lists);
}
// a negative count, a null pointer with n > 0 or n_lists > 0, a decreasing off, a first that does not run from 0 to n without decreasing; min_len: the least length
// of a value (32 for the generic entry: a shorter leaf would be embedded in its parent, trie/hasher.go:176-178; 0 for transactions, which the walk judges).  A
// value within 16 bytes of 2^32 is refused where lengths are looked at: the leaf's three headers would not fit the sponge's sixteen prefix bytes.
bool roots_args_ok(const uint8_t *vals, const uint64_t *off, int n, const int *first, int n_lists, bool outputs, uint64_t min_len) {
  if (n < 0 || n_lists < 0) { zkgpu_set_error("trie roots: a negative count"); return false; }
  if ((n || n_lists) && (!off || !first || !outputs || (n && !vals))) { zkgpu_set_error("trie roots: a null pointer"); return false; }
  for (int i = 0; i < n; i++) if (off[i + 1] < off[i]) { zkgpu_set_error("trie roots: offsets decrease"); return false; }
  if (first && (first[0] != 0 || first[n_lists] != n)) { zkgpu_set_error("trie roots: first does not run from 0 to n"); return false; }
  for (int b = 0; b < n_lists; b++) if (first[b] > first[b + 1]) { zkgpu_set_error("trie roots: first decreases at list " + std::to_string(b)); return false; }
  if (min_len) for (int i = 0; i < n; i++) { const uint64_t len = off[i + 1] - off[i];   // (a transaction that long leaves its block without a root: k_trie_leaf)
    if (len < min_len) { zkgpu_set_error("trie roots: value " + std::to_string(i) + " has under 32 bytes: its leaf could be embedded in its parent, which the device does not do"); return false; }
    if (len > 0xFFFFFFFFull - 16) { zkgpu_set_error("trie roots: value " + std::to_string(i) + " has 2^32 - 16 bytes or more"); return false; } }
  return true;
}
// the device part under the device mutex: the number of defined roots, or ZKGPU_ERR_NO_DEVICE / ZKGPU_ERR_RUNTIME with both outputs zeroed
int roots_run(const uint8_t *vals, const uint64_t *off, int n, const int *first, int n_lists, bool want_tx, uint8_t *roots, uint8_t *defined) {
  const int rc = guarded_device([&] { return (int)trie_roots(vals, off, (size_t)n, RootsRequest{first, (size_t)n_lists, roots, defined}, want_tx); });
  if (rc < 0) roots_zero(n_lists, roots, defined);                                                  // a step failed midway: nothing half-written stays
  return rc;
}
}  // namespace

extern "C" {
int zkgpu_list_trie_roots(const uint8_t *vals, const uint64_t *off, int n, const int *first, int n_lists, uint8_t *roots) {
  if (!roots_args_ok(vals, off, n, first, n_lists, roots != nullptr, 32)) { roots_zero(n_lists, roots, nullptr); return ZKGPU_ERR_ARG; }   // (before the device is asked for)
  if (n_lists == 0) return ZKGPU_OK;
  const int rc = roots_run(vals, off, n, first, n_lists, false, roots, nullptr);
  return rc < 0 ? rc : ZKGPU_OK;
}
int zkgpu_tx_roots(const uint8_t *txs, const uint64_t *off, int n, const int *block_first, int n_blocks, uint8_t *roots, uint8_t *defined) {
  if (!roots_args_ok(txs, off, n, block_first, n_blocks, roots && defined, 0)) { roots_zero(n_blocks, roots, defined); return ZKGPU_ERR_ARG; }
  if (n_blocks == 0) return 0;
  return roots_run(txs, off, n, block_first, n_blocks, true, roots, defined);
}
int zkTxRoots(const uint8_t *txs, const uint64_t *off, int n, const int *block_first, int n_blocks, uint8_t (*roots)[32], unsigned char *defined) {
  const int rc = zkgpu_tx_roots(txs, off, n, block_first, n_blocks, (uint8_t *)roots, defined);
  if (rc < 0) { fprintf(stderr, "libzkgpu: zkTxRoots: %s\n", zkgpu_last_error()); return -1; }
  return rc;
}
}  // extern "C"
