// extern "C" surface of the block bodies from their bytes (include/zk_raw_bodies.h, include/zkgpu.h "block bodies from their bytes"): the arguments are
// checked here, before anything is queued; the device work is gpu_txs.hip's; the chain call is capi_bodies.cpp's chain_bodies in its raw form.  Every C++ exception ends
// at this boundary.
#include <cstdio>
#include <cstring>
#include "txs_host.hpp"
using namespace zk;

namespace {
struct SplitOut { uint64_t *tx_beg; uint32_t *tx_size; int *block_first; uint8_t *body_status; int *n_txs; uint8_t *packed; uint64_t *packed_off; };
// the per-transaction outputs as -2 and every failure leave them; nothing is written through a null pointer or for a negative count
void split_zero_txs(int cap, size_t packed_bytes, const SplitOut &o) {
  if (cap > 0) { if (o.tx_beg) memset(o.tx_beg, 0, 8 * (size_t)cap); if (o.tx_size) memset(o.tx_size, 0, 4 * (size_t)cap); }
  if (o.packed && packed_bytes) memset(o.packed, 0, packed_bytes);
  if (o.packed_off && cap >= 0) memset(o.packed_off, 0, 8 * ((size_t)cap + 1));
}
void split_zero(int n_blocks, int cap, size_t packed_bytes, const SplitOut &o) {
  split_zero_txs(cap, packed_bytes, o);
  if (o.block_first && n_blocks >= 0) memset(o.block_first, 0, 4 * ((size_t)n_blocks + 1));
  if (o.body_status && n_blocks > 0) memset(o.body_status, 0, (size_t)n_blocks);
  if (o.n_txs) *o.n_txs = 0;
}
// a negative count, a null pointer with n_blocks > 0 (tx_beg and tx_size only where cap > 0; n_txs and block_first always), a decreasing body_off
bool split_args_ok(const uint8_t *bodies, const uint64_t *body_off, int n_blocks, int cap, const SplitOut &o, bool test) {
  const char *why = nullptr;
  if (n_blocks < 0 || cap < 0) why = "raw bodies: a negative count";
  else if (!o.n_txs || !o.block_first || (n_blocks && (!bodies || !body_off || !o.body_status)) || (cap && (!o.tx_beg || !o.tx_size)) || (test && !o.packed_off)) why = "raw bodies: a null pointer";
  else for (int b = 0; b < n_blocks && !why; b++) if (body_off[b + 1] < body_off[b]) why = "raw bodies: offsets decrease";
  if (!why && test && n_blocks && body_off[n_blocks] > body_off[0] && !o.packed) why = "raw bodies: a null pointer";
  if (why) zkgpu_set_error(why);
  return !why;
}
int split_run(const uint8_t *bodies, const uint64_t *body_off, int n_blocks, int cap, const SplitOut &o, bool test) {
  if (!split_args_ok(bodies, body_off, n_blocks, cap, o, test)) { split_zero(n_blocks, cap, 0, o); return ZKGPU_ERR_ARG; }   // (before the device is asked for; packed's size is not known to be sane)
  const size_t packed_bytes = test && n_blocks ? (size_t)(body_off[n_blocks] - body_off[0]) : 0;
  if (n_blocks == 0) { split_zero(0, cap, 0, o); return 0; }
  RawSplit found = {0, 0, 0, true};
  const int rc = guarded_device([&] { found = body_split(RawBodiesIn{bodies, body_off, (size_t)n_blocks, (size_t)cap}, RawBodiesOut{o.tx_beg, o.tx_size, o.block_first, o.body_status}, o.packed,
                                                         o.packed_off); return 0; });
  if (rc < 0) { split_zero(n_blocks, cap, packed_bytes, o); return rc; }                            // a step failed midway: nothing half-written stays
  *o.n_txs = (int)found.n;
  if (!found.fits) { split_zero_txs(cap, packed_bytes, o); zkgpu_set_error("raw bodies: " + std::to_string(found.n) + " transactions, room for " + std::to_string(cap)); return ZKGPU_ERR_CAP; }
  return (int)found.k;
}
}  // namespace

extern "C" {
int zkgpu_body_split(const uint8_t *bodies, const uint64_t *body_off, int n_blocks, int cap, uint64_t *tx_beg, uint32_t *tx_size, int *block_first, uint8_t *body_status, int *n_txs) {
  return split_run(bodies, body_off, n_blocks, cap, SplitOut{tx_beg, tx_size, block_first, body_status, n_txs, nullptr, nullptr}, false);
}
int zkgpu_test_body_split(const uint8_t *bodies, const uint64_t *body_off, int n_blocks, int cap, uint64_t *tx_beg, uint32_t *tx_size, int *block_first, uint8_t *body_status, int *n_txs,
                          uint8_t *packed, uint64_t *packed_off) {
  return split_run(bodies, body_off, n_blocks, cap, SplitOut{tx_beg, tx_size, block_first, body_status, n_txs, packed, packed_off}, true);
}
int zkBodySplit(const uint8_t *bodies, const uint64_t *body_off, int n_blocks, int cap, uint64_t *tx_beg, uint32_t *tx_size, int *block_first, uint8_t *body_status, int *n_txs) {
  const int rc = zkgpu_body_split(bodies, body_off, n_blocks, cap, tx_beg, tx_size, block_first, body_status, n_txs);
  if (rc == ZKGPU_ERR_CAP) return -2;
  if (rc < 0) { fprintf(stderr, "libzkgpu: zkBodySplit: %s\n", zkgpu_last_error()); return -1; }
  return rc;
}
int verifyChainRawBodies(zk_proof_cache *cache, const uint8_t *bodies, const uint64_t *body_off, int n_blocks, int cap, int signer, uint64_t chain_id, zk_accts *accts, zk_tree *tree,
                         const long long *prior_anchors, int n_prior, int window, zk_snset *set, zk_block_record *recs, uint8_t (*rec_froms)[20], int32_t *rec_of, uint8_t (*txhash)[32],
                         uint8_t (*froms)[20], uint8_t *code, uint8_t *status, unsigned char *ok, int32_t *anchor_of, long long *accts_sizes, long long *set_sizes, long long *tree_sizes,
                         int *n_recs, const uint8_t (*want_roots)[32], uint8_t (*roots)[32], unsigned char *root_ok, uint64_t *tx_beg, uint32_t *tx_size, int *block_first,
                         uint8_t *body_status, int *n_txs) {
  const RawChain raw = {bodies, body_off, cap, tx_beg, tx_size, block_first, body_status, n_txs};
  return chain_bodies("verifyChainRawBodies", true, cache, nullptr, nullptr, cap, nullptr, n_blocks, signer, chain_id, accts, tree, prior_anchors, n_prior, window, set, recs, rec_froms, rec_of, txhash,
                      froms, code, status, ok, anchor_of, accts_sizes, set_sizes, tree_sizes, n_recs, want_roots, roots, root_ok, &raw);
}
}  // extern "C"
