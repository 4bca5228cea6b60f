// extern "C" surface of the records from the block bodies' bytes and of the chain call on them (include/zk_bodies.h, include/zkgpu.h "Records from the block
// bodies' bytes"): the arguments are checked here, before anything is queued; the device work is gpu_txs.hip's, the decision on the records is
// verifyChainAccounts'.  verifyChainBodiesRoots (include/zk_tx_roots.h) is the same call with the headers' transaction roots.  Every C++ exception ends
// at this boundary.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/zk_bodies.h"
#include "../../include/zk_tx_roots.h"
#include "txs_host.hpp"
using namespace zk;

namespace {
// every output as a failure leaves it: nothing is written through a null pointer or for a negative count
void bodies_zero(int n, const BodyOut &o) {
  if (n <= 0) return;
  if (o.recs) memset(o.recs, 0, sizeof(zk_block_record) * (size_t)n);
  if (o.rec_froms) memset(o.rec_froms, 0, 20 * (size_t)n);
  if (o.rec_of) memset(o.rec_of, 0, 4 * (size_t)n);
  if (o.txhash) memset(o.txhash, 0, 32 * (size_t)n);
  if (o.froms) memset(o.froms, 0, 20 * (size_t)n);
  if (o.code) memset(o.code, 0, (size_t)n);
  if (o.status) memset(o.status, 0, (size_t)n);
}
// zkTxSenders' refusals, and the three arrays of the records
bool bodies_args_ok(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, const BodyOut &o) {
  return txs_args_ok("bodies", txs, off, n, signer, chain_id, o.froms && o.code && o.status && o.recs && o.rec_froms && o.rec_of);
}
// what verifyChainRawBodies adds to the outputs, as a failure leaves it
void raw_zero(const RawChain &r, int n_blocks) {
  if (r.cap > 0) { if (r.tx_beg) memset(r.tx_beg, 0, 8 * (size_t)r.cap); if (r.tx_size) memset(r.tx_size, 0, 4 * (size_t)r.cap); }
  if (n_blocks >= 0 && r.block_first) memset(r.block_first, 0, 4 * ((size_t)n_blocks + 1));
  if (n_blocks > 0 && r.body_status) memset(r.body_status, 0, (size_t)n_blocks);
  if (r.n_txs) *r.n_txs = 0;
}
// the device part under the device mutex: m, or ZKGPU_ERR_NO_DEVICE / ZKGPU_ERR_RUNTIME with every output zeroed.  rq (may be null): the transaction trie roots of the
// blocks between the borders, and defined, on the same upload; zeroed by the caller on an error.  n = 0 with rq: every block is empty, the trie's finish launch alone.
int bodies_run(const TxsIn &in, const BodyOut &o, size_t *first_bad, const int *borders, size_t n_borders, int *rec_borders, const RootsRequest *rq = nullptr) {
  const int rc = guarded_device([&] {
    if (rq && !in.n) { trie_roots(in.txs, in.off, 0, *rq, true); return 0; }
    return (int)tx_records(in, o, first_bad, borders, n_borders, rec_borders, rq); });
  if (rc < 0) bodies_zero((int)in.n, o);                                                            // a step failed midway: nothing half-written stays
  return rc;
}
}  // namespace

extern "C" {
int zkgpu_tx_records(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, zk_block_record *recs, uint8_t *rec_froms, int32_t *rec_of, uint8_t *txhash,
                     uint8_t *froms, uint8_t *code, uint8_t *status) {
  const BodyOut o = {recs, rec_froms, rec_of, txhash, froms, code, status};
  if (!bodies_args_ok(txs, off, n, signer, chain_id, o)) { bodies_zero(n, o); return ZKGPU_ERR_ARG; }   // (before the device is asked for)
  if (n == 0) return 0;
  return bodies_run(TxsIn{txs, off, (size_t)n, signer, chain_id}, o, nullptr, nullptr, 0, nullptr);
}
int zkTxRecords(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, zk_block_record *recs, uint8_t (*rec_froms)[20], int32_t *rec_of, uint8_t (*txhash)[32],
                uint8_t (*froms)[20], uint8_t *code, uint8_t *status) {
  const int rc = zkgpu_tx_records(txs, off, n, signer, chain_id, recs, (uint8_t *)rec_froms, rec_of, (uint8_t *)txhash, (uint8_t *)froms, code, status);
  if (rc < 0) { fprintf(stderr, "libzkgpu: zkTxRecords: %s\n", zkgpu_last_error()); return -1; }
  return rc;
}
int zkgpu_test_bodies_gather(int bytewise) { std::lock_guard<std::mutex> lk(g_gpu_mutex); tx_records_gather_bytewise(bytewise != 0); return ZKGPU_OK; }

}  // extern "C"

// verifyChainBodies (with_roots false: the three last arguments are null and nothing of them is looked at), verifyChainBodiesRoots, and verifyChainRawBodies
// (include/zk_raw_bodies.h; capi_raw_bodies.cpp): with raw, txs, off and block_first are null and n is the caller's cap until step 1 has found the transactions
int zk::chain_bodies(const char *name, bool with_roots, zk_proof_cache *cache, const uint8_t *txs, const uint64_t *off, int n, const int *block_first, int n_blocks, int signer, uint64_t chain_id,
                        zk_accts *accts, zk_tree *tree, const long long *prior_anchors, int n_prior, int window, zk_snset *set, zk_block_record *recs, uint8_t (*rec_froms)[20], int32_t *rec_of,
                        uint8_t (*txhash)[32], uint8_t (*froms)[20], uint8_t *code, uint8_t *status, unsigned char *ok, int32_t *anchor_of, long long *accts_sizes, long long *set_sizes,
                        long long *tree_sizes, int *n_recs, const uint8_t (*want_roots)[32], uint8_t (*roots)[32], unsigned char *root_ok, const RawChain *raw) {
  const BodyOut o = {recs, (uint8_t *)rec_froms, rec_of, (uint8_t *)txhash, (uint8_t *)froms, code, status};
  // every output zeroed; anchor_of: -1, "no anchor", as verifyChainAccounts leaves it.  The sizes arrays are not written: verifyChainAccounts may have reported the
  // sizes after an impossible rewind in their last entries (zk_accounts_chain.h).
  auto fail = [&](const std::string &why) {
    zkgpu_set_error(why); fprintf(stderr, "libzkgpu: %s: %s\n", name, why.c_str());
    bodies_zero(n, o);
    if (with_roots && n_blocks > 0) { if (roots) memset(roots, 0, 32 * (size_t)n_blocks); if (root_ok) memset(root_ok, 0, (size_t)n_blocks); }
    for (int i = 0; i < n; i++) { if (ok) ok[i] = 0; if (anchor_of) anchor_of[i] = -1; }
    if (n_recs) *n_recs = 0;
    if (raw) raw_zero(*raw, n_blocks);
    return -1; };
  try {
    // 0. the arguments of both parts — verifyChainAccounts looks at its own again — before anything is queued or written
    if (raw) {
      if (n < 0) { n = 0; return fail("raw bodies: a negative cap"); }
      if (!raw->n_txs || (n_blocks >= 0 && !raw->block_first) || (n_blocks > 0 && !raw->body_status) || (n && (!raw->tx_beg || !raw->tx_size))) return fail("raw bodies: a null pointer");
      if (!txs_args_ok("raw bodies", raw->bodies, raw->body_off, n_blocks, signer, chain_id, true)) return fail(zkgpu_last_error());
      if (n && !(o.froms && o.code && o.status && o.recs && o.rec_froms && o.rec_of)) return fail("raw bodies: a null pointer");
    }
    else if (!bodies_args_ok(txs, off, n, signer, chain_id, o)) return fail(zkgpu_last_error());
    if (n_blocks < 0 || (n && !ok) || !n_recs) return fail("a negative count or a null pointer");
    if (!tree) return fail("no tree");
    if (!accts) return fail("no account table");
    if (!raw) {
      if (!block_first || block_first[0] != 0 || block_first[n_blocks] != n) return fail("block_first does not run from 0 to n");
      for (int b = 0; b < n_blocks; b++) if (block_first[b] > block_first[b + 1]) return fail("block_first decreases at block " + std::to_string(b));
    }
    if (n_prior < 0 || (n_prior && !prior_anchors)) return fail("a negative number of prior anchors or a null pointer");
    if (window < 0) return fail("a negative window");
    if (with_roots && n_blocks > 0 && (!want_roots || !roots || !root_ok)) return fail("a null pointer for the roots");
    if (with_roots && n_blocks > 0 && !raw && !off) return fail("a null pointer");                         // (the roots of empty blocks still go through the upload: off[0] is read)
    if (!gpu_available()) return fail(NO_DEVICE);
    uint64_t tree_before = 0; if (zkgpu_tree_size((zkgpu_tree *)tree, &tree_before) != ZKGPU_OK) return fail(zkgpu_last_error());
    for (int a = 0; a < n_prior; a++) if (prior_anchors[a] < 0 || (uint64_t)prior_anchors[a] > tree_before) return fail("prior anchor " + std::to_string(a) + " is negative or above the tree's size");
    // 1. zkTxRecords on all n transactions; the records before each block border from the prefix values the device left
    std::vector<int> rec_first((size_t)n_blocks + 1, 0); size_t first_bad = 0; int m = 0;
    //    (with the roots: DeriveSha of every block on the same upload, a block of no transactions included)
    //    (raw: the split first, which says what n and block_first are; more transactions than the caller has room for end the call before anything else is written)
    if (raw) {
      RawSplit found = {0, 0, 0, true}; const int cap = n; size_t mm = 0; n = 0;
      if (n_blocks) { const int rc = guarded_device([&] {
          found = raw_records(RawBodiesIn{raw->bodies, raw->body_off, (size_t)n_blocks, (size_t)cap}, RawBodiesOut{raw->tx_beg, raw->tx_size, raw->block_first, raw->body_status}, signer, chain_id, o,
                              &first_bad, rec_first.data(), (uint8_t *)roots, root_ok, &mm);
          return 0; });
        if (rc < 0) { n = cap; return fail(zkgpu_last_error()); }
        if (!found.fits) { *raw->n_txs = (int)found.n; return -2; } }
      else raw->block_first[0] = 0;
      n = (int)found.n; m = (int)mm; block_first = raw->block_first; *raw->n_txs = n;
      for (int b = 0; b < n_blocks; b++) if (raw->body_status[b] != ZK_BODY_OK) { memset(roots[b], 0, 32); root_ok[b] = 0; }   // no root: the body does not decode, or the block is refused whole
    }
    const RootsRequest rq = {block_first, (size_t)n_blocks, (uint8_t *)roots, root_ok};
    if (!raw && (n || (with_roots && n_blocks))) { m = bodies_run(TxsIn{txs, off, (size_t)n, signer, chain_id}, o, &first_bad, block_first, (size_t)n_blocks + 1, rec_first.data(), with_roots ? &rq : nullptr);
      if (m < 0) return fail(zkgpu_last_error()); }
    // 2. B0: the first block that holds a transaction with status != ZK_TX_OK — or, with the roots, whose root is undefined or is not the header's (root_ok holds
    //    "defined" here and "defined and equal" from here on; a raw body that is not ZK_BODY_OK has root_ok = 0 already)
    int B0 = n_blocks;
    if (n && first_bad < (size_t)n) { B0 = 0; while (B0 < n_blocks && (size_t)block_first[B0 + 1] <= first_bad) B0++; }
    if (with_roots) for (int b = n_blocks - 1; b >= 0; b--) { root_ok[b] = root_ok[b] && memcmp(roots[b], want_roots[b], 32) == 0; if (!root_ok[b] && b < B0) B0 = b; }
    // 3. verifyChainAccounts on the records of blocks [0, B0); a refusal there has left the three states alone
    const int n0 = rec_first[B0];
    const int k = verifyChainAccounts(cache, recs, (const uint8_t (*)[20])rec_froms, n0, rec_first.data(), B0, accts, tree, prior_anchors, n_prior, window, set, ok, anchor_of, accts_sizes, set_sizes, tree_sizes);
    if (k < 0) return fail(zkgpu_last_error());
    // 4. from B0 on nothing is decided, and the sizes are the ones the call leaves
    for (int j = n0; j < m; j++) { ok[j] = 0; if (anchor_of) anchor_of[j] = -1; }
    if (B0 < n_blocks) {
      long long a_now = B0 && accts_sizes ? accts_sizes[B0 - 1] : zkAcctsSize(accts), s_now = B0 && set_sizes ? set_sizes[B0 - 1] : (set ? zkSnSetSize(set) : 0), t_now = B0 && tree_sizes ? tree_sizes[B0 - 1] : 0;
      if (!(B0 && tree_sizes)) { uint64_t t = 0; if (zkgpu_tree_size((zkgpu_tree *)tree, &t) != ZKGPU_OK) t = tree_before; t_now = (long long)t; }
      for (int b = B0; b < n_blocks; b++) { if (accts_sizes) accts_sizes[b] = a_now; if (set && set_sizes) set_sizes[b] = s_now; if (tree_sizes) tree_sizes[b] = t_now; }
    }
    *n_recs = m;
    return k;
  }
  catch (const std::exception &e) { return fail(e.what()); }
  catch (...) { return fail("unknown error"); }
}

extern "C" {
int verifyChainBodies(zk_proof_cache *cache, const uint8_t *txs, const uint64_t *off, int n, const int *block_first, int n_blocks, int signer, uint64_t chain_id, zk_accts *accts,
                      zk_tree *tree, const long long *prior_anchors, int n_prior, int window, zk_snset *set, zk_block_record *recs, uint8_t (*rec_froms)[20], int32_t *rec_of,
                      uint8_t (*txhash)[32], uint8_t (*froms)[20], uint8_t *code, uint8_t *status, unsigned char *ok, int32_t *anchor_of, long long *accts_sizes, long long *set_sizes,
                      long long *tree_sizes, int *n_recs) {
  return zk::chain_bodies("verifyChainBodies", false, cache, txs, off, n, block_first, n_blocks, signer, chain_id, accts, tree, prior_anchors, n_prior, window, set, recs, rec_froms, rec_of, txhash, froms,
                      code, status, ok, anchor_of, accts_sizes, set_sizes, tree_sizes, n_recs, nullptr, nullptr, nullptr, nullptr);
}
int verifyChainBodiesRoots(zk_proof_cache *cache, const uint8_t *txs, const uint64_t *off, int n, const int *block_first, int n_blocks, int signer, uint64_t chain_id, zk_accts *accts,
                           zk_tree *tree, const long long *prior_anchors, int n_prior, int window, zk_snset *set, zk_block_record *recs, uint8_t (*rec_froms)[20], int32_t *rec_of,
                           uint8_t (*txhash)[32], uint8_t (*froms)[20], uint8_t *code, uint8_t *status, unsigned char *ok, int32_t *anchor_of, long long *accts_sizes, long long *set_sizes,
                           long long *tree_sizes, int *n_recs, const uint8_t (*want_roots)[32], uint8_t (*roots)[32], unsigned char *root_ok) {
  return zk::chain_bodies("verifyChainBodiesRoots", true, cache, txs, off, n, block_first, n_blocks, signer, chain_id, accts, tree, prior_anchors, n_prior, window, set, recs, rec_froms, rec_of, txhash,
                      froms, code, status, ok, anchor_of, accts_sizes, set_sizes, tree_sizes, n_recs, want_roots, roots, root_ok, nullptr);
}
}  // extern "C"
