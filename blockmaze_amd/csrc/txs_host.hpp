// What the units of the transaction calls share (gpu_txs.hip, gpu_senders.hip, capi_txs.cpp, capi_bodies.cpp, capi_tx_roots.cpp, capi_headers.cpp): the argument structs and the
// prototypes of the functions they export to each other, and the two pieces every C entry of them starts with.  The workspace layouts: txs_layout.hpp.
#pragma once
#include <cstdint>
#include <mutex>
#include <string>
#include "../../include/zkgpu.h"
#include "../../include/zk_records.h"
#include "../../include/zk_txs.h"
#include "../../include/zk_headers.h"
#include "../../include/zk_raw_bodies.h"
#include "gpu.hpp"
#include "txs_layout.hpp"

extern std::mutex g_gpu_mutex;
extern void zkgpu_set_error(const std::string &s);

namespace zk {
// n transactions: txs[off[i] .. off[i+1]) under a signer and a chain id (include/zk_txs.h)
struct TxsIn { const uint8_t *txs; const uint64_t *off; size_t n; int signer; uint64_t chain_id; };
// zkTxSigningInputs' outputs; zkTxSenders leaves sighash and sigs null, and froms is deposit_from (may be null) or froms
struct SenderInputsOut { uint8_t *txhash, *sighash, *sigs, *froms, *code, *status; };
// zkTxRecords' outputs (include/zk_bodies.h), room for n each; txhash may be null
struct BodyOut { zk_block_record *recs; uint8_t *rec_froms; int32_t *rec_of; uint8_t *txhash, *froms, *code, *status; };
// the trie roots of n_lists lists: first, n_lists + 1 entries from 0 to n; roots 32 bytes a list; defined a byte a list (null for zkgpu_list_trie_roots)
struct RootsRequest { const int *first; size_t n_lists; uint8_t *roots, *defined; };

// zkHeaders (include/zk_headers.h): n headers, hdrs[off[i] .. off[i+1]), the engine's two numbers, the clock, the parent of header 0; the outputs, room for n each
struct HeadersIn { const uint8_t *hdrs; const uint64_t *off; size_t n; uint64_t period, epoch, now; int have_parent; const uint8_t *parent_hash; uint64_t parent_number, parent_time; };
struct HeadersOut { uint8_t *hash, *sealhash, *signer, *coinbase, *tx_root, *rtcmt; uint64_t *number, *time; uint8_t *difficulty, *vote; uint32_t *extra_beg, *extra_size, *cmt_beg, *cmt_count; uint8_t *status; };

// gpu_txs.hip.  The caller has checked the arguments and holds the device mutex.
size_t tx_sender_inputs(const TxsIn &in, bool want_senders, const SenderInputsOut &o);
size_t tx_records(const TxsIn &in, const BodyOut &o, size_t *first_bad, const int *borders, size_t n_borders, int *rec_borders, const RootsRequest *roots);
size_t headers_decide(const HeadersIn &in, const HeadersOut &o);
size_t trie_roots(const uint8_t *vals, const uint64_t *off, size_t n, const RootsRequest &rq, bool want_tx);
// zkBodySplit and verifyChainRawBodies (include/zk_raw_bodies.h): n_blocks > 0 bodies, bodies[body_off[b] .. body_off[b+1]); tx_beg and tx_size have room for cap,
// block_first for n_blocks + 1, body_status for n_blocks.  What the split found: n transactions, k leading bodies that are OK, the packed bytes; fits: n <= cap —
// without it block_first and body_status alone are written (body_split) or nothing at all (raw_records), and nothing else is queued.
struct RawBodiesIn { const uint8_t *bodies; const uint64_t *body_off; size_t n_blocks, cap; };
struct RawBodiesOut { uint64_t *tx_beg; uint32_t *tx_size; int *block_first; uint8_t *body_status; };
struct RawSplit { size_t n, k, total; bool fits; };
// packed (may be null; the test entry): the packed bytes, room for body_off[n_blocks] - body_off[0], and packed_off, cap + 1 values
RawSplit body_split(const RawBodiesIn &in, const RawBodiesOut &o, uint8_t *packed, uint64_t *packed_off);
// the split, then tx_records on what it packed with the blocks' roots (roots, defined: n_blocks each); rec_borders: n_blocks + 1; *m: the records
RawSplit raw_records(const RawBodiesIn &in, const RawBodiesOut &o, int signer, uint64_t chain_id, const BodyOut &bo, size_t *first_bad, int *rec_borders, uint8_t *roots, uint8_t *defined, size_t *m);
// capi_bodies.cpp: the chain call on the bodies' bytes in its three forms.  raw (verifyChainRawBodies; null for the other two): the bodies as they were delivered and
// what the split leaves; n is then the caller's cap, and txs, off and block_first are null.
struct RawChain { const uint8_t *bodies; const uint64_t *body_off; int cap; uint64_t *tx_beg; uint32_t *tx_size; int *block_first; uint8_t *body_status; int *n_txs; };
int chain_bodies(const char *name, bool with_roots, zk_proof_cache *cache, const uint8_t *txs, const uint64_t *off, int n, const int *block_first, int n_blocks, int signer, uint64_t chain_id,
                 zk_accts *accts, zk_tree *tree, const long long *prior_anchors, int n_prior, int window, zk_snset *set, zk_block_record *recs, uint8_t (*rec_froms)[20], int32_t *rec_of,
                 uint8_t (*txhash)[32], uint8_t (*froms)[20], uint8_t *code, uint8_t *status, unsigned char *ok, int32_t *anchor_of, long long *accts_sizes, long long *set_sizes,
                 long long *tree_sizes, int *n_recs, const uint8_t (*want_roots)[32], uint8_t (*roots)[32], unsigned char *root_ok, const RawChain *raw);
void probe_keccak256(const uint8_t *msgs, const uint64_t *off, size_t n, uint8_t *out);
void tx_records_gather_bytewise(bool on);
// gpu_senders.hip
size_t recover_senders_out_words(size_t n);
#ifdef __HIP__                                           // (the HIP units, which have the runtime's header before this one)
void recover_senders_queue(const uint32_t *hash, const uint32_t *rs, const uint8_t *v, size_t n, bool homestead, uint32_t *out, hipStream_t s);
#endif
void senders_keep_head(const uint32_t *head);

// ---- the start of every C entry -----------------------------------------------------------------------------------------------------------------------------------
constexpr const char *NO_DEVICE = "no HIP device visible; libzkgpu has no CPU fallback";
// fn runs under the device mutex; ZKGPU_ERR_NO_DEVICE without a device, ZKGPU_ERR_RUNTIME for whatever it throws
template <class Fn> int guarded_device(Fn fn) {
  try {
    if (!gpu_available()) { zkgpu_set_error(NO_DEVICE); return ZKGPU_ERR_NO_DEVICE; }
    std::lock_guard<std::mutex> lk(g_gpu_mutex); return fn();
  }
  catch (const std::exception &e) { zkgpu_set_error(e.what()); return ZKGPU_ERR_RUNTIME; }
  catch (...) { zkgpu_set_error("unknown error"); return ZKGPU_ERR_RUNTIME; }
}
// n < 0, a null pointer with n > 0 (outputs: the caller has every output it must have), an unknown signer, chain_id >= 2^62, a decreasing off; the error under the
// call's prefix, "txs" or "bodies"
inline bool txs_args_ok(const char *prefix, const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, bool outputs) {
  const char *why = nullptr;
  if (n < 0) why = ": a negative count";
  else if (n && (!txs || !off || !outputs)) why = ": a null pointer";
  else if (signer != ZK_SIGNER_FRONTIER && signer != ZK_SIGNER_HOMESTEAD && signer != ZK_SIGNER_EIP155) why = ": an unknown signer";
  else if (chain_id >> 62) why = ": a chain id of 2^62 or more";
  else for (int i = 0; i < n && !why; i++) if (off[i + 1] < off[i]) why = ": offsets decrease";
  if (why) zkgpu_set_error(std::string(prefix) + why);
  return !why;
}
}  // namespace zk
