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
