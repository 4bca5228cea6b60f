// extern "C" surface of the sender inputs from raw transactions (include/zk_txs.h, include/zkgpu.h "Sender inputs from raw transactions"): the arguments are checked
// here, before anything is queued; the device work is gpu_txs.hip's.  Every C++ exception ends at this boundary.
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include "../../include/zkgpu.h"
#include "../../include/zk_txs.h"
#include "gpu.hpp"

extern std::mutex g_gpu_mutex;
extern void zkgpu_set_error(const std::string &s);
namespace zk {
size_t tx_sender_inputs(const uint8_t *txs, const uint64_t *off, size_t n, int signer, uint64_t chain_id, bool want_senders, uint8_t *txhash, uint8_t *sighash, uint8_t *sigs,
                        uint8_t *froms, uint8_t *code, uint8_t *status);
void probe_keccak256(const uint8_t *msgs, const uint64_t *off, size_t n, uint8_t *out);
}
using namespace zk;

static const char *const NO_DEVICE = "no HIP device visible; libzkgpu has no CPU fallback";
// fn runs under the device mutex; ZKGPU_ERR_NO_DEVICE without a device, ZKGPU_ERR_RUNTIME for whatever it throws
template <class Fn> static int guarded_txs(Fn fn) {
  try {
    if (!gpu_available()) { zkgpu_set_error(NO_DEVICE); return ZKGPU_ERR_NO_DEVICE; }
    std::lock_guard<std::mutex> lk(g_gpu_mutex); return fn();
  }
  catch (const std::exception &e) { zkgpu_set_error(e.what()); return ZKGPU_ERR_RUNTIME; }
  catch (...) { zkgpu_set_error("unknown error"); return ZKGPU_ERR_RUNTIME; }
}
// every output as a failure leaves it: nothing is written through a null pointer or for a negative count
static void txs_zero(int n, uint8_t *txhash, uint8_t *sighash, uint8_t *sigs, uint8_t *froms, uint8_t *code, uint8_t *status) {
  if (n <= 0) return;
  if (txhash) memset(txhash, 0, 32 * (size_t)n);
  if (sighash) memset(sighash, 0, 32 * (size_t)n);
  if (sigs) memset(sigs, 0, 65 * (size_t)n);
  if (froms) memset(froms, 0, 20 * (size_t)n);
  if (code) memset(code, 0, (size_t)n);
  if (status) memset(status, 0, (size_t)n);
}
// n < 0, a null pointer with n > 0 (the caller names the outputs it must have), a decreasing off, an unknown signer, chain_id >= 2^62
static bool txs_args_ok(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, bool outputs) {
  if (n < 0) { zkgpu_set_error("txs: a negative count"); return false; }
  if (n && (!txs || !off || !outputs)) { zkgpu_set_error("txs: a null pointer"); return false; }
  if (signer != ZK_SIGNER_FRONTIER && signer != ZK_SIGNER_HOMESTEAD && signer != ZK_SIGNER_EIP155) { zkgpu_set_error("txs: an unknown signer"); return false; }
  if (chain_id >> 62) { zkgpu_set_error("txs: a chain id of 2^62 or more"); return false; }
  for (int i = 0; i < n; i++) if (off[i + 1] < off[i]) { zkgpu_set_error("txs: offsets decrease"); return false; }
  return true;
}

extern "C" {
int zkgpu_tx_signing_inputs(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, uint8_t *txhash, uint8_t *sighash, uint8_t *sigs, uint8_t *deposit_from,
                            uint8_t *code, uint8_t *status) {
  txs_zero(n, txhash, sighash, sigs, deposit_from, code, status);
  if (!txs_args_ok(txs, off, n, signer, chain_id, txhash && sighash && sigs && code && status)) return ZKGPU_ERR_ARG;      // (before the device is asked for)
  if (n == 0) return 0;
  const int rc = guarded_txs([&] { return (int)tx_sender_inputs(txs, off, (size_t)n, signer, chain_id, false, txhash, sighash, sigs, deposit_from, code, status); });
  if (rc == ZKGPU_ERR_RUNTIME) txs_zero(n, txhash, sighash, sigs, deposit_from, code, status);            // a step failed midway: nothing half-written stays
  return rc;
}
int zkgpu_tx_senders(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, uint8_t *txhash, uint8_t *froms, uint8_t *code, uint8_t *status) {
  txs_zero(n, txhash, nullptr, nullptr, froms, code, status);
  if (!txs_args_ok(txs, off, n, signer, chain_id, froms && code && status)) return ZKGPU_ERR_ARG;
  if (n == 0) return 0;
  const int rc = guarded_txs([&] { return (int)tx_sender_inputs(txs, off, (size_t)n, signer, chain_id, true, txhash, nullptr, nullptr, froms, code, status); });
  if (rc == ZKGPU_ERR_RUNTIME) txs_zero(n, txhash, nullptr, nullptr, froms, code, status);
  return rc;
}
int zkTxSigningInputs(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, uint8_t (*txhash)[32], uint8_t (*sighash)[32], uint8_t (*sigs)[65],
                      uint8_t (*deposit_from)[20], uint8_t *code, uint8_t *status) {
  const int rc = zkgpu_tx_signing_inputs(txs, off, n, signer, chain_id, (uint8_t *)txhash, (uint8_t *)sighash, (uint8_t *)sigs, (uint8_t *)deposit_from, code, status);
  if (rc < 0) { fprintf(stderr, "libzkgpu: zkTxSigningInputs: %s\n", zkgpu_last_error()); return -1; }
  return rc;
}
int zkTxSenders(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, uint8_t (*txhash)[32], uint8_t (*froms)[20], uint8_t *code, uint8_t *status) {
  const int rc = zkgpu_tx_senders(txs, off, n, signer, chain_id, (uint8_t *)txhash, (uint8_t *)froms, code, status);
  if (rc < 0) { fprintf(stderr, "libzkgpu: zkTxSenders: %s\n", zkgpu_last_error()); return -1; }
  return rc;
}
int zkgpu_test_keccak256(const uint8_t *msgs, const uint64_t *off, size_t n, uint8_t *out) {
  return guarded_txs([&] { probe_keccak256(msgs, off, n, out); return ZKGPU_OK; });
}
}  // extern "C"
