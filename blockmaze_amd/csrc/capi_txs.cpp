// extern "C" surface of the sender inputs from raw transactions (include/zk_txs.h, include/zkgpu.h "Sender inputs from raw transactions"): the arguments are checked
// here, before anything is queued; the device work is gpu_txs.hip's.  Every C++ exception ends at this boundary.
#include <cstdio>
#include <cstring>
#include "txs_host.hpp"
using namespace zk;

// every output as a failure leaves it: nothing is written through a null pointer or for a negative count
static void txs_zero(int n, const SenderInputsOut &o) {
  if (n <= 0) return;
  if (o.txhash) memset(o.txhash, 0, 32 * (size_t)n);
  if (o.sighash) memset(o.sighash, 0, 32 * (size_t)n);
  if (o.sigs) memset(o.sigs, 0, 65 * (size_t)n);
  if (o.froms) memset(o.froms, 0, 20 * (size_t)n);
  if (o.code) memset(o.code, 0, (size_t)n);
  if (o.status) memset(o.status, 0, (size_t)n);
}
// both calls: the outputs zeroed, the arguments checked (before the device is asked for), the device work; `outputs`: the caller has every output the call must have
static int txs_call(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, bool want_senders, const SenderInputsOut &o, bool outputs) {
  txs_zero(n, o);
  if (!txs_args_ok("txs", txs, off, n, signer, chain_id, outputs)) return ZKGPU_ERR_ARG;
  if (n == 0) return 0;
  const int rc = guarded_device([&] { return (int)tx_sender_inputs(TxsIn{txs, off, (size_t)n, signer, chain_id}, want_senders, o); });
  if (rc == ZKGPU_ERR_RUNTIME) txs_zero(n, o);                                                      // a step failed midway: nothing half-written stays
  return rc;
}

extern "C" {
int zkgpu_tx_signing_inputs(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, uint8_t *txhash, uint8_t *sighash, uint8_t *sigs, uint8_t *deposit_from,
                            uint8_t *code, uint8_t *status) {
  return txs_call(txs, off, n, signer, chain_id, false, SenderInputsOut{txhash, sighash, sigs, deposit_from, code, status}, txhash && sighash && sigs && code && status);
}
int zkgpu_tx_senders(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, uint8_t *txhash, uint8_t *froms, uint8_t *code, uint8_t *status) {
  return txs_call(txs, off, n, signer, chain_id, true, SenderInputsOut{txhash, nullptr, nullptr, froms, code, status}, froms && code && status);
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
  return guarded_device([&] { probe_keccak256(msgs, off, n, out); return ZKGPU_OK; });
}
}  // extern "C"
