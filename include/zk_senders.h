/* Optional extension of the drop-in surface: the senders of n transactions recovered from their signatures in one call, on the device (DESIGN.md "Senders from
 * signatures").
 *
 * verifyChainAccounts and verifyBlockAccounts (zk_accounts_chain.h, zk_accounts.h) take froms, one 20-byte sender per record, from the caller.  The reference never has
 * a sender at hand: it computes one per transaction, types.Sender(signer, tx) -> recoverPlain (core/types/transaction_signing.go:246-271) ->
 * crypto.ValidateSignatureValues (crypto/crypto.go:199-210) -> crypto.Ecrecover (crypto/signature_cgo.go:31) -> secp256k1_ecdsa_recover
 * (crypto/secp256k1/libsecp256k1/src/modules/recovery/main_impl.h:87-121) -> Keccak256(pub[1:])[12:], and spreads that over all cores (core/tx_cacher.go).
 * zkRecoverSenders decides n (signing hash, signature) pairs as recoverPlain decides them, one lane of the device per pair.
 *
 * froms is laid out as verifyChainAccounts and verifyBlockAccounts take it: the caller passes the array on, and treats any ok[i] == 0 as the reference treats an
 * error from Sender: the block is invalid.
 *
 * What stays with the caller:
 *   - the RLP hash itself: signer.Hash(tx) (transaction_signing.go:179-189 EIP155Signer.Hash, :231-240 FrontierSigner's, which HomesteadSigner shares);
 *   - the chain-id arithmetic on V: V = V - 2 chainId - 8 (transaction_signing.go:158-159), then V := byte(Vb.Uint64() - 27) (:250);
 *   - Vb.BitLen() > 8 (transaction_signing.go:247): a V that does not fit a byte is refused before the call;
 *   - an R or S longer than 32 bytes, which cannot be written into sigs[i] (transaction_signing.go:255-258 copies them into 32-byte fields): the caller rejects it
 *     before the call — ValidateSignatureValues would, since such a value is at or above N.
 *
 * Not here: the RLP hash; a chain call that takes signatures instead of froms; signing; VerifySignature (crypto/signature_cgo.go:66); the GLV endomorphism
 * (the walk is a plain interleaved 4-bit window walk); recovery ids 2 and 3 (x = r + N), which geth's V cannot express.
 *
 * May be called from any thread; calls are served one at a time.  Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_SENDERS_H
#define ZK_SENDERS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* sighash[i]: the 32 bytes the reference's signer.Hash(tx) returns.  sigs[i]: R (32 bytes, big-endian) || S (32) || V (1), V as recoverPlain holds it after
 * "V := byte(Vb.Uint64() - 27)", i.e. 0 or 1 for a signature that can be valid.  homestead: recoverPlain's flag (S above N/2 refused).
 * froms[i]: the sender, 20 bytes; all zero where ok[i] == 0.  pubs (may be NULL): X || Y, 64 bytes, of the recovered key; all zero where ok[i] == 0.
 * ok[i]: 1 exactly where recoverPlain returns an address without an error.  Returns the number of records with ok = 1;
 * -1 (every ok 0, every output zeroed) for n < 0, a null pointer with n > 0, no device, or a failure of any step.  n = 0 returns 0 and queues nothing. */
int zkRecoverSenders(const uint8_t (*sighash)[32], const uint8_t (*sigs)[65], int n, int homestead, uint8_t (*froms)[20], uint8_t (*pubs)[64], unsigned char *ok);

#ifdef __cplusplus
}
#endif
#endif
