/* Optional extension of the drop-in surface: what a sender recovery needs, from the raw transactions of a block body, in one call, on the device.
 *
 * zkRecoverSenders (zk_senders.h) takes a signing hash and a signature per transaction and leaves "the RLP hash" with the caller.  This header takes that over,
 * together with the rest of what the reference's types.Sender(signer, tx) does before recoverPlain (core/types/transaction_signing.go:72-94):
 *   - rlp.DecodeBytes into txdata (core/types/transaction.go:64-100; rlp/decode.go), with every rule of the strict decoder;
 *   - signer.Hash(tx) (transaction_signing.go:179-189 EIP155Signer's, :231-240 FrontierSigner's, which HomesteadSigner shares);
 *   - the chain-id arithmetic on V (:151-161; deriveChainId :274-284; isProtectedV transaction.go:165-172), then V := byte(Vb.Uint64() - 27) (:250);
 *   - tx.Hash(), the Keccak-256 of the transaction's encoding;
 *   - the fork's own rule for a deposit: Sender returns ZKAdrress and recovers no key (transaction_signing.go:72-76).
 * zkTxSenders goes on through the recovery of zk_senders.h without a trip to the host, and returns froms as verifyChainAccounts and verifyBlockAccounts
 * (zk_accounts_chain.h, zk_accounts.h) take it: an import is zkTxSenders, then verifyChainAccounts.
 *
 * Transaction i is txs[off[i] .. off[i+1]): one RLP list as it stands in a block body.  off has n + 1 non-decreasing entries.
 *
 * status[i] is the first rule that applies, in the reference's own order:
 *   ZK_TX_MALFORMED  rlp.DecodeBytes(tx, &txdata) would return an error (rlp/decode.go):
 *     - the outer item is a list (:438, :762) whose payload ends exactly at off[i+1] (:142-144 "more than one value", :886 "value larger than the input");
 *       an empty transaction, and one longer than 2^32 - 1 bytes (this library's own bound), are malformed;
 *     - txdata has 26 fields with an RLP encoding (transaction.go:64-96, Code to S; Hash is tagged "-"): fewer items (:443-444) and more (:449, :778) are errors;
 *     - size headers are canonical: the long form only from 56 up (:938, :957), no leading zero in a length (:980-985), no header byte and no element beyond
 *       the end of its list (:891, :1016-1034);
 *     - a one-byte string below 0x80 must be the byte itself (:662, :423, :726);
 *     - uint8 and uint64 fields (Code; AccountNonce, GasLimit, ZKValue, ZKNounce): a string of at most 1 or 8 bytes (:716), no leading zero (:721-723), the
 *       byte 0x00 refused (:710);
 *     - *big.Int fields (Price, Amount, X, Y, DepositTxV/R/S, V, R, S): a string with no leading zero byte (:271-287), the byte 0x00 included;
 *     - *common.Hash, common.Hash and *common.Address without a tag (ZKSN, ZKSNS, ZKCMT, ZKCMTS, RTcmt; ZKAdrress): a string of exactly 32 or 20 bytes (:395-430);
 *     - Recipient, tagged "nil": a string of 20 bytes, or an empty string or an empty list (0xC0), both of which mean nil (:486-496);
 *     - CMTBlock: a list (:324) of canonical uint64s (:338-365);
 *     - Payload, ZKProof, AUX: any string (:386-393).
 *   ZK_TX_CHAIN_ID   only under ZK_SIGNER_EIP155, only for code != 3, only for a protected V — V is not 27 or 28, or is wider than 8 bits (transaction.go:165-172):
 *     deriveChainId(V) != chain_id (transaction_signing.go:155-157), the id derived with the reference's uint64 arithmetic, the wrap below 35 included.  A V wider
 *     than 64 bits never matches a chain_id below 2^62.
 *   ZK_TX_SIG        only for code != 3: V, after the signer's subtraction (V - 2 chain_id - 8 for a protected V under EIP155, :158-159), has BitLen() > 8 (:247),
 *     or R or S is longer than 32 bytes (:255-258 copies them into 32-byte fields).  In zkTxSenders also whatever recoverPlain refuses: ok = 0 of zkRecoverSenders.
 * For a MALFORMED record every output is zero.
 *
 * txhash[i] is the Keccak-256 of the reference's re-encoding of the decoded transaction, which is what tx.Hash() returns.  The strict decoder makes the
 * re-encoding equal to the input bytes with one exception: a Recipient of 0xC0 re-encodes as 0x80.  The device hashes the input bytes with that one byte
 * substituted, in both hashes; nothing else is re-encoded.
 * sighash[i]: under ZK_SIGNER_EIP155 with a protected V, rlpHash([nonce, price, gas, to, value, payload, chain_id, 0, 0]) (:179-189); otherwise the six-field hash
 * (:231-240; an unprotected V under EIP155 takes Homestead's road, :152-154).  Fields 1 to 6 are consecutive items of the input: the message is a fresh list
 * header, their bytes as they stand, and for EIP155 the canonical encoding of chain_id followed by 0x80 0x80.
 *
 * Not here: the transaction trie root (DeriveSha); signing; DepositTxV/R/S; streaming a block body's outer list (the caller passes off); any change to the
 * recovery.  The records, a deposit's ExtractPKBAddress rule and a chain call that takes transactions are zk_bodies.h's.
 *
 * May be called from any thread; calls are served one at a time.  Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_TXS_H
#define ZK_TXS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { ZK_SIGNER_FRONTIER = 0, ZK_SIGNER_HOMESTEAD = 1, ZK_SIGNER_EIP155 = 2 };
enum { ZK_TX_OK = 0, ZK_TX_MALFORMED = 1, ZK_TX_CHAIN_ID = 2, ZK_TX_SIG = 3 };

/* code[i]: txdata.Code.  sigs[i]: R || S || V exactly as zkRecoverSenders takes them — R and S left-padded to 32 bytes, V = byte(v - 27) after the signer's
 * subtraction; all 65 bytes zero where status[i] != ZK_TX_OK.  For a deposit (code 3, always ZK_TX_OK once decoded) R and S are written where they have at most
 * 32 bytes and V's byte where no rule above would have refused V, zero otherwise: the reference never looks at them there.  deposit_from (may be NULL):
 * ZKAdrress for code 3, zero otherwise.
 * Returns the number of records with status ZK_TX_OK; -1, with every output zeroed, for n < 0, a null pointer with n > 0, a decreasing off, an unknown signer,
 * chain_id >= 2^62, no device, or a failure of any step.  The arguments are checked before the device is asked for.  n = 0 returns 0 and queues nothing. */
int zkTxSigningInputs(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, uint8_t (*txhash)[32], uint8_t (*sighash)[32], uint8_t (*sigs)[65],
                      uint8_t (*deposit_from)[20], uint8_t *code, uint8_t *status);

/* The same walk and hashes, then the recovery of zk_senders.h (homestead = signer != ZK_SIGNER_FRONTIER) on what they left on the device.  froms[i]: ZKAdrress for
 * code 3; the recovered address where status[i] == ZK_TX_OK; zero otherwise.  txhash may be NULL.  Returns and refuses as zkTxSigningInputs does. */
int zkTxSenders(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, uint8_t (*txhash)[32] /* may be NULL */, uint8_t (*froms)[20], uint8_t *code,
                uint8_t *status);

#ifdef __cplusplus
}
#endif
#endif
