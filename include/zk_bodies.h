/* Optional extension of the drop-in surface: a stretch of the chain decided from nothing but the bytes of its block bodies.
 *
 * zkTxSenders (zk_txs.h) leaves three things with the node between a body's bytes and verifyChainAccounts (zk_accounts_chain.h): copying each transaction's fields
 * into a 720-byte zk_block_record, the deposit's own signature rule, and the compaction of a body that mixes public transactions with ZK ones.  This header takes
 * them over.  zkTxRecords is zkTxSenders plus the records; verifyChainBodies is zkTxRecords, then verifyChainAccounts on the records it made.
 *
 * Transaction i is txs[off[i] .. off[i+1]), as in zk_txs.h; signer and chain_id are zkTxSenders'.
 *
 * status[i], code[i], txhash[i] and froms[i] are exactly what zkTxSenders writes, for every code other than 3.  For code 3 (DepositTx, core/types/transaction.go:43)
 * a decoded transaction is ZK_TX_OK only where the reference's ApplyTransaction (core/state_processor.go:141-146; the pool makes the same check,
 * core/tx_pool.go:578-586) would go on to the proof, and ZK_TX_DEPOSIT_KEY otherwise:
 *   - addr1 = ExtractPKBAddress(HomesteadSigner{}, tx) (state_processor.go:141): recoverPlain over HomesteadSigner's hash — the six-field hash, never the nine-field
 *     one, whatever signer the block has (core/types/transaction_signing.go:96-113, :206-208, :231-240) — with the transaction's raw V, R, S and homestead = true:
 *       V has BitLen() > 8 (:247), or V - 27 is not 0 or 1 (:250 with crypto/crypto.go:209, ValidateSignatureValues' v == 0 || v == 1): refused.  A protected V such as 37 is refused:
 *         HomesteadSigner does no chain-id arithmetic;
 *       R or S longer than 32 bytes (:255-258), or refused by ValidateSignatureValues(V, R, S, true) — zero, not below N, s above N / 2 — also under
 *         ZK_SIGNER_FRONTIER (:251 with crypto.go:199-210, :205 for s): refused;
 *       the recovery fails (:261-267): refused.
 *   - addr2 = crypto.PubkeyToAddress({X, Y}) = Keccak256(pad32(X) || pad32(Y))[12:] (crypto/crypto.go:212-215 over FromECDSAPub's elliptic.Marshal, :136-141).  X or Y longer
 *     than 32 bytes: refused.  This is NOT verbatim: the reference's elliptic.Marshal slices out of range there and the node dies; as elsewhere in this library, an
 *     input that a reference node cannot handle is rejected.  No curve check is made on (X, Y): the reference makes none.
 *   - addr1 != addr2 (state_processor.go:144): refused.
 * froms[i] of an accepted deposit stays ZKAdrress (transaction_signing.go:72-76); addr1 is the pk of VerifyDepositProof (zktx/zktx.go:180-182) and goes into the record.
 * A refused deposit has no record, a zero froms, and the txhash zkTxSenders writes.
 *
 * A record is made for every transaction with status ZK_TX_OK and code 1 (mint), 2 (send), 3 (deposit) or 5 (redeem) — the codes with a ZK branch in ApplyTransaction
 * (state_processor.go:108-164); code 0, code 4 and every code above 5 have none.  Records are in transaction order and compacted: rec_of[i] is the index of
 * transaction i's record or -1, and rec_froms[j] is froms of record j's transaction — the two arrays verifyChainAccounts takes, recs and froms, without a pass over
 * them.  All 720 bytes of a record are defined (zk_proof_cache.h hashes them all): reserved is zero, unused args entries are zero, the twelve bytes behind pk are
 * zero, and the old slot is zero — the account table fills it (zk_accounts.h).  The fields, in the order in which zktx.go:122-210 marshals them into zk_verify_item:
 *
 *   code              kind              value_s   args[0]  args[1]          args[2]   args[3]  args[4]  args[5]
 *   1 mint, 5 redeem  ZK_KIND_MINT /    ZKValue   0 (old)  ZKSN             ZKCMT                                  (zktx.go:122-133, :198-210; state_processor.go:113, :158)
 *                     ZK_KIND_REDEEM
 *   2 send            ZK_KIND_SEND      0         0 (old)  ZKSN             ZKCMTS    ZKCMT                        (zktx.go:148-160; state_processor.go:124)
 *   3 deposit         ZK_KIND_DEPOSIT   0         RTcmt    addr1, 20 bytes  0 (old)   ZKSN     ZKCMT    ZKSNS      (zktx.go:180-194; state_processor.go:147)
 *
 * proof: the first 512 bytes of ZKProof where it has at least 512 (verify* reads only those), otherwise its bytes followed by zero bytes; a zero byte is no hex
 * digit, so such a record is rejected by the proof step.
 *
 * Not here: records handed to the chain call without the trip through recs; DepositTxV/R/S (no reference code path reads them
 * on import); a pool form; a miner's drop-and-go-on; nonce, balance and gas rules of public transactions; any change to the recovery or to verifyChainAccounts.  (A
 * body's outer list: zk_raw_bodies.h.)
 *
 * May be called from any thread; calls are served one at a time.  Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_BODIES_H
#define ZK_BODIES_H
#include <stdint.h>
#include "zk_txs.h"
#include "zk_accounts_chain.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { ZK_TX_DEPOSIT_KEY = 4 };   /* beside ZK_TX_OK .. ZK_TX_SIG of zk_txs.h: a deposit (code 3) whose signature does not recover the address of its (X, Y) */

/* recs, rec_froms, rec_of: room for n each; txhash may be NULL.  Returns m, the number of records: recs[0 .. m) and rec_froms[0 .. m) are written, rec_froms[m .. n)
 * is zeroed and recs[m .. n) is left as it was.  -1, with every output zeroed (recs over all n), for whatever zkTxSenders refuses — n < 0, a null pointer with n > 0,
 * a decreasing off, an unknown signer, chain_id >= 2^62, no device, a failure of any step — and for a null recs, rec_froms or rec_of with n > 0.  The arguments are
 * checked before the device is asked for.  n = 0 returns 0 and queues nothing. */
int zkTxRecords(const uint8_t *txs, const uint64_t *off, int n, int signer, uint64_t chain_id, zk_block_record *recs /* room for n */, uint8_t (*rec_froms)[20] /* room for n */,
                int32_t *rec_of /* n */, uint8_t (*txhash)[32] /* n, may be NULL */, uint8_t (*froms)[20] /* n */, uint8_t *code, uint8_t *status);

/* block_first: n_blocks + 1 entries over TRANSACTIONS, from 0 to n, not decreasing.  One signer serves a call: a caller splits a segment at a fork height.
 * The call decides exactly what these steps decide:
 *   1. zkTxRecords on all n transactions: recs, rec_froms, rec_of, txhash, froms, code, status and *n_recs = m are its outputs.
 *   2. B0: the first block that holds a transaction with status != ZK_TX_OK; n_blocks where there is none.
 *   3. verifyChainAccounts on the records of blocks [0, B0), its block_first the number of records before each block border; the result is k <= B0.  A block with no
 *      ZK transaction is an empty block there.
 *   4. Returns k; the table, the set and the tree are in the state after block k - 1.  ok (room for n), anchor_of (room for n, or NULL), the filled old slots of recs
 *      and accts_sizes, set_sizes, tree_sizes (n_blocks entries each, any may be NULL) are verifyChainAccounts' for the records and blocks it saw.  The records of the
 *      blocks from B0 on are not decided: ok = 0, anchor_of = -1, old slots zero; the sizes of those blocks are the sizes the call leaves.
 * Why block k failed, for k < n_blocks: status of its transactions if k == B0, ok of its records (rec_of leads from a transaction to its record) otherwise.
 *   5. -1, with every output of step 1 zeroed, every ok = 0, every anchor_of = -1, *n_recs = 0 and the three states as they were: whatever either part refuses — a
 *      null ok with n > 0, a null n_recs — and a block_first that does not run from 0 to n over the transactions.  Every argument of both parts that can be checked
 *      without the records is checked before anything is queued or written; "the sends do not fit into the tree" and "no room in the table's log" are found by
 *      verifyChainAccounts, before it writes.  The sizes arrays are not written then, with the one exception zk_accounts_chain.h names.
 * In this version the records make one trip through the caller's recs between the two parts. */
int verifyChainBodies(zk_proof_cache *cache, const uint8_t *txs, const uint64_t *off, int n, const int *block_first, int n_blocks, int signer, uint64_t chain_id, zk_accts *accts,
                      zk_tree *tree, const long long *prior_anchors, int n_prior, int window, zk_snset *set, zk_block_record *recs, uint8_t (*rec_froms)[20], int32_t *rec_of,
                      uint8_t (*txhash)[32], uint8_t (*froms)[20], uint8_t *code, uint8_t *status, unsigned char *ok /* per record */, int32_t *anchor_of /* per record, may be NULL */,
                      long long *accts_sizes, long long *set_sizes, long long *tree_sizes, int *n_recs);

#ifdef __cplusplus
}
#endif
#endif
