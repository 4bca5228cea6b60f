/* Optional extension of the drop-in surface: the transaction trie roots of a segment's block bodies, on the device, and the chain call that holds them against the
 * headers' roots.
 *
 * verifyChainBodies (zk_bodies.h) decides a stretch of the chain from the bytes of its block bodies and never asks whether those are the bodies the headers name.
 * The reference ties a body to its header before any transaction is applied: eth/downloader/queue.go:772 holds a delivered body against header.TxHash, and
 * ValidateBody (core/block_validator.go:70) checks types.DeriveSha(block.Transactions()) != header.TxHash.  This header computes DeriveSha for every block of a
 * segment in one call, and gives the chain call a form that takes header.TxHash of each block.
 *
 * DeriveSha (core/types/derive_sha.go:32-41) is the root of a Merkle-Patricia trie, hashed with Keccak-256, that holds rlp(i) -> rlp(tx_i) for i = 0 .. n - 1:
 *   - the key of transaction i is rlp.Encode(uint(i)) (derive_sha.go:37): 0 -> 80; 1 .. 0x7f -> the byte itself; 0x80 .. 0xff -> 81 xx; 0x100 .. 0xffff -> 82 xx xx;
 *     0x10000 .. 0xffffff -> 83 xx xx xx; beyond -> 84 xx xx xx xx (rlp/encode.go: an integer is its big-endian bytes without leading zeros, as a string);
 *   - the value is rlp.EncodeToBytes(tx) (derive_sha.go:38, GetRlp): by zk_txs.h's "nothing is re-encoded" the input bytes of a transaction that decodes, a Recipient
 *     of 0xC0 read as 0x80 — the one byte the walk records and the hashes already substitute;
 *   - keys are walked as nibbles (trie/encoding.go keybytesToHex); a leaf is the two-item list [hexToCompact(the rest of the key, terminator set), value], an
 *     extension [hexToCompact(the shared nibbles), child], a branch a 17-item list of its sixteen children and a value slot (trie/node.go EncodeRLP, trie/trie.go
 *     insert :218-285);
 *   - a node whose encoding has at least 32 bytes is referenced by its Keccak-256, a shorter one is embedded in its parent (trie/hasher.go:176-178); the root is always
 *     hashed (force = true: trie.go hashRoot, hasher.go:77-119);
 *   - the root of no transactions is emptyRoot, 56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421 (trie/trie.go:32).
 * No key is a prefix of another (RLP is self-delimiting), so no branch carries a value.  Every value here has at least 32 bytes — a transaction that decodes holds
 * five 32-byte hashes — so a leaf has at least 35 bytes and every branch and extension holds a 33-byte reference: every node is referenced by hash, nothing is
 * embedded.
 *
 * A block that holds a ZK_TX_MALFORMED transaction has no root in the reference: its body does not decode.  Its 32 bytes are zero and defined[b] = 0.
 * Transactions of every other status decode, so their blocks have roots.  MALFORMED is decided by the decoder's rules alone: the signer and the chain id play
 * no part in it, and these entries take neither.
 *
 * Not here: CalcUncleHash; the receipts root (the engine entry zkgpu_list_trie_roots computes DeriveSha of any list of values of at least 32 bytes, no call uses it
 * for receipts); header.RTCMT / header.CMT against the tree; header validation; nodes under 32 bytes; tries over arbitrary keys; storing trie nodes.
 *
 * May be called from any thread; calls are served one at a time.  Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_TX_ROOTS_H
#define ZK_TX_ROOTS_H
#include <stdint.h>
#include "zk_bodies.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Transaction i is txs[off[i] .. off[i+1]), as in zk_txs.h; block b holds transactions block_first[b] .. block_first[b+1] - 1 (n_blocks + 1 entries, from 0 to n,
 * not decreasing).  roots[b]: DeriveSha of block b's transactions, emptyRoot for a block with none, zero where defined[b] = 0.  One upload, one download.
 * Returns the number of blocks with a defined root; -1, with every output zeroed, for a negative count, a null pointer with n > 0 or n_blocks > 0, a decreasing
 * off, a block_first that does not run from 0 to n without decreasing, no device (there is no host path), or a failure of any step.  The arguments are checked
 * before the device is asked for.  n_blocks = 0 returns 0 and queues nothing. */
int zkTxRoots(const uint8_t *txs, const uint64_t *off, int n, const int *block_first, int n_blocks, uint8_t (*roots)[32] /* n_blocks */, unsigned char *defined /* n_blocks */);

/* verifyChainBodies (zk_bodies.h) with one change in its step 2:
 *   2. B0: the first block that holds a transaction with status != ZK_TX_OK OR whose root is undefined or differs from want_roots[b] (header.TxHash of block b);
 *      n_blocks where there is none.
 * The roots are computed inside step 1, on the same upload.  roots[b] (as zkTxRoots writes it) and root_ok[b] (1: defined and equal to want_roots[b]) are written
 * for ALL blocks, also for those from B0 on.  Why block k failed, when k == B0: look at root_ok[k] first, then at status of its transactions; otherwise at ok of
 * its records.  Everything else, every -1 rule included, is verifyChainBodies' word for word; in addition a null want_roots, roots or root_ok with n_blocks > 0
 * gives -1, and -1 zeroes roots and root_ok as well. */
int verifyChainBodiesRoots(zk_proof_cache *cache, const uint8_t *txs, const uint64_t *off, int n, const int *block_first, int n_blocks, int signer, uint64_t chain_id,
                           zk_accts *accts, zk_tree *tree, const long long *prior_anchors, int n_prior, int window, zk_snset *set, zk_block_record *recs, uint8_t (*rec_froms)[20],
                           int32_t *rec_of, uint8_t (*txhash)[32], uint8_t (*froms)[20], uint8_t *code, uint8_t *status, unsigned char *ok /* per record */,
                           int32_t *anchor_of /* per record, may be NULL */, long long *accts_sizes, long long *set_sizes, long long *tree_sizes, int *n_recs,
                           const uint8_t (*want_roots)[32] /* n_blocks */, uint8_t (*roots)[32] /* n_blocks */, unsigned char *root_ok /* n_blocks */);

#ifdef __cplusplus
}
#endif
#endif
