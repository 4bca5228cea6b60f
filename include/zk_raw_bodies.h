/* Optional extension of the drop-in surface: block bodies from their bytes, split and packed on the device.
 *
 * Every call of zk_txs.h, zk_bodies.h and zk_tx_roots.h takes the position of every single transaction: txs, off, n, block_first.  A node does not have those
 * positions.  What a peer delivers (eth/protocol.go:177-183, blockBody) and what the database keeps is rlp(types.Body) = rlp([[tx ...], [uncle ...]])
 * (core/types/block.go:143-146), so a caller of those headers walks every body's outer list and reads one RLP head a transaction before the device sees a byte.
 * This header takes the bodies as they were delivered, one offset a BLOCK: body b is bodies[body_off[b] .. body_off[b+1]), body_off has n_blocks + 1
 * non-decreasing entries.
 *
 * body_status[b] is the first of these rules that applies:
 *   ZK_BODY_MALFORMED  rlp.DecodeBytes(body, &types.Body{}) would fail on the body's structure.  The heads are decided by the strict reader the transaction walk
 *                      uses (zk_txs.h; Stream.readKind, rlp/decode.go:902-960, with Kind's bound :883-894):
 *     - the outer item is no list (makeStructDecoder, decode.go:438, List :762), or its payload does not end exactly at body_off[b+1] (beyond the input: :886, :891;
 *       short of it: DecodeBytes :142-144, ErrMoreThanOneValue);
 *     - it does not hold exactly two items: "too few elements" where a field finds the list at its end (:443-444), "input list has too many elements" where the
 *       list goes on behind the last field (:449, ListEnd :778);
 *     - item 0 (Transactions) or item 1 (Uncles) is no list: both fields are slices, decodeListSlice asks for a list (:323-326);
 *     - an element head inside item 0 is not canonical — the long form for a size under 56 (:938, :957), a leading zero byte in the size (readUint :980-985), a
 *       one-byte string below 0x80 that should have stood alone (:662, :423, :726) — or ends beyond item 0 (:886, :891): every element's head is read by Stream.Kind
 *       before anything of the element is decoded, so such a head refuses the body whatever the element is;
 *     - the body is empty: io.ErrUnexpectedEOF (:142 with :910);
 *     - the body is longer than 2^32 - 1 bytes: this library's own bound, as for headers (zk_headers.h).
 *   ZK_BODY_UNCLES     item 1 is a canonical list that is not empty, whatever it holds.  The reference refuses such a block one way or another: the uncles do not
 *                      decode as headers; or VerifyUncles says "uncles not allowed" (consensus/clique/clique.go:450-455); or CalcUncleHash(block.Uncles()) is not
 *                      header.UncleHash (core/block_validator.go:67; eth/downloader/queue.go:772), which zkHeaders (zk_headers.h) has held to Keccak256(c0), the hash
 *                      of the empty list.  This call does not tell the three apart.
 *   ZK_BODY_OK         otherwise.
 * An element of item 0 is NOT judged here: its extent — its head and its payload, or the lone byte — goes to the walk as transaction i, and the walk decides
 * ZK_TX_MALFORMED as it always has.  An element that is a string or a lone byte lands there (Transaction.DecodeRLP wants a list, decode.go:438).
 * A body that is not OK contributes NO transactions: block_first[b+1] == block_first[b], wherever its fault lies.
 *
 * Outputs: *n_txs = n, the number of transactions of all OK bodies; block_first (n_blocks + 1 entries, from 0 to n) is over those transactions; tx_beg[i] and
 * tx_size[i] are transaction i's extent in the caller's own bodies buffer, so the transaction behind a status, a txhash or a record is found without walking anything.
 *
 * Not here: the 3-item block form [header, txs, uncles] (zkHeaders wants contiguous headers); parsing the outer list of a BlockBodiesMsg; decoding uncles; a
 * parallel walk inside one body's list; the snapshot; any change to the walk, the recovery, the trie or verifyChainAccounts.
 *
 * May be called from any thread; calls are served one at a time.  Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_RAW_BODIES_H
#define ZK_RAW_BODIES_H
#include <stdint.h>
#include "zk_tx_roots.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { ZK_BODY_OK = 0, ZK_BODY_MALFORMED = 1, ZK_BODY_UNCLES = 2 };

/* Returns k, the number of leading bodies with status ZK_BODY_OK.
 * -2 where n > cap: *n_txs, block_first and body_status are valid, tx_beg and tx_size are zeroed; the caller can call again with room.
 * -1, with every output zeroed, for a negative count, a null pointer with n_blocks > 0, a decreasing body_off, more than 2^30 - 1 transactions, no device (there is
 * no host path), or a failure of any step.  The arguments are checked before the device is asked for.  n_blocks = 0 returns 0, sets *n_txs = 0 and block_first[0] = 0
 * where they are given, and queues nothing. */
int zkBodySplit(const uint8_t *bodies, const uint64_t *body_off, int n_blocks, int cap, uint64_t *tx_beg /* cap */, uint32_t *tx_size /* cap */,
                int *block_first /* n_blocks + 1 */, uint8_t *body_status /* n_blocks */, int *n_txs);

/* verifyChainBodiesRoots (zk_tx_roots.h) word for word on the transactions the split found — txs, off, n and block_first are the device's own, the bodies' bytes
 * cross the bus once — with three differences:
 *   - B0 is also the first block whose body_status != ZK_BODY_OK; such a block has roots[b] zero and root_ok[b] = 0;
 *   - n > cap returns -2 with *n_txs set: nothing else is written and nothing is committed, so the caller can call again with room;
 *   - -1 also zeroes tx_beg, tx_size, block_first, body_status and *n_txs; a negative cap or a null pointer among them gives -1.
 * Every per-transaction output (recs .. status, ok, anchor_of, tx_beg, tx_size) has room for cap.  Why block k failed: look at body_status[k] first, then at
 * verifyChainBodiesRoots' own order. */
int verifyChainRawBodies(zk_proof_cache *cache, const uint8_t *bodies, const uint64_t *body_off, int n_blocks, int cap, int signer, uint64_t chain_id, zk_accts *accts,
                         zk_tree *tree, const long long *prior_anchors, int n_prior, int window, zk_snset *set, zk_block_record *recs, uint8_t (*rec_froms)[20],
                         int32_t *rec_of, uint8_t (*txhash)[32], uint8_t (*froms)[20], uint8_t *code, uint8_t *status, unsigned char *ok /* per record */,
                         int32_t *anchor_of /* per record, may be NULL */, long long *accts_sizes, long long *set_sizes, long long *tree_sizes, int *n_recs,
                         const uint8_t (*want_roots)[32] /* n_blocks */, uint8_t (*roots)[32] /* n_blocks */, unsigned char *root_ok /* n_blocks */,
                         uint64_t *tx_beg /* cap */, uint32_t *tx_size /* cap */, int *block_first /* n_blocks + 1 */, uint8_t *body_status /* n_blocks */, int *n_txs);

#ifdef __cplusplus
}
#endif
#endif
