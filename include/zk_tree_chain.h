/* Optional extension of the drop-in surface: a stretch of the chain — many blocks — decided against the resident commitment tree in one call (DESIGN.md "A
 * stretch of the chain").
 *
 * A node that syncs, or imports again after a long reorganisation, holds hundreds of blocks at once.  verifyBlockTree (zk_tree_block.h) with commit = 1 decides one
 * of them; a block of some hundred records never reaches the block equation and pays the per-proof path, call after call.  verifyChainTree takes the whole segment:
 * the proof step runs once over every record, the sends' commitments become leaves in one append, every deposit is compared with the roots of its own window of
 * anchors, and the spend step runs once.  What it decides is exactly what this loop decides:
 *
 *   for b = 0, 1, ...:  verifyBlockTree(cache, block b, tree, A[lo_b .. hi_b), set, commit = 1)
 *     every record accepted: go on with block b + 1;
 *     otherwise: take block b back whole — zkSnSetRewind and zkTreeRewind to the sizes before it — and stop.
 *
 * which is the network's rule: a block with a failing transaction is invalid.  A is the anchor sequence: prior_anchors[0 .. n_prior) in the caller's order, then
 * s_0 ... s_{n_blocks - 1}, where s_b is the tree's size after block b.  A deposit of block b may match A[lo_b .. hi_b) with hi_b = n_prior + b and
 * lo_b = max(0, hi_b - window): the last size it can reach is the end of the block before it, never its own block's end (the append comes last in a block).  A caller
 * that wants the size at the start of the segment among the anchors puts it last into prior_anchors.  window = 0 rejects every deposit.
 *
 * There is no commit argument: this is the block processor's call.  It appends to the tree and spends into the set, so on one tree and one set it must not overlap
 * verifyBlockTree with commit != 0, zkTreeAppend, zkTreeRewind, zkSnSetRewind or another verifyChainTree; the pool's verifyBlockTree with commit = 0, zkTreeRoot* and
 * the genDepositproofTree* calls may run beside it.  A reader that runs beside it may see the tree and the set ahead of what the call leaves: the call works on the
 * longest prefix of blocks that can still be valid and takes back what a later step refuses.
 *
 * Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_TREE_CHAIN_H
#define ZK_TREE_CHAIN_H
#include <stdint.h>
#include "zk_tree_block.h"
#ifdef __cplusplus
extern "C" {
#endif

/* recs, n, cache, set (NULL: no spend step): as verifyBlockTree takes them.  block_first: n_blocks + 1 entries, non-decreasing, block_first[0] = 0 and
 * block_first[n_blocks] = n; block b is recs[block_first[b] .. block_first[b + 1]) and may be empty.  prior_anchors: n_prior tree sizes, 0 <= size <= the tree's size.
 * Returns the number of leading blocks accepted whole, 0 ... n_blocks; the set and the tree are left in the state after the last of them.
 *   ok[i]:         1 for a record of an accepted block; for the first rejected block what verifyBlockTree with commit = 0 says about it against the state after the
 *                  block before it; 0 for every record of a later block.
 *   anchor_of[i]   (n entries, or NULL): for a deposit of an accepted block or of the first rejected one that passed the proof step and matched, the lowest index
 *                  INTO A (not into its window) inside its window; -1 for every other record.
 *   set_sizes[b], tree_sizes[b] (n_blocks entries each, or NULL; set_sizes is not written without a set): the sizes after block b for an accepted block — what a
 *                  caller stores for later rewinds and anchors —, for every other block the sizes the call leaves.
 * -1, with every ok[i] = 0, every anchor_of[i] = -1 and the tree and the set as they were: a null tree; n < 0, n_blocks < 0, a null recs or ok with n > 0, a null or
 * malformed block_first; n_prior < 0 or a null prior_anchors with n_prior > 0; window < 0; a prior anchor that is negative or above the tree's size; more send
 * records in the call than the tree has room for (the segment is refused whole before any proof is looked at); no device; a device failure in any later step — the
 * call then rewinds what it has appended and spent. */
int verifyChainTree(zk_proof_cache *cache, const zk_block_record *recs, int n, const int *block_first, int n_blocks, zk_tree *tree, const long long *prior_anchors,
                    int n_prior, int window, zk_snset *set, unsigned char *ok, int32_t *anchor_of, long long *set_sizes, long long *tree_sizes);

#ifdef __cplusplus
}
#endif
#endif
