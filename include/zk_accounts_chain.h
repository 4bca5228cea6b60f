/* Optional extension of the drop-in surface: a stretch of the chain — many blocks — decided in one call from nothing but the transactions' own fields and their
 * senders, against the resident account table, commitment tree and spent set (DESIGN.md "A stretch of the chain with accounts").
 *
 * verifyChainTree (zk_tree_chain.h) takes the records' OLD balance commitments from the caller.  The reference never takes them from a transaction: they are chain
 * state, statedb.GetCMTBalance(msg.From()), chained through every earlier transaction of the same sender (zk_accounts.h).  verifyBlockAccounts reads them from the
 * table for one block; verifyChainAccounts does it for a whole segment.  What it decides is exactly what this loop decides:
 *
 *   for b = 0, 1, ...:  r = verifyBlockAccounts(cache, block b, its froms, accts, tree, A[lo_b .. hi_b), set, commit = 1, ...)
 *     r == the block's record count: go on with block b + 1
 *     otherwise: stop   (verifyBlockAccounts has already taken the set and the tree back and left the table alone)
 *
 * A, lo_b, hi_b, block_first, window, cache and set == NULL are as zk_tree_chain.h defines them; tree is required, as there.
 *
 * The old slots are filled once, over the whole segment, every earlier record of the same sender taken as accepted.  As long as every earlier block was accepted
 * whole, and inside the first rejected block up to its first rejected record f, that assumption holds, and the filled value IS the sender's current value.  Beyond
 * f it does not: those verdicts are reported as "not decided", as verifyBlockAccounts reports them.
 *
 * Who may call what at the same time: the table's mutex is held only inside the fill and inside the append, never together with the cache's, the set's or the
 * tree's.  On one table, set and tree the call must not overlap another committing call (verifyChainAccounts, verifyChainTree, verifyBlockAccounts or verifyBlockTree
 * with commit != 0, zkAcctsSet, zkTreeAppend, or a rewind of any of the three); readers and calls with commit = 0 may run beside it, and may see the set and the tree
 * ahead of what the call leaves.
 *
 * Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_ACCOUNTS_CHAIN_H
#define ZK_ACCOUNTS_CHAIN_H
#include <stdint.h>
#include "zk_accounts.h"
#include "zk_tree_chain.h"
#ifdef __cplusplus
extern "C" {
#endif

/* recs, n, block_first, n_blocks, prior_anchors, n_prior, window, cache, set: as verifyChainTree takes them.  froms[i]: the sender of record i.
 * Returns the number of leading blocks accepted whole, 0 ... n_blocks; the table, the set and the tree are left in the state after the last of them.
 *   ok[i]:         1 for a record of an accepted block; in the first rejected block 1 before its first rejected record f and 0 from f on; 0 for every later block.
 *   anchor_of[i]   (n entries, or NULL): as verifyChainTree reports it — an index INTO A — for the records of accepted blocks and for the records up to AND INCLUDING f
 *                  of the first rejected block (a deposit that matched and lost at the spend step keeps its anchor, as in verifyBlockTree); -1 for every other record.
 *   recs:          the OLD slot of every record with kind <= 3 holds the chained fill over the whole segment — what zkAcctsFillRecords(chained = 1) on the whole segment
 *                  writes — and nothing else of the 720 bytes changes.  For accepted blocks, and up to f in the first rejected one, these are the statements that were
 *                  verified, and they equal what the loop writes.  Beyond that they are values under an assumption that failed: the loop would never have formed them.
 *   accts_sizes[b], set_sizes[b], tree_sizes[b] (n_blocks entries each, any of them may be NULL; set_sizes is not written without a set): for an accepted block
 *                  the sizes after block b — what a caller stores for later rewinds and anchors —, for every other block the sizes the call leaves.
 * -1, with every ok[i] = 0, every anchor_of[i] = -1 and the table, the set and the tree as they were: any argument verifyChainTree refuses; a null accts; a null froms
 * with n > 0; a log without room for the segment; no device; a failure of any step.  Every argument is checked before recs is written or anything is queued; after a
 * failure of a later step recs may hold the filled old slots.  If the table's append fails after verifyChainTree has committed, the set and the tree are rewound to
 * their sizes before the call.  One exception: if that rewind is impossible (another writer broke the rule above), the call returns -1, says so on stderr, and writes
 * the sizes as they now are into the LAST entry of each sizes array; the caller rewinds to the sizes it stored before the call. */
int verifyChainAccounts(zk_proof_cache *cache, zk_block_record *recs, const uint8_t (*froms)[20], int n, const int *block_first, int n_blocks, zk_accts *accts,
                        zk_tree *tree, const long long *prior_anchors, int n_prior, int window, zk_snset *set, unsigned char *ok, int32_t *anchor_of,
                        long long *accts_sizes, long long *set_sizes, long long *tree_sizes);

#ifdef __cplusplus
}
#endif
#endif
