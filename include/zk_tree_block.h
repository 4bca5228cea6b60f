/* Optional extension of the drop-in surface: a block of records decided against the resident commitment tree, in one call (DESIGN.md "A block against the
 * resident tree").
 *
 * verifyBlockState (zk_spent_pk.h) decides a block for the reference's depth-8 scheme, in which a deposit names the commitments of its blocks.  A deployment that
 * keeps ONE tree of depth d in a zk_tree (zk_tree.h, zk_tree_states.h) proves its deposits against a root of that tree instead, and this is its block call:
 *   1. the proof step of verifyBlockState — cache, block equation, per-proof path — with the deposit records under the key of depth d (depth 8: depositvk.txt,
 *      any other: deposit<d>vk.txt), which is also the key the cache's entries for deposits are tagged with;
 *   2. the anchor step: a deposit still accepted stays so only if its RT (args[0]) is the root of the tree at one of the sizes the caller offers — the sizes of the
 *      tree after the blocks it accepts as anchors, for instance its last W blocks.  The roots are made and compared on the device; no root crosses to the host;
 *   3. the spend step of verifyBlockState: a deposit brings its serial number and its pk address, every other accepted record its serial number;
 *   4. with commit, the append step: the cmtS (args[2]) of every send still accepted becomes a leaf of the tree, in record order, as one zkTreeAppend — the
 *      reference builds a block's header.CMT from exactly these (miner/worker.go:461-467).
 *
 * Who may call what at the same time:
 *   - a call with commit != 0, zkTreeAppend and zkTreeRewind on one tree belong to the block processor and must not overlap each other;
 *   - calls with commit = 0 are the pool's: they may run beside readers and beside the block processor, as may zkTreeRoot* and the genDepositproofTree* calls;
 *   - the commitments of the block itself are no anchors: the append comes last, so a deposit cannot be proved against a send of its own block.
 *
 * Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_TREE_BLOCK_H
#define ZK_TREE_BLOCK_H
#include <stdint.h>
#include "zk_tree_states.h"
#include "zk_spent_pk.h"
#ifdef __cplusplus
extern "C" {
#endif

/* recs, n, cache, set, commit, ok: as verifyBlockState takes them.  anchors: n_anchors tree sizes, 0 <= anchors[a] <= the tree's size, in any order, repeats and 0
 * (the empty root) allowed; n_anchors = 0 rejects every deposit.  anchor_of (n entries, or NULL): the lowest a with RT == root(anchors[a]) for a deposit that passed
 * the proof step and matched, -1 for every other record.  set = NULL skips the spend step.  *set_size_out (or NULL): the set's size as verifyBlockState reports it;
 * *tree_size_out (or NULL): the tree's number of leaves after the call.  With commit = 0 neither the set nor the tree changes.
 * Returns the number of records accepted.  -1, with every ok[i] = 0, every anchor_of[i] = -1 and nothing changed: n < 0, n_anchors < 0, a null recs or ok with n > 0,
 * a null anchors with n_anchors > 0, an anchor that is negative or above the tree's size, with commit more send records than the tree has room for (the block is
 * refused whole before any proof is looked at), no device, a device failure in the anchor step (the tree has no host model), or an append that fails although the
 * block fitted when the call began — another writer broke the rule above; the call then takes its own spend back (zkSnSetRewind to the size before it).
 * tree = NULL: exactly verifyBlockState(cache, recs, n, NULL, NULL, set, commit, ok, set_size_out), every anchor_of[i] = -1 and *tree_size_out = -1. */
int verifyBlockTree(zk_proof_cache *cache, const zk_block_record *recs, int n, zk_tree *tree, const long long *anchors, int n_anchors, zk_snset *set, int commit,
                    unsigned char *ok, int32_t *anchor_of, long long *set_size_out, long long *tree_size_out);

#ifdef __cplusplus
}
#endif
#endif
