/* Optional extension of zk_tree.h: the resident commitment tree at past sizes, and its rewind after a reorganisation of the chain (DESIGN.md "Past states of
 * the commitment tree").
 *
 * A zk_tree is append-only, but it never overwrites a complete subtree, so it still holds every state it went through: state `size` is the tree of its first
 * `size` leaves, 0 <= size <= the current number of leaves.  A caller keeps the sizes it cares about — zkTreeAppend returns the size after each block — and asks
 * for the root of any of them, proves a deposit against the root at the end of a block that is already final, and, when the chain drops its last blocks, rewinds
 * the tree to the size before them.  None of these calls sees the commitments again, and each costs one walk up the tree whatever its size.
 *
 * Two things to keep in mind:
 *   - A size names a state only as long as the tree has not been rewound below it.  If the tree was rewound below `size` and has grown past it again with other
 *     leaves, state `size` is a DIFFERENT state under the same number.  genDepositproofTreeAt returns in rt_out the root it actually proved against; the caller
 *     compares it with the root it meant.
 *   - Every call sees one state of the tree under one lock.  A rewind does not disturb calls that already hold their snapshot: a proof that took its path before
 *     the rewind is finished against the root of that path.
 *
 * Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_TREE_STATES_H
#define ZK_TREE_STATES_H
#include <stdint.h>
#include "zk_tree.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the root of the first `size` leaves: 64 hex characters, malloc'd like zkTreeRoot's; at depth 8 equal to genRoot over those commitments.  NULL on failure
 * (no device, a negative size, a size above the tree's). */
char     *zkTreeRootAt(zk_tree *t, long long size);
/* roots: q x 32 bytes, root i of the first sizes[i] leaves as the bytes of its common.Hash; sizes in any order, repeats allowed, q = 0 allowed.  One kernel launch
 * for all of them.  Returns 0, or -1 with nothing written: no device, a negative size or count, a size above the tree's. */
int       zkTreeRootsAt(zk_tree *t, const long long *sizes, int q, uint8_t *roots);
/* The tree goes back to its first `size` leaves.  Returns the new number of leaves; -1 and nothing changed if `size` exceeds the current number or is negative.
 * The commitments after `size` need not be passed and cannot be brought back: append the new branch's commitments next. */
long long zkTreeRewind(zk_tree *t, long long size);
/* genDepositproofTree against state `size`: cmtS is looked for among the first `size` leaves only, and path and root are those of that state; the key is the one
 * of the tree's depth.  rt_out receives the root the proof was made against.  Failure — cmtS is not among those leaves, `size` is negative or exceeds the tree's
 * size (for instance after a rewind below it), no key, a statement that violates the circuit: the reference's sentinel proof and rt_out[0] = 0. */
char *genDepositproofTreeAt(uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *sns, char *rs, char *cmtB_old,
                            char *cmtB, uint64_t value_s, char *pk, char *sn_A_old, char *cmtS, char *sk, zk_tree *t, long long size, char rt_out[65]);

#ifdef __cplusplus
}
#endif
#endif
