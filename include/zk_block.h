/* Optional extension of the drop-in surface: verification of a whole block with one randomized pairing-product check (DESIGN.md "Block verification").
 *
 * verifyBlock takes the same items as verifyBatch (zk_batch.h) and reaches the same verdicts, by another road: one equation over the records of every kind with
 * at least 8,192 records in the block (random 128-bit weights from getrandom(2), one final exponentiation for the block) instead of one pairing check per proof.
 * If the equation fails — some record is bad — or cannot be formed, every record is decided by verifyBatch's per-proof path, so ok[] then says which proof
 * failed.  The check is
 * probabilistic: a block holding a bad proof passes the equation with probability at most 1/(2^128 - 1); verifyBatch is deterministic.  A smaller kind
 * takes the per-proof path at once (below that size it is the faster one).
 *
 * Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_BLOCK_H
#define ZK_BLOCK_H
#include "zk_batch.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ok[i] = 1 if item i is accepted, 0 otherwise, exactly as verifyBatch decides.  Returns the number of accepted proofs, or -1 if no decision could be made
 * (every ok[i] is 0 then). */
int verifyBlock(const zk_verify_item *items, int n, unsigned char *ok);

#ifdef __cplusplus
}
#endif
#endif
