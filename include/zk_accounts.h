/* Optional extension of the drop-in surface: the accounts' balance commitments kept resident next to the verifier, and a block decided in one call from nothing
 * but the transactions' own fields and their senders (DESIGN.md "Account table").
 *
 * The reference never takes cmtA_old (deposit: cmtb_old) from a transaction: it reads statedb.GetCMTBalance(msg.From()) and hands that to the verify symbol
 * (core/state_processor.go:112-157; the pool: core/tx_pool.go:618-641), and after the message is applied core/state_transition.go:221-223 stores the transaction's
 * ZKCMT() with SetCMT(msg.From(), cmt).  Genesis seeds the value; an account that does not exist reads as the zero hash.  So args[0] of a mint, send or redeem
 * record and args[2] of a deposit record (zk_records.h) are chain state.  A zk_accts is that state: a map from a 20-byte address to the 32 bytes of a common.Hash,
 * held in device memory as an append-only log of (address, value) entries with an index over it.
 *
 *   kind            the record's OLD slot (read from the table)     its NEW slot (stored after the block)
 *   mint / redeem   args[0]                                         args[2]
 *   send            args[0]                                         args[3]
 *   deposit         args[2]                                         args[4]
 *
 * Sizes name states, as in zk_tree_states.h and zk_spent.h: state `size` is the first `size` entries of the log; every zkAcctsSet record and every transaction of an
 * accepted block is one entry.  The value of an address at a state is the value of its latest entry below that size, or 32 zero bytes.  A caller keeps the size at
 * the end of every block, asks about any of them, and rewinds when the chain drops its last blocks.
 *
 * The block processor calls verifyBlockAccounts.  The pool verifies every pending transaction against the current state, whatever else is pending for the same
 * sender (tx_pool.go): its road is zkAcctsFillRecords(chained = 0) and then verifyBlockTree(commit = 0) (zk_tree_block.h) on the filled records.
 *
 * Who may call what at the same time: on one table, verifyBlockAccounts with commit != 0, zkAcctsSet and zkAcctsRewind belong to the block processor and must not
 * overlap each other; zkAcctsGet, zkAcctsFillRecords and calls with commit = 0 may run beside them, and each sees one state of the table.  There is no host table:
 * without a HIP device zkAcctsNew returns NULL.
 *
 * Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_ACCOUNTS_H
#define ZK_ACCOUNTS_H
#include <stdint.h>
#include "zk_tree_block.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct zkgpu_accts zk_accts;
zk_accts *zkAcctsNew(void);                                /* NULL on failure (no device) */
void      zkAcctsFree(zk_accts *accts);
long long zkAcctsSize(zk_accts *accts);                    /* the number of log entries, -1 on failure */
/* addrs[i] gets values[i], unconditionally and in order: an address may repeat, and then the later value wins.  Genesis and state import.  Returns 0, or -1 with
 * nothing changed: no device, a negative count, a null pointer. */
int zkAcctsSet(zk_accts *accts, const uint8_t (*addrs)[20], const uint8_t (*values)[32], int n);
/* out[i] = the value of addrs[i] at state at_size (-1: the current state), 32 zero bytes for an address without an entry there.  Returns 0, or -1 with nothing
 * written: no device, a negative count, a null pointer, a size above the table's. */
int zkAcctsGet(zk_accts *accts, const uint8_t (*addrs)[20], int n, long long at_size, uint8_t (*out)[32]);
/* The table goes back to its first `size` entries.  Returns 0; -1 and nothing changed if `size` is negative or exceeds the current size. */
int zkAcctsRewind(zk_accts *accts, long long size);
/* Overwrites the OLD slot of every record with kind <= 3, and nothing else of its 720 bytes; froms[i] is the sender of record i.  chained = 0: the table's current
 * value, for every record (the pool's rule).  chained != 0: the NEW slot of the closest earlier record of the call with the same sender and kind <= 3, or the
 * table's value if there is none (the block processor's rule, every earlier record taken as accepted).  The table does not change.  Returns 0, or -1 with nothing
 * written. */
int zkAcctsFillRecords(zk_accts *accts, const uint8_t (*froms)[20], zk_block_record *recs, int n, int chained);
/* A block decided as core/state_processor.go decides it, the balance commitments included:
 *   1. the arguments: verifyBlockTree's, and a null accts, or a null froms with n > 0;
 *   2. zkAcctsFillRecords(chained = 1) into recs — the caller gets the statements that were verified back;
 *   3. verifyBlockTree(cache, recs, n, tree, anchors, n_anchors, set, commit, ok, anchor_of, ...) on the filled records;
 *   4. f = the first record with ok = 0.  None: with commit, every record with kind <= 3 becomes an entry of the table, in record order, its NEW slot the value.
 *      Otherwise ok[i] = 0 and anchor_of[i] = -1 for every i > f — not decided: their statements assumed record f accepted —, with commit the set and the tree
 *      are rewound to their sizes before the call, and the table is untouched.
 * Returns the number of leading accepted records: n exactly when the block is valid.  A miner that wants to drop record f and go on calls again without it.
 * With commit = 0 nothing changes.  *accts_size_out, *set_size_out, *tree_size_out (each may be NULL): the sizes after the call (no set: not written; no tree: -1).
 * -1, with every output as verifyBlockTree leaves it on failure and the table, the set and the tree as they were: a bad argument — every one of them, an anchor's
 * range and the room for the block's sends included, is checked before recs is written or anything runs —, no device, a failure of any step; after a failure of a
 * later step recs may hold the filled old slots.  One exception: if, with commit, a step after verifyBlockTree fails AND the set or the tree cannot be rewound
 * (another writer broke the rule above), the call returns -1, says so on stderr, and writes the three sizes as they now are: the set or the tree may then hold
 * what the block added, and the caller rewinds them to the sizes it stored before the call. */
int verifyBlockAccounts(zk_proof_cache *cache, zk_block_record *recs, const uint8_t (*froms)[20], int n, zk_accts *accts, zk_tree *tree, const long long *anchors,
                        int n_anchors, zk_snset *set, int commit, unsigned char *ok, int32_t *anchor_of, long long *accts_size_out, long long *set_size_out,
                        long long *tree_size_out);

#ifdef __cplusplus
}
#endif
#endif
