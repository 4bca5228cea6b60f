/* Optional extension of the drop-in surface: the set of spent serial numbers kept resident next to the verifier, and a block's proofs, roots and serial numbers
 * decided in one call (DESIGN.md "Spent serial numbers").
 *
 * The reference node makes one state check for every zk transaction (core/state_processor.go:106-163): statedb.Exist(common.BytesToAddress(tx.ZKSN().Bytes()))
 * fails the transaction with "sn is already used" — the single exempt value is initSN — and after the proof is accepted CreateAccount and SetNonce burn the address.
 * A zk_snset is that set of addresses: an append-only log of distinct 20-byte keys in insertion order, held in device memory with an index over it.  A key is bytes
 * 12..31 of the serial number's common.Hash, which is what common.BytesToAddress keeps.  The serial number of a record (zk_records.h) is args[1] for mint, send and
 * redeem and args[3] (snold) for deposit.
 *
 * Sizes name states, as in zk_tree_states.h: state `size` is the first `size` keys of the log, zkSnSetSpend and verifyBlockFull return the size after the call, a
 * caller keeps the size at the end of every block, asks about any of them, and when the chain drops its last blocks rewinds the set to the size before them.  A size
 * names a state only as long as the set has not been rewound below it.
 *
 * Deposit's one-time pk address lives in the same account space in the reference.  It is NOT part of a record's check here: with two keys a record, whether one record
 * is accepted would depend on whether an earlier one was, one after the other through the block.  A caller that wants pk checked passes those addresses (20 bytes at
 * offset 12 of a 32-byte entry) through zkSnSetSpend in a call of its own.  zk_spent_pk.h has the calls that decide both keys of a record together, as the reference does.
 *
 * A call is an upload, three kernel launches and a download whatever the number of keys, and whatever the size of the set: measured on one MI355X 0.03 ms for one
 * key, 0.06 ms for 8,192 and 0.13-0.18 ms for 65,536 (profiles/snset.txt; DESIGN.md "Spent serial numbers").  Against a hash map on one host core that is 6-8 times
 * slower for a single key and 30-110 times faster for 8,192 or more keys on sets of a million entries and up; a call pays from a few hundred keys on.  One cost to know: a call needs keys + tombstones + the call's own keys to fit half of the index.  A committing call that finds less room rebuilds
 * the index once, larger, and keeps it; a check-only call (commit = 0) must leave the set untouched, so it runs on a rebuilt copy and drops it — and so does every later
 * check-only call, a full rebuild each, until a committing call has grown the index.  After a committing call at least half of the index is free, so this is met only
 * by a check-only call with more keys than the set holds, or in the window after rewinds and before the next committing call.
 * Calls may arrive on any thread; each sees one state of the set.  There is no host set:
 * without a HIP device zkSnSetNew returns NULL.
 *
 * Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_SPENT_H
#define ZK_SPENT_H
#include <stdint.h>
#include "zk_records.h"
#include "zk_roots.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct zkgpu_snset zk_snset;
/* exempt_sn: the 32 bytes of a common.Hash that is never in conflict and never inserted (the node passes initSN), or NULL.  NULL on failure (no device). */
zk_snset *zkSnSetNew(const uint8_t *exempt_sn);
void      zkSnSetFree(zk_snset *set);
long long zkSnSetSize(zk_snset *set);                       /* the number of keys, -1 on failure */
/* in[i] = 1 if sns[i] (n x 32 bytes, each the bytes of a common.Hash) is among the first `size` keys, else 0; size < 0: the current state.  Returns 0, or -1 with
 * nothing written: no device, a negative count, a null pointer, a size above the set's. */
int       zkSnSetContains(zk_snset *set, long long size, const uint8_t *sns, int n, unsigned char *in);
/* The set goes back to its first `size` keys.  Returns the new size; -1 and nothing changed if `size` is negative or exceeds the current size. */
long long zkSnSetRewind(zk_snset *set, long long size);
/* The reference's loop over sns[0 .. n) in order: spent[i] = 1 if sns[i] is in the set or equals an earlier sns[j] of this call, else 0 — and then, with commit != 0,
 * it is added.  The exempt value gives 0 and is never added.  commit = 0 leaves the set exactly as it was.  Returns the size after the call, -1 on failure (nothing
 * written, nothing changed). */
long long zkSnSetSpend(zk_snset *set, const uint8_t *sns, int n, int commit, unsigned char *spent);
/* verifyBlockRecordsRoots(recs, n, l, list_of, ok) — l and list_of may be NULL as there — and then the loop above over the serial numbers of the records that are
 * still accepted: ok[i] is cleared where record i spends a serial number that is in the set, or that an earlier accepted record of this block spends.  commit = 0 is
 * the transaction pool's check, commit = 1 is block processing: the serial numbers of the accepted records are added.  size_out (may be NULL) receives the size after
 * the call.  Returns the number of records still accepted, or -1 with every ok[i] = 0 and the set unchanged if no decision could be made.  set = NULL: exactly
 * verifyBlockRecordsRoots, and size_out is not written. */
int verifyBlockFull(const zk_block_record *recs, int n, const zk_cmt_lists *l, const int32_t *list_of, zk_snset *set, int commit, unsigned char *ok, long long *size_out);

#ifdef __cplusplus
}
#endif
#endif
