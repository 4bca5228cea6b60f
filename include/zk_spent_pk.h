/* Optional extension of the drop-in surface: the spent set decides records with two keys, a deposit's one-time pk address included (DESIGN.md "Two keys a record").
 *
 * The reference burns two addresses for a deposit (core/state_processor.go:136-179): the serial number's before the message is applied, and after ApplyMessage the
 * one-time pk address, which fails with "cannot use randompubkey for a second time".  Both live in one account space, so here both are keys of one zk_snset
 * (zk_spent.h).  The calls below decide a batch exactly as the reference's loop does record by record — a miner that drops the failing transaction and goes on, and
 * the pool's check, get the reference's answer:
 *   - a record is rejected if one of its keys is in the set, or was inserted by an earlier ACCEPTED record of the same call, or if its two keys are equal;
 *   - a rejected record inserts nothing: a deposit rejected for its pk has not burnt its serial number, and one rejected for its serial number leaves its pk free for
 *     a later deposit of the block;
 *   - an accepted deposit adds its serial number and then its pk, so it advances the size by two.  Sizes name states as before; a rewind may land between the two.
 *
 * One case differs from the reference.  The exempt value of zkSnSetNew (initSN) applies to serial numbers only and is never inserted, so it cannot be told apart from
 * a fresh key later; a record whose pk address equals the exempt key is therefore rejected, conservatively.  The reference would accept the first such deposit.  The
 * difference costs nothing short of a 160-bit collision between a pk address and initSN's address.
 *
 * The decision is not made one record after the other: it is the lowest-index-first greedy choice on the graph of records that share a key, taken in parallel rounds
 * on the device.  A batch without a conflict among its own keys takes one round; an adversarial chain of L double-spending deposits takes L / 2, so after 8 rounds
 * the host finishes what is still open.  One cost to know: with commit, a slot that a rejected record had claimed in the last round stays behind as a tombstone, as
 * after a rewind, and counts against the index until its next rebuild.  The room a call needs is keys + tombstones + 2n at or below half of the index.
 *
 * Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_SPENT_PK_H
#define ZK_SPENT_PK_H
#include <stdint.h>
#include "zk_spent.h"
#include "zk_proof_cache.h"
#ifdef __cplusplus
extern "C" {
#endif

/* zkSnSetSpend with an optional second key a record.  sns: n x 32 bytes as there.  pks: n x 32 bytes, the address in bytes 12..31 of each entry as zkSnSetSpend's
 * callers already pass it; an entry of 32 zero bytes means that record i has no second key, and pks = NULL that none has.  spent[i] = 1 if record i is rejected by
 * the rules above, else 0 — and then, with commit != 0, sns[i] and pks[i] are added, in this order.  The exempt value as sns[i] is neither checked nor added, and the
 * record's pk still is.  commit = 0 leaves the set exactly as it was.  Returns the size after the call, -1 on failure (nothing written, nothing changed). */
long long zkSnSetSpendPairs(zk_snset *set, const uint8_t *sns, const uint8_t *pks, int n, int commit, unsigned char *spent);
/* verifyBlockFullCached(cache, recs, n, l, list_of, set, commit, ok, size_out) — cache = NULL: verifyBlockFull — with the pk address checked: a deposit record that is
 * still accepted brings two keys, its serial number and the 20 bytes of pk in args[1][0..19]; every other accepted record brings its serial number; a record with
 * ok[i] = 0 brings none.  This is the call for a miner's block assembly and for the pool (commit = 0), as it is for a block from the network (commit = 1).  Returns the
 * number of records still accepted, or -1 with every ok[i] = 0 and the set unchanged if no decision could be made.  set = NULL: exactly verifyBlockRecordsRoots (behind
 * the cache, if one is given), and size_out is not written. */
int verifyBlockState(zk_proof_cache *cache, const zk_block_record *recs, int n, const zk_cmt_lists *l, const int32_t *list_of, zk_snset *set, int commit,
                     unsigned char *ok, long long *size_out);

#ifdef __cplusplus
}
#endif
#endif
