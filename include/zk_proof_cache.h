/* Optional extension of the drop-in surface: a cache of the proofs this process has already verified (DESIGN.md "Proof cache").
 *
 * The reference node verifies every zk transaction twice: when it enters the pool (core/tx_pool.go:612-645) and again when its block is applied
 * (core/state_processor.go:106-163).  A zk_proof_cache remembers the records whose proof was accepted, so that the second verification is a lookup.  The pool and the
 * block processor share ONE cache: the pool's calls of verifyRecordsCached fill it, and verifyBlockFullCached finds a block's proofs there.
 *
 * The key of a record is the first 20 bytes of
 *     SHA-256( salt[32] || vktag[32] || record[720] )
 * salt: 32 bytes from getrandom(2), drawn when the cache is made and never shown.  vktag: the SHA-256 of the bytes of the verifying-key file of the record's kind,
 * taken when that file is loaded and kept beside the loaded key, so it names the key that verification uses — a key file that changes makes every stored key of its
 * kind unreachable.  All 720 bytes of the record are hashed, also `reserved` and the argument bytes zk_records.h calls ignored: two records that differ only there are
 * two keys, which costs a miss and never a wrong hit.  Records of a kind above 3, or of a kind whose key cannot be loaded, have no key: they are never looked up and
 * never stored.
 *
 * What is cached: "this record's proof verified under this key", and only acceptances.  What is not: everything that depends on the state of the chain.  The roots
 * (zk_roots.h) and the serial numbers (zk_spent.h) are decided on every call over all records exactly as verifyBlockFull decides them; a record whose proof is stored
 * but whose root is wrong or whose serial number is spent is rejected.  A proof's validity depends on the record and the key alone, so the cache needs no rewind
 * after a reorganisation, and storing does not depend on `commit`.
 *
 * False hits.  A wrong acceptance needs a record whose 160 truncated bits equal a stored key under a salt its sender never sees.  Even with the salt known that is a
 * second preimage on SHA-256 truncated to 160 bits, 2^160 work.  A pair of records crafted together to collide would be 2^80 work with the salt known — the only
 * birthday case, and it needs one record of the pair to be valid and accepted first.
 *
 * Size.  `capacity` is a number of entries, 20 bytes of key and 8 to 16 bytes of index each.  The cache keeps two generations of capacity / 2 entries: when the young
 * one is full the old one is dropped, so a record stays for at least capacity / 2 later insertions.  A call that brings more than capacity / 2 new records stores
 * the first capacity / 2 of them.
 *
 * If a step of the cache fails (the device, memory), the call says so on stderr and decides every record by verification, as the uncached entry does: the cache never
 * costs a decision.  Calls may arrive on any thread; two threads that verify the same record at the same time both verify it, and it is stored once.
 * There is no host cache: without a HIP device zkProofCacheNew returns NULL, and NULL in place of a cache gives exactly the uncached entry.
 *
 * Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_PROOF_CACHE_H
#define ZK_PROOF_CACHE_H
#include <stdint.h>
#include "zk_records.h"
#include "zk_roots.h"
#include "zk_spent.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct zkgpu_proof_cache zk_proof_cache;
zk_proof_cache *zkProofCacheNew(long long capacity);   /* NULL without a device or for capacity < 2 */
void zkProofCacheFree(zk_proof_cache *cache);
int  zkProofCacheClear(zk_proof_cache *cache);         /* forgets every record; the counters go on.  0, or -1 on failure */
/* out = {hits, misses, records stored, entries held now}, the first three counted since the cache was made.  0, or -1 on failure */
int  zkProofCacheStats(zk_proof_cache *cache, uint64_t out[4]);
/* verifyBlockRecords(recs, n, ok) with the proof step cached: the records found in the cache are accepted at once, the others are verified together as
 * verifyBlockRecords verifies them, and those accepted are stored.  The transaction pool's call, for one arrival or a few. */
int  verifyRecordsCached(zk_proof_cache *cache, const zk_block_record *recs, int n, unsigned char *ok);
/* verifyBlockFull(recs, n, l, list_of, set, commit, ok, size_out) with the same proof step. */
int  verifyBlockFullCached(zk_proof_cache *cache, const zk_block_record *recs, int n, const zk_cmt_lists *l, const int32_t *list_of,
                           zk_snset *set, int commit, unsigned char *ok, long long *size_out);

#ifdef __cplusplus
}
#endif
#endif
