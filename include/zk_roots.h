/* Optional extension of the drop-in surface: the roots of many commitment lists in one call, and a block of records verified together with the roots its
 * deposits name (DESIGN.md "Roots of many lists").
 *
 * A node checks a deposit's root by gathering the commitments of the blocks the transaction names, calling genRoot on them and comparing the result with the
 * transaction's RT: one hex string and 255 compressions on one core per deposit.  genRoots takes the commitments of a whole block's deposits as bytes — one shared
 * array and one range per list — and computes every root on the device; verifyBlockRecordsRoots does that beside verifyBlockRecords and ANDs the comparison into
 * the verdicts.
 *
 * A list is ONE contiguous range of the shared array.  Lists may overlap, coincide or be empty, so commitments that several transactions name are passed once;
 * a list made of several non-adjacent pieces of the array is not supported: the caller lays such a list out once more as a range of its own.
 *
 * Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_ROOTS_H
#define ZK_ROOTS_H
#include <stdint.h>
#include "zk_records.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t first, count; } zk_cmt_range;   /* a list = commitments first .. first + count - 1 of the array */
typedef struct {
  const uint8_t      *cmts;     /* n_cmts x 32 bytes, each commitment as the bytes of its common.Hash */
  uint64_t            n_cmts;
  const zk_cmt_range *lists;
  int                 n_lists;
} zk_cmt_lists;

/* roots: n_lists x 32 bytes, each as the bytes of a common.Hash; at depth 8 root i is what genRoot prints for the commitments of list i.  depth: 1..32.
 * Returns 0, or -1 with nothing written: no device, a depth out of range, a range that leaves the array, a list longer than 2^depth. */
int genRoots(const zk_cmt_lists *l, int depth, uint8_t *roots);

/* verifyBlockRecords, and then for every record i with list_of[i] >= 0: ok[i] stays 1 only if args[0] (RT) of the record equals the depth-8 root of list
 * list_of[i].  list_of[i] = -1: no root check for record i.  A record with list_of[i] >= 0 is rejected if it is no deposit record, if list_of[i] is not below
 * n_lists or if its list holds more than 256 commitments; any other negative list_of[i] rejects the record as well.  Returns the number of records accepted after the
 * root check, or -1 with every ok[i] = 0: no decision could be made, a range leaves the array, or l is NULL while some list_of[i] >= 0.  list_of: n entries, or NULL
 * for no root check at all. */
int verifyBlockRecordsRoots(const zk_block_record *recs, int n, const zk_cmt_lists *l, const int32_t *list_of, unsigned char *ok);

#ifdef __cplusplus
}
#endif
#endif
