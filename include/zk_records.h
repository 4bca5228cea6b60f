/* Optional extension of the drop-in surface: verification of a whole block from the records as the node holds them (DESIGN.md "Block verification", "From records").
 *
 * verifyBlockRecords takes one contiguous array of fixed-size binary records — the statement as the bytes of go-ethereum's common.Hash values, the proof as the
 * 512 characters of tx.ZKProof — and decides it exactly as verifyBlock (zk_block.h) decides the equivalent item list.  Nothing is formatted as "0x..." strings
 * by the caller and nothing is parsed on the host: the hex digits become field elements and the hashes become the packed public input on the device.
 *
 * Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_RECORDS_H
#define ZK_RECORDS_H
#include <stdint.h>
#include "zk_batch.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint8_t  kind;          /* ZK_KIND_* of zk_batch.h */
  uint8_t  reserved[7];   /* ignored */
  uint64_t value_s;       /* mint / redeem; ignored for the other kinds */
  char     proof[512];    /* the 512 characters gen*proof returned, as tx.ZKProof stores them; no NUL */
  uint8_t  args[6][32];   /* the kind's verify arguments in zk_verify_item's order, each as the bytes of the common.Hash (big-endian: the order common.ToHex
                             prints); deposit's pk: its 20 bytes in args[1][0..19], the rest ignored; unused entries ignored */
} zk_block_record;        /* 720 bytes, no padding */
#ifdef __cplusplus
static_assert(sizeof(zk_block_record) == 720, "zk_block_record has no padding");
#else
_Static_assert(sizeof(zk_block_record) == 720, "zk_block_record has no padding");
#endif

/* ok[i] and the return value are what verifyBlock gives for the item list in which record i is {kind, proof = the 512 bytes and a NUL, args[k] = "0x" and the
 * lower-case hex of the 32 (pk: 20) bytes, value_s}: a proof holding any byte outside [0-9a-f] is rejected, an unknown kind is rejected.  Returns the number of
 * accepted proofs, or -1 if no decision could be made (every ok[i] is 0 then). */
int verifyBlockRecords(const zk_block_record *recs, int n, unsigned char *ok);

#ifdef __cplusplus
}
#endif
#endif
