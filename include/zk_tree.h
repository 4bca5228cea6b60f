/* Optional extension of the drop-in surface: the commitment tree of the deposit circuit kept resident next to the prover (DESIGN.md "Commitment tree").
 *
 * genRoot and genDepositproof take the whole list of commitments as one hex string on every call and are fixed at Merkle depth 8 (256 commitments).  A zk_tree
 * is the same tree — SHA-256 compression nodes, all-zero unseen leaves — of any depth from 1 to 32, held in device memory: it is appended to as blocks arrive and
 * answers root and path queries without seeing the list again.  genDepositproofTree proves against it at the tree's depth, verifyDepositproofDepth verifies at a
 * given depth.  Keys: depth 8 uses depositpk.txt / depositvk.txt, any other depth d deposit<d>pk.txt / deposit<d>vk.txt in the same directory (ZK_PRFKEY_DIR).
 * Calls may arrive concurrently on any thread; every call sees one state of the tree.
 *
 * Exported by libzkgpu.so only: a caller that wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_TREE_H
#define ZK_TREE_H
#include <stdbool.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct zkgpu_tree zk_tree;
zk_tree *zkTreeNew(int depth);                               /* NULL on failure (no device, depth outside 1..32) */
void     zkTreeFree(zk_tree *t);
/* cmtarray in genRoot's format: n items of 66 characters ("0x" + 64 hex digits).  Returns the new number of leaves, -1 on failure; a call that would
 * take the tree beyond 2^depth leaves fails and changes nothing. */
long long zkTreeAppend(zk_tree *t, char *cmtarray, int n);
char    *zkTreeRoot(zk_tree *t);                             /* 64 hex characters, malloc'd like genRoot's; at depth 8 equal to genRoot over the same leaves */
/* genDepositproof's arguments without cmtarray / n / RT.  rt_out receives the 64 hex digits + NUL of the root the proof was made against: the tree may grow
 * between a caller's zkTreeRoot and its proof, and only this call knows which state its path came from.
 * Failure (cmtS is not in the tree, no key for the tree's depth, a statement that violates the circuit): the reference's sentinel proof, as genDepositproof,
 * and rt_out[0] = 0. */
char *genDepositproofTree(uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *sns, char *rs, char *cmtB_old,
                          char *cmtB, uint64_t value_s, char *pk, char *sn_A_old, char *cmtS, char *sk, zk_tree *t, char rt_out[65]);
/* verifyDepositproof with the key of the given Merkle depth */
bool  verifyDepositproofDepth(int depth, char *data, char *RT, char *pk, char *cmtb_old, char *snold, char *cmtb, char *sns);

#ifdef __cplusplus
}
#endif
#endif
