// edv_merkle.hip -- kernels of the Merkle-tree extension (edv_merkle.h, row
// f-5), a translation unit of their own so the verify kernels' code does not
// move.  One workgroup owns one tile of kMerkleT item indices: lane j brings
// item j in (pass 0: hashes its leaf; later passes: reads the tile root the
// pass before wrote), then kMerkleLogT levels are reduced in two LDS buffers
// used in turn, one __syncthreads() per level.  Workgroups never talk to each
// other: a pass reads what the pass before wrote, and passes are separate
// launches on one stream.  The batched append (row f-6) adds one kernel after
// them: one lane per new leaf, the root after it and its audit path.  Proof
// verification (row f-7) is two kernels of the same shape: one lane per proof.
// Catch-up (row f-10) is one more after the passes: one lane per reply.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edv_merkle.h"
#include "edv_launch.h"

using namespace edv;

namespace {

template <bool kLeaves>
__global__ __launch_bounds__(kMerkleT) void edv_merkle_pass_kernel(MerklePass a, uint64_t tile0, const uint8_t* leaves,
                                                                   const uint64_t* off, uint64_t leaf_base) {
  __shared__ uint32_t lvl[2][8 * kMerkleT];  // 2 x 8 KiB
  const uint64_t tile = tile0 + blockIdx.x;
  const uint32_t j = threadIdx.x;
  uint64_t g;
  if (merkle_item_index(a, tile, j, &g)) {
    uint32_t H[8];
    if (kLeaves) {
      const uint64_t i = g - a.old_size;
      const uint64_t o0 = off[i] - leaf_base, o1 = off[i + 1] - leaf_base;
      merkle_leaf_hash(H, leaves + o0, o1 - o0);
    } else {
      merkle_load_hash(H, a.in + 8 * (g - (a.old_size >> a.h0)));
    }
    merkle_item_put(a, g, j, H, lvl[0]);
  }
#pragma unroll 1
  for (int hl = 1; hl <= kMerkleLogT; hl++) {
    __syncthreads();
    if (j < (uint32_t(kMerkleT) >> hl)) merkle_level(a, tile, hl, j, lvl[(hl - 1) & 1], lvl[hl & 1]);
  }
}

__global__ __launch_bounds__(64) void edv_merkle_finish_kernel(uint64_t old_size, uint64_t new_size,
                                                               const uint32_t* old_hashes, uint32_t* new_hashes,
                                                               uint32_t* root) {
  if (blockIdx.x == 0 && threadIdx.x == 0) merkle_finish(old_size, new_size, old_hashes, new_hashes, root);
}

// Row f-6: one lane per new leaf folds the root of the tree after it and
// copies its audit path (merkle_append_leaf), from the leaf and node hashes the
// passes before it on the stream have written.  No LDS, no lane talks to
// another; lanes of a wave differ in trip count through the low bits of s.
constexpr int kMerkleAppendLanes = 64;
__global__ __launch_bounds__(kMerkleAppendLanes) void edv_merkle_append_kernel(MerkleAppend a) {
  const uint64_t i = uint64_t(blockIdx.x) * kMerkleAppendLanes + threadIdx.x;
  if (i < a.n) merkle_append_leaf(a, i);
}

// Row f-7: one lane walks one proof (merkle_verify_inclusion_lane /
// merkle_verify_consistency_lane): a serial chain of two compressions per
// entry, so the batch is the parallelism.  As the append kernel: no LDS, no
// lane talks to another, 64-lane workgroups so that a batch of a few thousand
// proofs already spreads over the CUs; lanes of a wave differ in trip count
// (path length, leaf length) and rejoin at the status store.  With leaf bytes
// the lane hashes its own leaf first, in the same launch: a separate leaf-hash
// launch would write and re-read 32 bytes per proof and add a kernel boundary
// to save nothing, the leaf's blocks being one more serial stretch of the
// lane's chain either way.
template <bool kLeaves>
__global__ __launch_bounds__(kMerkleAppendLanes) void edv_merkle_verify_inclusion_kernel(MerkleVerifyInclusion a) {
  const uint64_t i = uint64_t(blockIdx.x) * kMerkleAppendLanes + threadIdx.x;
  if (i < a.n) merkle_verify_inclusion_lane<kLeaves>(a, i);
}
__global__ __launch_bounds__(kMerkleAppendLanes) void edv_merkle_verify_consistency_kernel(MerkleVerifyConsistency a) {
  const uint64_t i = uint64_t(blockIdx.x) * kMerkleAppendLanes + threadIdx.x;
  if (i < a.n) merkle_verify_consistency_lane(a, i);
}

// Row f-8: one lane makes one proof out of the stored hashes
// (merkle_prove_inclusion_lane / merkle_prove_consistency_lane): its stored
// entries are 32-byte copies, the one cut-off entry and the tree head come out
// of one fold of popcount(tree_size) - 1 node hashes.  The same shape again: no
// LDS, no lane talks to another, 64-lane workgroups; lanes of a wave differ in
// trip count through popcount(tree_size) and rejoin at the status store.
__global__ __launch_bounds__(kMerkleAppendLanes) void edv_merkle_prove_inclusion_kernel(MerkleProveInclusion a) {
  const uint64_t i = uint64_t(blockIdx.x) * kMerkleAppendLanes + threadIdx.x;
  if (i < a.n) merkle_prove_inclusion_lane(a, i);
}
__global__ __launch_bounds__(kMerkleAppendLanes) void edv_merkle_prove_consistency_kernel(MerkleProveConsistency a) {
  const uint64_t i = uint64_t(blockIdx.x) * kMerkleAppendLanes + threadIdx.x;
  if (i < a.n) merkle_prove_consistency_lane(a, i);
}

// Row f-9: one lane checks one stored entry (merkle_audit_node_lane: two
// 32-byte child loads, the stored node, two compressions; merkle_audit_leaf_lane:
// the leaf's blocks and one stored hash).  The same shape once more: no LDS, no
// lane reads what another wrote, 64-lane workgroups.  A node's children are
// gathers above height 1 (neighbouring positions do not have neighbouring
// children); the plain form is kept, see DESIGN.md section 3b row f-9.  The
// summary is reduced in the workgroup first: a workgroup is one wave of 64
// lanes in position order, so the ballot of the bad lanes gives the count and,
// by its lowest set bit, the lowest bad position; lane 0 of a workgroup that
// found something adds them to the caller's two words.  Every lane reaches the
// ballot.
static_assert(kMerkleAppendLanes == 64, "the audit summary takes a workgroup to be one wave of 64 lanes");
__device__ void merkle_audit_reduce(bool bad, uint64_t first_pos, uint64_t* summary) {
  const unsigned long long mask = __ballot(bad);
  if (threadIdx.x == 0 && mask != 0) {
    unsigned long long* s = reinterpret_cast<unsigned long long*>(summary);
    atomicAdd(s, static_cast<unsigned long long>(__popcll(mask)));
    atomicMin(s + 1, static_cast<unsigned long long>(first_pos + uint64_t(__ffsll(mask) - 1)));
  }
}
__global__ __launch_bounds__(kMerkleAppendLanes) void edv_merkle_audit_nodes_kernel(MerkleAuditNodes a, uint64_t* summary) {
  const uint64_t i0 = uint64_t(blockIdx.x) * kMerkleAppendLanes, i = i0 + threadIdx.x;
  const bool bad = i < a.count && merkle_audit_node_lane(a, i);
  merkle_audit_reduce(bad, a.node_lo + i0, summary);
}
__global__ __launch_bounds__(kMerkleAppendLanes) void edv_merkle_audit_leaves_kernel(MerkleAuditLeaves a, uint64_t* summary) {
  const uint64_t i0 = uint64_t(blockIdx.x) * kMerkleAppendLanes, i = i0 + threadIdx.x;
  const bool bad = i < a.n && merkle_audit_leaf_lane(a, i);
  merkle_audit_reduce(bad, a.leaf_lo + i0, summary);
}

// Row f-10: one lane per catch-up reply folds the root of the tree at the
// reply's end out of the hashes the passes before it on the stream have
// written and walks the reply's consistency proof to the target
// (merkle_catchup_lane).  The append and verify kernels' shape: no LDS, no
// lane talks to another; lanes of a wave differ in trip count through
// popcount(s) and the proof's length and rejoin at the status store.
__global__ __launch_bounds__(kMerkleAppendLanes) void edv_merkle_catchup_kernel(MerkleCatchup a) {
  const uint64_t k = uint64_t(blockIdx.x) * kMerkleAppendLanes + threadIdx.x;
  if (k < a.replies) merkle_catchup_lane(a, k);
}

}  // namespace

namespace edv {

hipError_t launch_merkle_pass_kernel(hipStream_t s, const MerklePass& a, const uint8_t* leaves, const uint64_t* off,
                                     uint64_t leaf_base) {
  const uint64_t tiles = merkle_pass_tiles(a.old_size, a.new_size, a.h0);
  if (tiles == 0) return hipSuccess;
  const uint64_t tile0 = merkle_pass_first_tile(a.old_size, a.h0);
  // a.in at height 0: the caller's leaf hashes (extend from hashes, row f-9)
  if (a.h0 == 0 && !a.in)
    edv_merkle_pass_kernel<true><<<dim3(unsigned(tiles)), dim3(kMerkleT), 0, s>>>(a, tile0, leaves, off, leaf_base);
  else
    edv_merkle_pass_kernel<false><<<dim3(unsigned(tiles)), dim3(kMerkleT), 0, s>>>(a, tile0, nullptr, nullptr, 0);
  return hipGetLastError();
}

hipError_t launch_merkle_finish_kernel(hipStream_t s, uint64_t old_size, uint64_t new_size, const uint32_t* old_hashes,
                                       uint32_t* new_hashes, uint32_t* root) {
  edv_merkle_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(old_size, new_size, old_hashes, new_hashes, root);
  return hipGetLastError();
}

hipError_t launch_merkle_append_kernel(hipStream_t s, const MerkleAppend& a) {
  if (a.n == 0 || (!a.roots && !a.paths)) return hipSuccess;
  const uint64_t blocks = (a.n + kMerkleAppendLanes - 1) / kMerkleAppendLanes;
  edv_merkle_append_kernel<<<dim3(unsigned(blocks)), dim3(kMerkleAppendLanes), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_merkle_catchup_kernel(hipStream_t s, const MerkleCatchup& a) {
  if (a.replies == 0) return hipSuccess;
  const uint64_t blocks = (a.replies + kMerkleAppendLanes - 1) / kMerkleAppendLanes;
  edv_merkle_catchup_kernel<<<dim3(unsigned(blocks)), dim3(kMerkleAppendLanes), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_merkle_verify_inclusion_kernel(hipStream_t s, const MerkleVerifyInclusion& a) {
  if (a.n == 0) return hipSuccess;
  const uint64_t blocks = (a.n + kMerkleAppendLanes - 1) / kMerkleAppendLanes;
  if (a.leaves)
    edv_merkle_verify_inclusion_kernel<true><<<dim3(unsigned(blocks)), dim3(kMerkleAppendLanes), 0, s>>>(a);
  else
    edv_merkle_verify_inclusion_kernel<false><<<dim3(unsigned(blocks)), dim3(kMerkleAppendLanes), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_merkle_verify_consistency_kernel(hipStream_t s, const MerkleVerifyConsistency& a) {
  if (a.n == 0) return hipSuccess;
  const uint64_t blocks = (a.n + kMerkleAppendLanes - 1) / kMerkleAppendLanes;
  edv_merkle_verify_consistency_kernel<<<dim3(unsigned(blocks)), dim3(kMerkleAppendLanes), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_merkle_prove_inclusion_kernel(hipStream_t s, const MerkleProveInclusion& a) {
  if (a.n == 0) return hipSuccess;
  const uint64_t blocks = (a.n + kMerkleAppendLanes - 1) / kMerkleAppendLanes;
  edv_merkle_prove_inclusion_kernel<<<dim3(unsigned(blocks)), dim3(kMerkleAppendLanes), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_merkle_prove_consistency_kernel(hipStream_t s, const MerkleProveConsistency& a) {
  if (a.n == 0) return hipSuccess;
  const uint64_t blocks = (a.n + kMerkleAppendLanes - 1) / kMerkleAppendLanes;
  edv_merkle_prove_consistency_kernel<<<dim3(unsigned(blocks)), dim3(kMerkleAppendLanes), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_merkle_audit_nodes_kernel(hipStream_t s, const MerkleAuditNodes& a, uint64_t* summary) {
  if (a.count == 0) return hipSuccess;
  const uint64_t blocks = (a.count + kMerkleAppendLanes - 1) / kMerkleAppendLanes;
  edv_merkle_audit_nodes_kernel<<<dim3(unsigned(blocks)), dim3(kMerkleAppendLanes), 0, s>>>(a, summary);
  return hipGetLastError();
}

hipError_t launch_merkle_audit_leaves_kernel(hipStream_t s, const MerkleAuditLeaves& a, uint64_t* summary) {
  if (a.n == 0) return hipSuccess;
  const uint64_t blocks = (a.n + kMerkleAppendLanes - 1) / kMerkleAppendLanes;
  edv_merkle_audit_leaves_kernel<<<dim3(unsigned(blocks)), dim3(kMerkleAppendLanes), 0, s>>>(a, summary);
  return hipGetLastError();
}

}  // namespace edv
