// The AdamBlock protocol of adamw_step_kernel (adamw.hip's header: "Who writes the block") for the
// update kernels of the flat-arena compressors (signsgd.hip, quant.hip, topk.hip), which step with
// the AdamW element rule of adamw_elem.h behind their decompressed average.
//
//   adam_block_read     every thread, BEFORE the workgroup's barrier: thread 0 reads b1pow / b2pow /
//                       steps (uniform address: scalar loads) and leaves the two products' inputs in
//                       LDS for the other waves.  No wave reads the block after it.
//   adam_launch_scalars (adamw_elem.h) behind that barrier, from pow_sh: the same in every workgroup.
//   adam_block_advance  every thread, behind its stores: thread 0 draws the two-level arrival ticket
//                       (arrival.h); the last arriver of the grid, which every workgroup's read
//                       precedes, writes {p1, p2, steps + 1, 0} with plain stores and re-arms the
//                       ticket.  No workgroup waits for another, nothing of a workgroup's stores is
//                       read by another (no drain), and a replayed graph finds the ticket zeroed.
#pragma once
#include <hip/hip_runtime.h>

#include "adamw_elem.h"
#include "arrival.h"
#include "ndp_kernels.h"

namespace ndp {

// pow_sh: 2 floats of LDS.  Returns steps in thread 0 (0 elsewhere).
__device__ __forceinline__ unsigned adam_block_read(const AdamBlock* block, float* pow_sh) {
  unsigned steps = 0;
  if (threadIdx.x == 0) {
    pow_sh[0] = block->b1pow;
    pow_sh[1] = block->b2pow;
    steps = block->steps;
  }
  return steps;
}

__device__ __forceinline__ void adam_block_advance(unsigned* ctr, AdamBlock* block, float p1, float p2,
                                                   unsigned steps) {
  if (threadIdx.x != 0 || !arrive_last_grouped(ctr)) return;
  // last arriver: every workgroup has drawn its ticket, hence read the block
  block->b1pow = p1;
  block->b2pow = p2;
  block->steps = steps + 1u;
  block->pad = 0u;
  arrive_rearm(ctr);
}

}  // namespace ndp
