// Launch geometry of the streaming kernels (kernels.hip, lars.hip): 256
// threads per block, grid-stride loops, the grid capped at 2048 blocks.

#pragma once

#define GEOPS_THREADS 256
#define GEOPS_MAX_BLOCKS 2048

static inline int geops_blocks(long long work, int per_thread = 1) {
  long long b = (work + (long long)GEOPS_THREADS * per_thread - 1) /
                ((long long)GEOPS_THREADS * per_thread);
  if (b < 1) b = 1;
  if (b > GEOPS_MAX_BLOCKS) b = GEOPS_MAX_BLOCKS;
  return (int)b;
}
