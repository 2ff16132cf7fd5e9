// devpaths.h — path extraction on the device (devpaths.hip, driven by paths_batch.cpp): getPaths + getAllPaths for every
// forest of a batch in ONE launch, one workgroup per forest.  What a member hands the kernel, and what comes back.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace sffk {

#define SFFK_PATHS_OK 0
#define SFFK_PATHS_POOL_FULL 1     // the plan pool ran out: the host route finishes this member
#define SFFK_PATHS_BAD_STATE 2     // a count or an id lies outside the arrays: nothing was followed, the member fails
#define SFFK_PATHS_MAX_TREES 64    // (a lane per tree, the one-wavefront loops' bound)
#define SFFK_PATHS_THREADS 256

// One pair's row of the neighbouring matrix while the kernel works (HBM, n_trees x n_trees, used where i < j)
struct PathRow {
  int32_t n1, n2;     // n1 < 0: no path
  int32_t off, len;   // the plan: pool[off, off + len)
  double dist;
  int32_t aux, pad;   // stage scratch: node1's chain length, then the plan's first entry in the packed answer
};
// ... and as it comes down: only the pairs with a path, in row-major order; their plans follow back to back
struct PathRowOut {
  int32_t i, j, n1, n2;
  int32_t len, pad;
  double dist;
};
// Header of a member's answer (one per member, contiguous for the whole call: the first, small copy)
struct PathsHead {
  int32_t status;                 // SFFK_PATHS_*
  int32_t n_connected, n_rows, n_entries;
  int32_t pool_used, n_nodes, n_borders, pad;
  int32_t connected[SFFK_PATHS_MAX_TREES];
};
// the packed answer of a member behind its header: PathRowOut[n_rows] | int32 ids[n_entries] (padded to 8 bytes) |
// double pos[6 * n_entries]
inline size_t paths_packed_bytes(int n_rows, int n_entries) {
  return (size_t)n_rows * sizeof(PathRowOut) + (((size_t)n_entries * 4 + 7) & ~(size_t)7) + (size_t)n_entries * 48;
}

struct PathsArgs {
  const DevCtrl* ctrl;            // n_nodes, n_borders
  const double* spos;             // Ctx::spos
  const int32_t* stree;           // Ctx::stree
  const int32_t* parent;          // DevEngine::parent, d_root
  const double* d_root;
  const int32_t *b_n1, *b_n2, *b_ta, *b_tb;
  double* b_dist;                 // rewritten: DistanceHolder::UpdateDistance of every border
  const uint8_t* pair;            // n_trees x n_trees
  PathRow* rows;                  // n_trees x n_trees
  int32_t* pool;                  // pool_cap plan entries
  char* packed;                   // room for paths_packed_bytes(n_trees (n_trees - 1) / 2, pool_cap)
  PathsHead* head;
  int32_t n_trees, pool_cap, node_cap, border_cap;
};
hipError_t launch_paths_batch(hipStream_t s, const PathsArgs* members_dev, int n);

// the used parts of the members' answers into one contiguous block (the second copy): 8-byte words
struct PathsGather {
  const char* src;
  char* dst;
  unsigned long long bytes;       // a multiple of 8
};
hipError_t launch_paths_gather(hipStream_t s, const PathsGather* parts_dev, int n);

}  // namespace sffk
