// devpaths.hip - post-loop path extraction on the device: SpaceForest::getPaths (src/forest.h:420-462) and
// Solver::getAllPaths (src/problemStruct.h:184-253) for every forest of a batch in ONE launch (devpaths.h: PathsArgs).
// On the host the same two steps are Forest::get_paths / get_all_paths (paths.cpp) over a downloaded forest; here they read
// the device engine's own arrays, and only the plans and the positions of their entries go down.
//
// k_paths_batch, workgroup b (256 threads) = member b, its arguments through the uniform pointer.  Stages, a workgroup
// barrier between them:
//   0  connectedTrees (src/forest.h:379-418) over the pair matrix, serial on thread 0: its order decides the closure's order
//   1  getPaths: every border's cost d_root[n1] + d_root[n2] + dist6 rewritten (one thread per border); per pair of trees
//      the flat border list scanned in list order with the reference's pick (paths_rules.h: not an argmin); the two root
//      chains of every picked border walked side by side, one thread per chain, a node's parent and d_root issued together -
//      once for the lengths (the plan's place in the pool), once to write node1's chain reversed and node2's behind it
//   2  getAllPaths: the k loop in sequence; for one k a step reads only rows that involve connected[k] and writes only rows
//      that do not, so the unordered pairs {a, b} of one k are independent items, a thread each: the order that comes first
//      in the reference's loop (a before b in connectedTrees), then the other; strip, cost and acceptance are paths_rules.h's
//   3  the surviving plans and the fp64 position of every plan entry packed behind a small header
// Plans live in a per-member pool handed out by one counter in LDS; a replaced plan's entries are not taken back.  A member
// whose pool runs out says so in its header (SFFK_PATHS_POOL_FULL) and the host route finishes it.  Every id is checked
// against the arrays' extents before it is followed (SFFK_PATHS_BAD_STATE): nothing is read or written out of bounds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "devpaths.h"
#include "paths_rules.h"

namespace sffk {

namespace {

#define PATHS_DBL_MAX 1.7976931348623157e308

// the member's status as every thread of the workgroup sees it between two stages: read between two barriers, so that no
// thread reads it after another one has already changed it in the next stage (the stages' own barriers hang on it)
__device__ __forceinline__ int stage_status(const int* s_status) {
  __syncthreads();
  const int st = *(const volatile int*)s_status;
  __syncthreads();
  return st;
}

__device__ __forceinline__ int row_of(int a, int b, int T) { return a < b ? a * T + b : b * T + a; }

// one order of a closure item: the paths x -> id3 and y -> id3 joined, the row (x, y) replaced if the join is shorter
__device__ __forceinline__ void closure_try(const PathsArgs& A, int x, int y, int id3, int* s_pool, int* s_status) {
  const int T = A.n_trees;
  const PathRow r1 = A.rows[row_of(x, id3, T)], r2 = A.rows[row_of(y, id3, T)];
  if (r1.n1 < 0 || r2.n1 < 0) return;
  const bool f1 = A.stree[r1.n1] == x, f2 = A.stree[r2.n1] == y;
  const int node1 = f1 ? r1.n1 : r1.n2, node2 = f2 ? r2.n1 : r2.n2;
  const sffr::PlanView p1{A.pool + r1.off, r1.len, f1}, p2{A.pool + r2.off, r2.len, f2};
  const double* spos = A.spos;
  sffr::Join J;
  if (!sffr::join_plans(p1, p2, [spos](int node) { return spos + 6 * (size_t)node; }, J)) return;
  PathRow* cur = A.rows + row_of(x, y, T);
  if (!sffr::join_accepts(J.dist, cur->dist)) return;
  const int off = atomicAdd(s_pool, J.len);
  if (off < 0 || off + J.len > A.pool_cap) { atomicMax(s_status, SFFK_PATHS_POOL_FULL); return; }
  const bool fwd = sffr::join_stored_forward(node1, node2);
  for (int q = 0; q < J.len; ++q) A.pool[off + (fwd ? q : J.len - 1 - q)] = sffr::join_at(p1, p2, J, q);
  cur->n1 = fwd ? node1 : node2;
  cur->n2 = fwd ? node2 : node1;
  cur->off = off;
  cur->len = J.len;
  cur->dist = J.dist;
}

}  // namespace

__global__ __launch_bounds__(SFFK_PATHS_THREADS) void k_paths_batch(const PathsArgs* __restrict__ members, int n) {
  if ((int)blockIdx.x >= n) return;
  const PathsArgs A = members[blockIdx.x];
  __shared__ int s_status, s_pool, s_nn, s_nb, s_nc, s_rows, s_entries;
  __shared__ int s_conn[SFFK_PATHS_MAX_TREES], s_stack[SFFK_PATHS_MAX_TREES];
  __shared__ uint8_t s_flag[SFFK_PATHS_MAX_TREES];
  const int tid = threadIdx.x, NT = SFFK_PATHS_THREADS, T = A.n_trees;

  // ---- stage 0: counts, connectedTrees
  if (tid == 0) {
    const int nn = A.ctrl->n_nodes, nb = A.ctrl->n_borders;
    s_nn = nn; s_nb = nb; s_pool = 0; s_nc = 0; s_rows = 0; s_entries = 0;
    s_status = SFFK_PATHS_OK;
    if (T < 1 || T > SFFK_PATHS_MAX_TREES || nn < 0 || nn > A.node_cap || nb < 0 || nb > A.border_cap || A.pool_cap < 0) {
      s_status = SFFK_PATHS_BAD_STATE;
    } else {
      for (int i = 0; i < T; ++i) s_flag[i] = 0;
      int max_conn = 0, remaining = T, unconnected = 0, nc = 0;
      while (max_conn < remaining) {
        nc = 0;
        int top = 0;
        s_stack[top++] = unconnected;
        s_flag[unconnected] = 1;
        while (top > 0) {
          const int root = s_stack[--top];   // (the reference's list is popped and pushed at its front)
          s_conn[nc++] = root;
          for (int i = 0; i < T; ++i) {
            if (root == i || s_flag[i]) continue;
            if (A.pair[row_of(root, i, T)]) { s_flag[i] = 1; s_stack[top++] = i; }
          }
        }
        max_conn = nc;
        for (int i = 0; i < T; ++i)
          if (!s_flag[i]) { unconnected = i; break; }
        remaining -= max_conn;
      }
      s_nc = nc;
    }
  }
  if (stage_status(&s_status) == SFFK_PATHS_OK) {
    const int nn = s_nn, nb = s_nb;
    for (int p = tid; p < T * T; p += NT) {
      PathRow r;
      r.n1 = r.n2 = -1; r.off = r.len = 0; r.dist = PATHS_DBL_MAX; r.aux = r.pad = 0;
      A.rows[p] = r;
    }
    // ---- stage 1a: every border's cost (DistanceHolder::UpdateDistance)
    for (int e = tid; e < nb; e += NT) {
      const int n1 = A.b_n1[e], n2 = A.b_n2[e], ta = A.b_ta[e], tb = A.b_tb[e];
      if (n1 < 0 || n1 >= nn || n2 < 0 || n2 >= nn || ta < 0 || ta >= T || tb < 0 || tb >= T || ta == tb) {
        atomicMax(&s_status, SFFK_PATHS_BAD_STATE);
        continue;
      }
      A.b_dist[e] = sffr::border_dist(A.d_root[n1], A.d_root[n2], A.spos + 6 * (size_t)n1, A.spos + 6 * (size_t)n2);
    }
  }
  if (stage_status(&s_status) == SFFK_PATHS_OK) {
    // ---- stage 1b: the pick of every pair, in list order
    const int nb = s_nb;
    for (int p = tid; p < T * T; p += NT) {
      const int i = p / T, j = p % T;
      if (i >= j || !A.pair[p]) continue;
      double best = -1;
      int bn1 = -1, bn2 = -1;
      for (int e = 0; e < nb; ++e) {
        const int ta = A.b_ta[e], tb = A.b_tb[e];
        if (!((ta == i && tb == j) || (ta == j && tb == i))) continue;
        const double d = A.b_dist[e];
        if (sffr::border_takes(best, d)) { best = d; bn1 = A.b_n1[e]; bn2 = A.b_n2[e]; }
      }
      if (bn1 >= 0) { A.rows[p].n1 = bn1; A.rows[p].n2 = bn2; A.rows[p].dist = best; }
    }
  }
  if (stage_status(&s_status) == SFFK_PATHS_OK) {
    // ---- stage 1c: the lengths of the two root chains of every picked border (off: node1's, len: node2's, for now)
    const int nn = s_nn;
    for (int c = tid; c < 2 * T * T; c += NT) {
      const int p = c >> 1, side = c & 1;
      if (p / T >= p % T || A.rows[p].n1 < 0) continue;
      int node = side ? A.rows[p].n2 : A.rows[p].n1, len = 0;
      bool bad = false;
      while (true) {
        if (node < 0 || node >= nn || len >= nn) { bad = true; break; }
        const double dr = A.d_root[node];
        const int par = A.parent[node];
        ++len;
        if (dr == 0) break;                      // Node::IsRoot
        node = par;
      }
      if (bad) { atomicMax(&s_status, SFFK_PATHS_BAD_STATE); len = 0; }
      if (side) A.rows[p].len = len; else A.rows[p].off = len;
    }
  }
  if (stage_status(&s_status) == SFFK_PATHS_OK) {
    for (int p = tid; p < T * T; p += NT) {
      if (p / T >= p % T || A.rows[p].n1 < 0) continue;
      const int len1 = A.rows[p].off, total = len1 + A.rows[p].len;
      const int off = atomicAdd(&s_pool, total);
      if (off < 0 || off + total > A.pool_cap) { atomicMax(&s_status, SFFK_PATHS_POOL_FULL); continue; }
      A.rows[p].aux = len1;
      A.rows[p].off = off;
      A.rows[p].len = total;
    }
  }
  if (stage_status(&s_status) == SFFK_PATHS_OK) {
    // ---- the chains again, written: node1 back to its root reversed, then node2 forward to its root
    for (int c = tid; c < 2 * T * T; c += NT) {
      const int p = c >> 1, side = c & 1;
      if (p / T >= p % T || A.rows[p].n1 < 0) continue;
      const int len1 = A.rows[p].aux, off = A.rows[p].off, len = side ? A.rows[p].len - len1 : len1;
      int node = side ? A.rows[p].n2 : A.rows[p].n1;
      for (int s = 0; s < len; ++s) {            // (the lengths are the first walk's: every node was in range)
        const int par = A.parent[node];
        A.pool[off + (side ? len1 + s : len1 - 1 - s)] = node;
        node = par;
      }
    }
  }
  // ---- stage 2: getAllPaths
  const int st2 = stage_status(&s_status);
  const int nc = s_nc;
  if (st2 == SFFK_PATHS_OK) {
    for (int k = 0; k < nc; ++k) {
      const int id3 = s_conn[k];
      for (int item = tid; item < nc * nc; item += NT) {
        const int i = item / nc, j = item % nc;
        if (i >= j || i == k || j == k) continue;
        if (*(volatile int*)&s_status != SFFK_PATHS_OK) continue;
        closure_try(A, s_conn[i], s_conn[j], id3, &s_pool, &s_status);
        closure_try(A, s_conn[j], s_conn[i], id3, &s_pool, &s_status);
      }
      __threadfence_block();
      __syncthreads();
    }
  }
  // ---- stage 3: the answer, packed
  const int st3 = stage_status(&s_status);
  if (st3 == SFFK_PATHS_OK && tid == 0) {
    PathRowOut* out = reinterpret_cast<PathRowOut*>(A.packed);
    int rows = 0, entries = 0;
    for (int p = 0; p < T * T; ++p) {
      if (p / T >= p % T || A.rows[p].n1 < 0) continue;
      const PathRow r = A.rows[p];
      PathRowOut o;
      o.i = p / T; o.j = p % T; o.n1 = r.n1; o.n2 = r.n2; o.len = r.len; o.pad = 0; o.dist = r.dist;
      out[rows++] = o;
      A.rows[p].aux = entries;
      entries += r.len;
    }
    s_rows = rows;
    s_entries = entries;
  }
  if (stage_status(&s_status) == SFFK_PATHS_OK) {
    const int rows = s_rows, entries = s_entries;
    int32_t* ids = reinterpret_cast<int32_t*>(A.packed + (size_t)rows * sizeof(PathRowOut));
    double* pos = reinterpret_cast<double*>(A.packed + (size_t)rows * sizeof(PathRowOut) + (((size_t)entries * 4 + 7) & ~(size_t)7));
    for (int p = 0; p < T * T; ++p) {
      if (p / T >= p % T || A.rows[p].n1 < 0) continue;
      const int off = A.rows[p].off, len = A.rows[p].len, at = A.rows[p].aux;
      for (int q = tid; q < len; q += NT) {
        const int id = A.pool[off + q];
        ids[at + q] = id;
        for (int a = 0; a < 6; ++a) pos[6 * (size_t)(at + q) + a] = A.spos[6 * (size_t)id + a];
      }
    }
    if (tid == 0 && (entries & 1)) ids[entries] = 0;   // (the padding word goes down too)
  }
  if (tid == 0) {
    PathsHead* h = A.head;
    h->status = st3;
    h->n_connected = st3 == SFFK_PATHS_OK ? nc : 0;
    h->n_rows = st3 == SFFK_PATHS_OK ? s_rows : 0;
    h->n_entries = st3 == SFFK_PATHS_OK ? s_entries : 0;
    h->pool_used = s_pool;
    h->n_nodes = s_nn;
    h->n_borders = s_nb;
    h->pad = 0;
    for (int i = 0; i < SFFK_PATHS_MAX_TREES; ++i) h->connected[i] = i < nc ? s_conn[i] : -1;
  }
}

hipError_t launch_paths_batch(hipStream_t s, const PathsArgs* members_dev, int n) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_paths_batch, dim3(n), dim3(SFFK_PATHS_THREADS), 0, s, members_dev, n);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_paths_gather(const PathsGather* __restrict__ parts, int n) {
  if ((int)blockIdx.x >= n) return;
  const PathsGather g = parts[blockIdx.x];
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(g.src);
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(g.dst);
  for (unsigned long long w = threadIdx.x; w < g.bytes / 8; w += 256) dst[w] = src[w];
}

hipError_t launch_paths_gather(hipStream_t s, const PathsGather* parts_dev, int n) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_paths_gather, dim3(n), dim3(256), 0, s, parts_dev, n);
  return hipGetLastError();
}

}  // namespace sffk
