// knn_dev.h - the one copy of what the exact k-nearest kernels share: k_knn_grid, knn_wg_search / k_knn_grid_wg (which
// spells two of the idioms out, see there),
// k_star_knn_wg (kernels.hip) and k_star_knn (devstar.hip).  Include behind kernels_dev.h (TopK, grid_coord, star_accepted)
// and star_pass_dev.h (STAR_INF, STAR_FAULT ...).
//   cells     : the cells of shell r / of the cube of half-width r around a cell, a cell's index and fill count, the end of a
//               shell search
//   lanes     : items of up to 64 cells dealt over the lanes (inclusive scan, owner lane of flat index j)
//   overflow  : a grid's shared overflow list ranked into a TopK
//   SFF*      : what follows the store search of an accepted sample - the same text for both star kernels
// Everything decides parity with the reference (same keys, same tie order): a change here reaches every kernel at once.
// All of it is __forceinline__ and takes the site's own predicate as a functor: no calls, the registers, LDS and
// occupancy classes the kernels' own copies had (profiles/knn_idioms_codegen.md; timing: profiles/README.md).
#pragma once

namespace sffk {

using namespace sffg;

// ------------------------------------------------------------------ cells
// Shell r >= 1 around a cell = the cube of half-width r minus the cube of half-width r - 1: two caps of w x w cells
// (w = 2 r + 1) and w - 2 rings of 8 r cells in between.  (Shell 0 is the cell itself: one cell, offset 0 - shell_cell gives it, the count is the caller's.)
struct Shell {
  int r, w, ww, ring, cells;   // (the dimensions once per shell, not once per cell)
};
__device__ __forceinline__ Shell shell_of(int r) {
  const int w = 2 * r + 1;
  const int ww = w * w, ring = 8 * r;
  return Shell{r, w, ww, ring, 2 * ww + (w - 2) * ring};
}
// offset of cell c of the shell
__device__ __forceinline__ void shell_cell(const Shell& s, int c, int& ox, int& oy, int& oz) {
  const int r = s.r, w = s.w, ww = s.ww, ring = s.ring;
  if (c < 2 * ww) {
    const int face = c >= ww ? 1 : 0, i = c - face * ww;
    ox = i % w - r; oy = i / w - r; oz = face ? r : -r;
  } else {
    const int cc = c - 2 * ww;
    const int layer = cc / ring, pp = cc - layer * ring;
    const int side = pp / (2 * r), t_ = pp - side * 2 * r;
    oz = -r + 1 + layer;
    ox = side == 0 ? -r + t_ : side == 1 ? r : side == 2 ? r - t_ : -r;
    oy = side == 0 ? -r : side == 1 ? -r + t_ : side == 2 ? r : r - t_;
  }
}
// cell c of the (2 r + 1)^3 cube of half-width r around the cell (cx, cy, cz)
__device__ __forceinline__ void cube_cell(int cx, int cy, int cz, int r, int c, int& x, int& y, int& z) {
  const int w = 2 * r + 1;
  x = cx + c % w - r; y = cy + (c / w) % w - r; z = cz + c / (w * w) - r;
}
// is (x, y, z) a cell of the grid, and which
__device__ __forceinline__ bool grid_cell_in(const GridView& g, int x, int y, int z, int& cell) {
  if (!(x >= 0 && x < g.nx && y >= 0 && y < g.ny && z >= 0 && z < g.nz)) return false;
  cell = (z * g.ny + y) * g.nx + x;
  return true;
}
// ... and its fill count in cg (a grid of g's shape: g itself, or the round's own grid), no more than a bucket holds; both
// stay as they are outside the grid.  OCC: cg's occupancy bits, where it has them, answer for the empty cells.
template <bool OCC = false>
__device__ __forceinline__ void grid_cell_fill(const GridView& g, const GridView& cg, int x, int y, int z, int& cell, int& m) {
  if (grid_cell_in(g, x, y, z, cell)) {
    if constexpr (OCC) {
      const bool maybe = cg.occ ? ((cg.occ[cell >> 5] >> (cell & 31)) & 1u) != 0 : true;
      if (maybe) { m = cg.cnt[cell]; if (m > cg.bk) m = cg.bk; }
    } else {
      m = cg.cnt[cell];
      if (m > cg.bk) m = cg.bk;
    }
  }
}
// The end of a shell search, after shell r: every node within shells_reach of the query has been seen (r cells minus
// the fp32 slack: cells are assigned from fp32 coordinates) - a full list whose k-th distance lies inside is final - or
// the cube of half-width r covers the whole grid.
__device__ __forceinline__ double shells_reach(int r, double cell_edge, double slack) { return (double)r * cell_edge - slack; }
__device__ __forceinline__ bool shells_cover_grid(const GridView& g, int cx, int cy, int cz, int r) {
  if (cx - r <= 0 && cy - r <= 0 && cz - r <= 0 && cx + r >= g.nx - 1 && cy + r >= g.ny - 1 && cz + r >= g.nz - 1) return true;
  return false;   // (a branch, as the kernels had it: with `return a && b ...` k_knn_grid_wg's stream is no longer the parent's)
}

// ------------------------------------------------------------------ lanes
// Items of up to 64 cells (lane = cell, m = its item count) dealt over the lanes: inc = inclusive prefix sum of m,
// __shfl(inc, 63) items in all; flat item jj belongs to the first lane whose inc exceeds it (six steps of bisection) and
// is that lane's item number lane_slot.  (grid_ball_items, kernels_dev.h, keeps the one-slot loops' copy.)
__device__ __forceinline__ int lane_scan_incl(int m, int lane) {
  int inc = m;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  return inc;
}
__device__ __forceinline__ int lane_owner(int inc, int jj) {
  int lo = 0, hi = 63;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (__shfl(inc, mid) > jj) hi = mid; else lo = mid + 1;
  }
  return lo;
}
__device__ __forceinline__ int lane_slot(int inc, int m, int jj, int owner) { return jj - (__shfl(inc, owner) - __shfl(m, owner)); }

// ------------------------------------------------------------------ overflow
// A grid's shared overflow list (usually empty) into the list.  One batch: this lane's entry *src, if valid;
// accept(id, tree) = the item is asked for; LIMITED: and not farther than `limit`.  have (the list's fill) goes in and
// comes back by value: by reference it leaves the scalar registers in the loop.
template <bool LIMITED = false, class Accept>
__device__ __forceinline__ int ovf_batch(bool valid, const GridItem* src, int lane, const double* qp, TopK& t, int k, int have,
                                          Accept&& accept, double limit = 0.0) {
  bool cand = false;
  double d = 1.0e300;
  int id = 0x7fffffff;
  const double worst = topk_worst(t, k, have);   // (a shuffle: outside the divergent code below)
  if (valid) {
    const GridItem it = *src;
    id = it.id;
    if (accept(id, it.tree)) {
      d = dist6(it.p, qp);
      if constexpr (LIMITED) cand = d <= limit && (have < k || key_less(d, id, worst, 0x7fffffff));
      else cand = have < k || key_less(d, id, worst, 0x7fffffff);
    }
  }
  topk_insert(t, lane, k, have, __ballot(cand), d, id);
  return have;
}
// the list's `no` entries from `first` on, `stride` apart (a wavefront's batches of 64)
template <bool LIMITED = false, class Accept>
__device__ __forceinline__ int ovf_scan_n(const GridItem* ovf, int no, int first, int stride, int lane, const double* qp, TopK& t, int k,
                                          int have, Accept&& accept, double limit = 0.0) {
  for (int base = first; base < no; base += stride) {
    const int j = base + lane;
    have = ovf_batch<LIMITED>(j < no, ovf + j, lane, qp, t, k, have, accept, limit);
  }
  return have;
}
template <bool LIMITED = false, class Accept>
__device__ __forceinline__ int ovf_scan(const GridView& g, int first, int stride, int lane, const double* qp, TopK& t, int k, int have,
                                         Accept&& accept, double limit = 0.0) {
  int no = g.ovf_cnt[0];
  if (no > g.ovf_cap) no = g.ovf_cap;
  return ovf_scan_n<LIMITED>(g.ovf, no, first, stride, lane, qp, t, k, have, accept, limit);
}

// ------------------------------------------------------------------ SFF*: an accepted sample after its store search
#define STAR_MATE_U 16                              // x 64 accepted samples of a round whose list is scanned from registers

// launch-wide: the passes' change flags, k_star_tail's barrier and verdict, the sublists
__device__ __forceinline__ void star_launch_reset(const StarView& S) {
  if (blockIdx.x == 0 && threadIdx.x < SFFK_STAR_PASSES) S.changed[threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) { S.changed[SFFK_STAR_BAR] = 0; S.hdr[STAR_PASSES_RUN] = 0; S.hdr[STAR_CONVERGED] = 0; }   // (k_star_tail)
  for (int t = blockIdx.x * 256 + threadIdx.x; t < SFFK_STAR_PASSES * SFFK_SUBLISTS * SFFK_STAR_SUB; t += gridDim.x * 256) S.sub[t] = 0;
}
// k = (size_t)(2e log10(#nodes)) with the nodes accepted before this sample counted in (src/forest.h:309)
__device__ __forceinline__ int star_k(const StarView& S, int Nn, int lane) {
  return __popcll(__ballot(lane > 0 && lane <= SFFK_STAR_KMAX + 1 && S.ktab[lane] <= Nn));
}
// The earlier accepted samples of the round (ranks below r), asked for beside the search: rank -> sample (sidv), then
// sample -> tree (trv) - two dependent trips that would otherwise follow the search.  on: this wavefront will run the stage.
__device__ __forceinline__ void star_earlier_ids(const StarView& S, int Tb, int r, int lane, bool on, int (&sidv)[STAR_MATE_U]) {
  const bool mates_small = on && r > 0 && r <= 64 * STAR_MATE_U;
#pragma unroll
  for (int u = 0; u < STAR_MATE_U; ++u) { const int rq = 64 * u + lane; sidv[u] = (mates_small && rq < r) ? Tb + S.acc_sample[rq] : -1; }
}
__device__ __forceinline__ void star_earlier_trees(const NodeStoreView& st, const int (&sidv)[STAR_MATE_U], int (&trv)[STAR_MATE_U]) {
#pragma unroll
  for (int u = 0; u < STAR_MATE_U; ++u) trv[u] = sidv[u] >= 0 ? st.tree[sidv[u]] : -1;
}

// candidates of a group of up to 64 cells of the round's own grid (lane = cell, m = its item count): samples accepted
// EARLIER in the round (temporary id in [Tb, self)) of the same tree, not farther than `limit`
__device__ __forceinline__ void star_cells_mates(const GridView& tg, int m, int cell, int lane, const double* qp, int tree, int Tb,
                                                 int self, double limit, const DevForestView& f, TopK& t, int k, int& have) {
  const int inc = lane_scan_incl(m, lane);
  const int total = __shfl(inc, 63);
  for (int base = 0; base < total; base += 64) {
    const int j = base + lane;
    const int jj = j < total ? j : total - 1;
    const int lo = lane_owner(inc, jj);
    const int src_cell = __shfl(cell, lo);
    const int slot = lane_slot(inc, m, jj, lo);
    bool cand = false;
    double d = 1.0e300;
    int id = 0x7fffffff;
    if (j < total) {
      const GridItem it = tg.items[(size_t)src_cell * tg.bk + slot];
      id = it.id;
      int rk;
      if (it.tree == tree && id >= Tb && id < self && star_accepted(f, id - Tb, rk)) {
        d = sffg::dist6(it.p, qp);
        cand = d <= limit;
      }
    }
    const double worst = topk_worst(t, k, have);
    cand = cand && (have < k || key_less(d, id, worst, 0x7fffffff));
    topk_insert(t, lane, k, have, __ballot(cand), d, id);
  }
}

// The samples accepted earlier in this round (ranks below r, k_commit's list) of the same tree join the list of the k
// nearest store nodes (t, have): those not farther than the k-th store node - or, while the store holds fewer than k nodes
// of the tree, all of them.  One wavefront; ml: its LDS buffer of 64 * STAR_MATE_U ids; sidv / trv: star_earlier_ids / _trees;
// (cx, cy, cz): the sample's cell in the node grid g, whose shape the round's own grid tg shares.
__device__ __forceinline__ void star_earlier_samples(const StarView& S, const DevForestView& f, const GridView& g, const GridView& tg,
                                                     const NodeStoreView& st, const double* qp, int mine, int Tb, int self, int r,
                                                     const int (&sidv)[STAR_MATE_U], const int (&trv)[STAR_MATE_U], int* ml,
                                                     int cx, int cy, int cz, int rmax, double cell_edge, double slack, int lane,
                                                     TopK& t, int k, int& have) {
  if (r <= 0) return;
  const bool all = have < k;
  const double limit = all ? 1.0e300 : topk_worst(t, k, have);
  if (r <= 64 * STAR_MATE_U) {
    // k_commit's list of the accepted samples: every rank's sample and tree were requested up front (two trips to
    // memory whatever the length), the few of the same tree are compacted in LDS and measured a batch at a time
    int nm = 0;
#pragma unroll
    for (int u = 0; u < STAR_MATE_U; ++u) {
      if (64 * u >= r) break;
      const bool mt = sidv[u] >= 0 && trv[u] == mine;
      const unsigned long long mm = __ballot(mt);
      if (mt) ml[nm + __popcll(mm & ((1ULL << lane) - 1ULL))] = sidv[u];
      nm += __popcll(mm);
    }
    __builtin_amdgcn_wave_barrier();
    for (int base = 0; base < nm; base += 64) {
      const int j = base + lane;
      bool cand = false;
      double d = 1.0e300;
      int sid = 0x7fffffff;
      if (j < nm) {
        sid = ml[j];
        double mp[6];
        for (int q = 0; q < 6; ++q) mp[q] = st.pos[6 * (size_t)sid + q];
        d = dist6(mp, qp);
        cand = d <= limit;
      }
      const double worst = topk_worst(t, k, have);
      cand = cand && (have < k || key_less(d, sid, worst, 0x7fffffff));
      topk_insert(t, lane, k, have, __ballot(cand), d, sid);
    }
  } else if (all) {
    for (int base = 0; base < r; base += 64) {   // (a tree wanted whole in a huge round: rare)
      const int rq = base + lane;
      bool cand = false;
      double d = 1.0e300;
      int sid = 0x7fffffff;
      if (rq < r) {
        sid = Tb + S.acc_sample[rq];
        if (st.tree[sid] == mine) {
          double mp[6];
          for (int q = 0; q < 6; ++q) mp[q] = st.pos[6 * (size_t)sid + q];
          d = dist6(mp, qp);
          cand = true;
        }
      }
      const double worst = topk_worst(t, k, have);
      cand = cand && (have < k || key_less(d, sid, worst, 0x7fffffff));
      topk_insert(t, lane, k, have, __ballot(cand), d, sid);
    }
  } else {
    // a large round: the round's own grid, cells of the cube around the ball of the k-th store node
    int rr = (int)((limit + slack) / cell_edge) + 1;
    if (rr > rmax) rr = rmax;
    const int w = 2 * rr + 1;
    const int total = w * w * w;
    for (int c0 = 0; c0 < total; c0 += 64) {
      const int cc = c0 + lane;
      int cell = 0, m = 0;
      if (cc < total) {
        int x, y, z;
        cube_cell(cx, cy, cz, rr, cc, x, y, z);
        grid_cell_fill<true>(g, tg, x, y, z, cell, m);
      }
      if (__any(m > 0)) star_cells_mates(tg, m, cell, lane, qp, mine, Tb, self, limit, f, t, k, have);
    }
    have = ovf_scan<true>(tg, 0, 64, lane, qp, t, k, have, [&](int id, int tree) {
      int rk;
      return tree == mine && id >= Tb && id < self && star_accepted(f, id - Tb, rk);
    }, limit);
  }
}

// The sample's members (the list: ids, distances; a member that is an earlier sample of the round gets the node id it will
// have), every member's toucher list, and lane 0's first guess: the plain SFF cost through the expanded node ex0
__device__ __forceinline__ void star_publish(const StarView& S, const DevForestView& f, int i, int N0, int Tb, unsigned ep, int lane,
                                             const TopK& t, int cnt, int ex0, double pd0, double dr0) {
  const bool mem = lane < cnt;
  int node = -1;
  if (mem) {
    if (t.id < N0) node = t.id;
    else { int rk; star_accepted(f, t.id - Tb, rk); node = N0 + rk; }
  }
  const size_t p = (size_t)i * SFFK_STAR_KC + lane;
  S.prop[p] = STAR_INF;
  if (mem) {
    S.m_id[p] = node;
    S.m_d[p] = t.d;
    const unsigned long long mark = ((unsigned long long)ep << 32) | (unsigned long long)(p + 1);
    const unsigned long long old = atomicExch(&S.head[node], mark);
    S.next[p] = (unsigned)(old >> 32) == ep ? (int)(unsigned)(old & 0xffffffffULL) : 0;
  }
  if (lane == 0) {
    S.m_cnt[i] = cnt;
    S.best[i] = pd0 + dr0;   // (first guess: the plain SFF cost)
    S.psel[i] = ex0;
    S.dcl[i] = pd0;
    S.cnt[2 * (size_t)i] = 0ULL; S.cnt[2 * (size_t)i + 1] = 0ULL;
  }
}

}  // namespace sffk
