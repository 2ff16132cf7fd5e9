// kernels_dev.h — device-side helpers shared by kernels.hip, devforest.hip, devstar.hip and devprio.hip: neighbour-grid
// addressing, the relaxed agent-scope loads / stores, the reference's integer draw, the top-k list, the sampler.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "sff_geom.h"

namespace sffk {

__device__ __forceinline__ int grid_coord(float v, float o, float inv, int n) {
  float f = floorf((v - o) * inv);
  int c = f < 0.0f ? 0 : (f > (float)(n - 1) ? n - 1 : (int)f);  // NaN compares false twice -> cast of NaN; guarded by callers
  return c;
}

__device__ __forceinline__ size_t grid_cell_of(const GridView& g, float x, float y, float z) {
  const int cx = grid_coord(x, g.ox, g.inv_cell, g.nx), cy = grid_coord(y, g.oy, g.inv_cell, g.ny),
            cz = grid_coord(z, g.oz, g.inv_cell, g.nz);
  return ((size_t)cz * g.ny + cy) * g.nx + cx;
}
// (the sq_* / wt_* accesses below, declared here for the compact layout's table)
__device__ __forceinline__ int sq_i32(const int32_t* p);
// The bucket of a cell for an INSERT (GridView, the compact layout): the one the table names, or - the cell's first insert -
// one taken from the pool and published with a compare-and-swap; whoever loses that race uses the winner's bucket and
// leaves its own unused (a node opens at most one bucket, so a pool as large as the store never runs out).  Nobody
// waits for anybody.  -1: the pool is used up and the cell still has none - the item belongs on the overflow list.
__device__ __forceinline__ int grid_bucket_open(const GridView& g, size_t cell) {
  int b = sq_i32(g.bucket + cell);
  if (b >= 0) return b;
  const int mine = atomicAdd(g.pool_cnt, 1);
  if (mine >= g.pool_cap) return atomicCAS(g.bucket + cell, -1, -1);   // (what another insert may have published meanwhile)
  const int was = atomicCAS(g.bucket + cell, -1, mine);
  return was < 0 ? mine : was;
}
__device__ __forceinline__ void grid_put(const GridView& g, const GridItem& it) {
  const size_t cell = grid_cell_of(g, (float)it.p[0], (float)it.p[1], (float)it.p[2]);
  if (g.bucket) {   // compact (wave-uniform: g is the launch's argument): fp64 items only, buckets from the pool
    const int b = grid_bucket_open(g, cell);
    const int slot = b >= 0 ? atomicAdd(g.cnt + cell, 1) : g.bk;   // (a cell without a bucket counts as empty: cnt stays)
    if (slot < g.bk) {
      g.items[(size_t)b * g.bk + slot] = it;
    } else {
      const int o = atomicAdd(g.ovf_cnt, 1);
      if (o < g.ovf_cap) g.ovf[o] = it;   // the host checks ovf_cnt against ovf_cap
    }
    return;
  }
  const int slot = atomicAdd(g.cnt + cell, 1);
  if (g.occ) atomicOr(g.occ + (cell >> 5), 1u << (cell & 31));
  GridItem32 lt;
  lt.x = (float)it.p[0]; lt.y = (float)it.p[1]; lt.z = (float)it.p[2];
  lt.yaw = (float)it.p[3]; lt.pitch = (float)it.p[4]; lt.roll = (float)it.p[5];
  lt.id = it.id; lt.tree = it.tree;
  if (slot < g.bk) {
    g.items[cell * g.bk + slot] = it;
    if (g.lite) g.lite[cell * g.bk + slot] = lt;
  } else {
    const int o = atomicAdd(g.ovf_cnt, 1);
    if (o < g.ovf_cap) {   // the host checks ovf_cnt against ovf_cap
      g.ovf[o] = it;
      if (g.ovf_lite) g.ovf_lite[o] = lt;
    }
  }
}

// ---- relaxed agent-scope accesses (prio_heap_dev.h's hl_i32 / hl_f64 are the same loads under the heap's names)
// sq_*: loads of forest state the launch may itself have written go past the vector L1 (`sc1` loads served by the L2 the
// workgroup's stores write through to); the environment, the robot and the engine words are immutable while it runs.
__device__ __forceinline__ int sq_i32(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long sq_u64(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double sq_f64(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ int sq_u8(const uint8_t* p) { return (int)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sq_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// wt_*: write-through stores - what one wavefront writes and a wavefront on another XCD reads in the same launch
__device__ __forceinline__ void wt_i32(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void wt_u64(unsigned long long* p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wt_f64(double* p, double v) {
  wt_u64(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v));
}
__device__ __forceinline__ void wt_u8(uint8_t* p, uint8_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- the idioms of the one-slot loops (seq_waves_body.inc, k_spec_waves, rrt_seq_batch.inc): ONE wavefront works for one
// attempt, all 64 lanes together.  The round kernels and sq_knn keep their own copies of the flattening below
// (qc_candidates, collect_from_grid ...): helpers cost time there, profiles/README.md ("Shared idioms") has the numbers;
// the k-nearest kernels share theirs through knn_dev.h (lane_scan_incl, lane_owner).
// fp32 half-edge of the cell box around an exact fp64 ball of radius r: the store's fp32 slack and a few ulps on top
__device__ __forceinline__ float ball_box_radius(double r, double sweep_abs_eps) {
  const double ri = (r + sweep_abs_eps) * (1.0 + 1e-5);
  return sqrtf((float)(ri * ri) * 1.000001f) * 1.000001f;
}
// an item of the node grid: its fp64 position, id and tree (the launch itself writes items, hence sq loads)
__device__ __forceinline__ void grid_item_load(const GridItem* src, double* p6, int& id, int& tree) {
  const unsigned long long* q8 = reinterpret_cast<const unsigned long long*>(src);
  for (int k = 0; k < 6; ++k) p6[k] = __longlong_as_double((long long)sq_u64(q8 + k));
  const unsigned long long w = sq_u64(q8 + 6);
  id = (int)(unsigned)(w & 0xffffffffULL); tree = (int)(unsigned)(w >> 32);
}
// The neighbour ball: every item of the cells the box of half-edge rf around qp touches, then the overflow list.  64
// cells at a time (lane = cell) give their fill counts; a prefix scan and a six-step bisection deal the items over the
// lanes (lane = item), so that a cell with several items costs no extra step.  take(valid, item) is called by all 64
// lanes together (it may __ballot); valid = this lane has an item.
template <class Take>
__device__ __forceinline__ void grid_ball_items(const GridView& g, const double* qp, float rf, int lane, Take&& take) {
  const float qx = (float)qp[0], qy = (float)qp[1], qz = (float)qp[2];
  const int lx = grid_coord(qx - rf, g.ox, g.inv_cell, g.nx), hx = grid_coord(qx + rf, g.ox, g.inv_cell, g.nx);
  const int ly = grid_coord(qy - rf, g.oy, g.inv_cell, g.ny), hy = grid_coord(qy + rf, g.oy, g.inv_cell, g.ny);
  const int lz = grid_coord(qz - rf, g.oz, g.inv_cell, g.nz), hz = grid_coord(qz + rf, g.oz, g.inv_cell, g.nz);
  const int wx = hx - lx + 1, wy = hy - ly + 1, wz = hz - lz + 1;
  const int total = wx * wy * wz;
  for (int c0 = 0; c0 < total; c0 += 64) {
    const int ci = c0 + lane;
    int cell = 0, m = 0;   // cell: from here on the cell's BUCKET (dense: the cell itself)
    if (ci < total) {
      const int q1 = ci / wx, q2 = q1 / wy;
      cell = ((lz + q2) * g.ny + (ly + q1 - q2 * wy)) * g.nx + (lx + ci - q1 * wx);
      m = sq_i32(g.cnt + cell);
      if (g.bucket) {   // compact: the table's word asked for together with the count (same address pattern, independent)
        cell = sq_i32(g.bucket + cell);
        if (cell < 0) { cell = 0; m = 0; }
      }
      if (m > g.bk) m = g.bk;
    }
    int inc = m;
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(inc, off);
      if (lane >= off) inc += o;
    }
    const int tot = __shfl(inc, 63);
    for (int base = 0; base < tot; base += 64) {
      const int j = base + lane;
      const int jj = j < tot ? j : tot - 1;
      int lo = 0, hi = 63;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (__shfl(inc, mid) > jj) hi = mid; else lo = mid + 1;
      }
      const int src_cell = __shfl(cell, lo);
      const int slot = jj - (__shfl(inc, lo) - __shfl(m, lo));
      take(j < tot, g.items + (size_t)src_cell * g.bk + slot);
    }
  }
  int no = sq_i32(g.ovf_cnt);
  if (no > g.ovf_cap) no = g.ovf_cap;
  for (int base = 0; base < no; base += 64) take(base + lane < no, g.ovf + base + lane);
}
// The neighbour rank: lane j < n_hit holds hit j (tree t, distance d, id; qk = it qualifies as a neighbour); the number
// of qualifying hits the reference's neighbour loop visits before this lane's: tree id, then distance, then id
__device__ __forceinline__ int nb_rank(int n_hit, int t, double d, int id, bool qk) {
  int rank = 0;
  for (int j = 0; j < n_hit; ++j) {
    const int tj = __shfl(t, j), idj = __shfl(id, j), qj = __shfl((int)qk, j);
    const double dj = __shfl(d, j);
    if (qj && (tj < t || (tj == t && (dj < d || (dj == d && idj < id))))) ++rank;
  }
  return rank;
}
// The border table (DevForestView::bt_key / bt_val, open addressing): the key of the node pair a < b (never 0), where its
// probe sequence starts, and the read-only probe - h = the slot that holds the key or the first free one, true = the pair
// has no live entry (the caller may then write one at h).  SQ: sq loads, for a table other launches' or wavefronts' stores
// may have filled; plain loads where the table is the wavefront's alone while the launch runs.
__device__ __forceinline__ unsigned long long border_key(int a, int b) {
  return ((unsigned long long)(uint32_t)a << 32) | ((unsigned long long)(uint32_t)b + 1ULL);
}
__device__ __forceinline__ size_t border_hash(const DevForestView& f, unsigned long long key) {
  return (size_t)((key * 0x9E3779B97F4A7C15ULL) >> 17) & (size_t)f.bt_mask;
}
template <bool SQ>
__device__ __forceinline__ bool border_probe(const DevForestView& f, unsigned long long key, size_t& h) {
  h = border_hash(f, key);
  for (int guard = 0; guard < (1 << 24); ++guard) {
    const unsigned long long cur = SQ ? sq_u64(f.bt_key + h) : f.bt_key[h];
    if (cur == key) return (SQ ? sq_u64(f.bt_val + h) : f.bt_val[h]) == ~0ULL;
    if (cur == 0ULL) return true;
    h = (h + 1) & (size_t)f.bt_mask;
  }
  return false;
}
// The connected-trees test, maxConnected() == numRoots: every tree is reachable from tree 0 over pairs that hold a border
// (pair: R x R flags).  A lane per tree: R <= 64.
__device__ __forceinline__ bool trees_connected(const uint8_t* pair, int R, int lane) {
  unsigned long long reach = 1ULL, frontier_set = 1ULL;
  unsigned long long row = 0ULL;   // lane a: bit b = pair (a, b) has a border
  if (lane < R) for (int b2 = 0; b2 < R; ++b2) if (sq_u8(pair + (size_t)lane * R + b2)) row |= 1ULL << b2;
  while (frontier_set) {
    const int a = __ffsll((long long)frontier_set) - 1;
    frontier_set &= frontier_set - 1;
    const unsigned long long ra = __shfl(row, a) & ~reach;
    reach |= ra; frontier_set |= ra;
  }
  return __popcll(reach) == R;
}

// libstdc++ uniform_int_distribution<int>(0, range - 1) on one 64-bit engine word (Lemire's multiply-shift):
// returns the draw, or -1 when the word falls into the rejection zone (the reference then draws again)
__device__ __forceinline__ int lemire_pick(unsigned long long word, unsigned long long range) {
  const unsigned long long lo = word * range;
  const unsigned long long hi = __umul64hi(word, range);
  if (lo < range) {
    const unsigned long long thr = (0ULL - range) % range;
    if (lo < thr) return -1;
  }
  return (int)hi;
}

// ---- clearance bits: the placement arithmetic and the slack it leans on.  The bits (EnvView::clear_bits: a posed robot,
// clear_bits_edge: an un-rotated edge sample) answer ~97 % of the collision work with one lookup, and every path that asks
// them must ask the same bit for the same sample.  The contract with Ctx::build_clearance (engine.cpp) is stated HERE and
// nowhere else:
//  - A pose's cell is taken in fp64 from the model origin: (c - clear_org) * clear_inv per axis.
//  - An edge's samples are placed in fp32, in cells of the grid, at g + idx * d: g = (float)((a - clear_org) * clear_inv)
//    is the start point, d = (float)(b - a) * ((float)clear_inv * __frcp_rn((float)parts)) one sample step - the step
//    with the HARDWARE reciprocal of the edge's part count (a relative 1e-7 on a step that spans a few cells).  The exact
//    kernels place the same sample in fp64 (edge_sample_pos); the fp32 cell is off that position by less than
//    1e-6 * (cells per axis) cells, and build_clearance puts exactly that into the threshold of the bits.
//  - Eight consecutive samples of an edge lie within 0.4 units of the fifth one (the sample spacing never exceeds the
//    0.1 of src/problemStruct.h:121), and the EDGE plane is built with that reach on top: one probe answers a group of
//    eight samples (clear_group); a group that is not clear goes to the exact kernel whole (clear_group_mask).
//  - The grid spans the environment's box inflated by the build threshold: a cell outside it is clear without a word.
//    A NaN position, or a plane that was not built, leaves the sample needed with no word to look at.
// A slot function only computes where the bit is: the caller loads the words of all its slots together (one memory
// latency for everything) and looks at them afterwards.
// Change any of this together with build_clearance: a placement that drifts accepts an edge the exact test rejects.
// The fp32 placement (the edge in cells, a sample's fp32 cell) is still spelled out at each of its sites - they point
// here, and profiles/README.md ("Clearance lookups") says why; keep them identical to this block.

// where a sample's bit is: wp = the word (null = no word to look at), sh = the bit in it; need = the bits may still say no
struct ClearSlot {
  bool need;
  const uint32_t* wp;
  int sh;
};
// a position c (a pose's model origin, an exact edge sample), fp64, in a plane `bits` that was built (not null).  The pose
// and the edge plane differ in the pointer alone.
__device__ __forceinline__ ClearSlot clear_slot_f64(const EnvView& env, const uint32_t* bits, const double* c) {
  ClearSlot s{true, nullptr, 0};
  const double fx = (c[0] - env.clear_org[0]) * env.clear_inv, fy = (c[1] - env.clear_org[1]) * env.clear_inv,
               fz = (c[2] - env.clear_org[2]) * env.clear_inv;
  if (fx == fx && fy == fy && fz == fz) {
    if (fx < 0 || fy < 0 || fz < 0 || fx >= env.clear_n[0] || fy >= env.clear_n[1] || fz >= env.clear_n[2]) {
      s.need = false;                                       // beyond the inflated box of the environment
    } else {
      const long long ci = ((long long)(int)fz * env.clear_n[1] + (int)fy) * env.clear_n[0] + (int)fx;
      s.wp = bits + (ci >> 5);
      s.sh = (int)(ci & 31);
    }
  }
  return s;
}
// the whole question for one position, load included: true = the plane `bits` calls it clear
__device__ __forceinline__ bool surely_clear_in(const EnvView& env, const uint32_t* bits, const double* c) {
  if (!bits) return false;
  const double fx = (c[0] - env.clear_org[0]) * env.clear_inv, fy = (c[1] - env.clear_org[1]) * env.clear_inv,
               fz = (c[2] - env.clear_org[2]) * env.clear_inv;
  if (!(fx == fx && fy == fy && fz == fz)) return false;
  if (fx < 0 || fy < 0 || fz < 0 || fx >= env.clear_n[0] || fy >= env.clear_n[1] || fz >= env.clear_n[2]) return true;
  const long long idx = ((long long)(int)fz * env.clear_n[1] + (int)fy) * env.clear_n[0] + (int)fx;
  return (bits[idx >> 5] >> (idx & 31)) & 1u;
}
// group g (0..7) of chunk `chunk` of an edge of ns samples: any = it has a sample, left = valid samples from its first one
// on, probe = the sample to look up (within four steps of every valid sample of the group)
struct ClearGroup {
  bool any;
  int left, probe;
};
__device__ __forceinline__ ClearGroup clear_group(int chunk, int g, int ns) {
  const int first = 1 + 64 * chunk + 8 * g;
  return ClearGroup{first <= ns, ns - first + 1, first + 4 <= ns ? first + 4 : ns};
}
// the chunk's mask of samples for the exact kernel, in all eight lanes of the chunk: every valid sample of the groups still needed
__device__ __forceinline__ unsigned long long clear_group_mask(bool need, int left, int g) {
  unsigned long long m = need ? (((left >= 8 ? 0xffULL : ((1ULL << left) - 1ULL))) << (8 * g)) : 0ULL;
  m |= __shfl_xor(m, 1);
  m |= __shfl_xor(m, 2);
  m |= __shfl_xor(m, 4);
  return m;
}

// ---- survivors of the clearance cull -> items of the exact kernel.  The lead lanes (lane % 8 == 0) of a step each hold one
// (edge slot, 64-sample chunk, mask) survivor.  The exact kernel's length is its longest item (one wavefront per item:
// broad phase of the masked samples' swept box, then every sample against every candidate triangle), so a survivor with
// many samples is emitted as up to four 16-sample items: four wavefronts, each with a tighter box and a quarter of the
// samples.  buf must have room for 32 more entries.
// Measured (profiles/r3_head_a / r3_c5_d, split at > 20 samples): the longest launch shrinks (178 -> 104 us on dense_3D)
// but the average grows (37 -> 49 us: every item pays its own broad phase), on building.obj 102 -> 96 us: off by default.
#ifndef SFFK_SPLIT_MIN
#define SFFK_SPLIT_MIN 64
#endif
__device__ __forceinline__ void surv_emit(SurvivorItem* buf, int& n_buf, bool lead, int lane, int slot, int chunk,
                                          unsigned long long m) {
  int parts = 0;
  const bool split = lead && __popcll(m) > SFFK_SPLIT_MIN;
  if (lead) parts = split ? ((m & 0xffffULL) != 0) + ((m & 0xffff0000ULL) != 0) + ((m & 0xffff00000000ULL) != 0) + ((m >> 48) != 0) : 1;
  int inc = parts;
  for (int off = 8; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  const int total = __shfl(inc, 56);
  if (lead) {
    int at = n_buf + inc - parts;
    if (!split) buf[at] = SurvivorItem{slot, chunk, m};
    else
      for (int q = 0; q < 4; ++q) {
        const unsigned long long mq = m & (0xffffULL << (16 * q));
        if (mq) buf[at++] = SurvivorItem{slot, chunk, mq};
      }
  }
  n_buf += total;
}

// ---- exact k nearest: the wave-resident top-k list of k_knn_linear, the one-slot loops' sq_knn and the grid k-nearest
// family (k_knn_grid, k_knn_grid_wg, k_star_knn_wg, k_star_knn), whose shared cell, lane and overflow idioms and SFF*
// stages are knn_dev.h's
// The wave's k best so far: lane j holds the j-th smallest (distance, id) key; lanes >= have hold +inf.
struct TopK {
  double d;
  int id;
};
__device__ __forceinline__ bool key_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }
// inserts the candidates flagged in `take` (one per lane: cd, cid), smallest lanes first; k = capacity, have = filled
__device__ __forceinline__ void topk_insert(TopK& t, int lane, int k, int& have, unsigned long long take, double cd, int cid) {
  while (take) {
    const int src = __ffsll((long long)take) - 1;
    take &= take - 1;
    const double nd = __shfl(cd, src);
    const int ni = __shfl(cid, src);
    // rank of the newcomer = entries that sort before it
    const bool before = lane < have && key_less(t.d, t.id, nd, ni);
    const int rank = __popcll(__ballot(before));
    if (rank >= k) continue;                       // (beaten by k entries that arrived in the meantime)
    const double pd = __shfl_up(t.d, 1);
    const int pi = __shfl_up(t.id, 1);
    if (lane > rank) { t.d = pd; t.id = pi; }
    else if (lane == rank) { t.d = nd; t.id = ni; }
    if (have < k) ++have;
  }
}
// merges one candidate per lane (cv: valid, key (cd, cid)) into the list by RANKING instead of inserting one by one: every
// candidate and every list entry is broadcast once (scalar reads of its lane), every lane counts the keys below its own
// entry and below its own candidate, and each survivor is pushed to the lane of its rank (ds_permute; lane 63 takes what
// falls out - k <= 56).  One insertion is a dozen DEPENDENT cross-lane operations, ~0.6 us on a wavefront that is alone on
// its SIMD; a merge of five candidates into seventeen entries costs about what two insertions cost.  Same list as
// topk_insert leaves (keys are unique: ids are).
__device__ __forceinline__ void topk_merge(TopK& t, int lane, int k, int& have, bool cv, double cd, int cid) {
  unsigned long long mb = __ballot(cv);
  if (!mb) return;
  const int nb = __popcll(mb);
  const unsigned long long tb = (unsigned long long)__double_as_longlong(t.d), cb = (unsigned long long)__double_as_longlong(cd);
  const int tlo = (int)(unsigned)(tb & 0xffffffffULL), thi = (int)(unsigned)(tb >> 32);
  const int clo = (int)(unsigned)(cb & 0xffffffffULL), chi = (int)(unsigned)(cb >> 32);
  int ra = lane, rb = 0;       // my list entry's / my candidate's rank in the union (the list is sorted: lane entries of it are below mine)
  while (mb) {
    const int j = __ffsll((long long)mb) - 1;
    mb &= mb - 1;
    const double sd = __longlong_as_double((long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(chi, j) << 32) |
                                                       (unsigned long long)(unsigned)__builtin_amdgcn_readlane(clo, j)));
    const int si = __builtin_amdgcn_readlane(cid, j);
    ra += key_less(sd, si, t.d, t.id) ? 1 : 0;
    rb += key_less(sd, si, cd, cid) ? 1 : 0;
  }
  for (int j = 0; j < have; ++j) {
    const double sd = __longlong_as_double((long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(thi, j) << 32) |
                                                       (unsigned long long)(unsigned)__builtin_amdgcn_readlane(tlo, j)));
    const int si = __builtin_amdgcn_readlane(t.id, j);
    rb += key_less(sd, si, cd, cid) ? 1 : 0;
  }
  const int da = (lane < have && ra < k) ? ra : 63, db = (cv && rb < k) ? rb : 63;
  const int a_lo = __builtin_amdgcn_ds_permute(da << 2, tlo), a_hi = __builtin_amdgcn_ds_permute(da << 2, thi);
  const int a_id = __builtin_amdgcn_ds_permute(da << 2, t.id), a_on = __builtin_amdgcn_ds_permute(da << 2, 1);
  const int b_lo = __builtin_amdgcn_ds_permute(db << 2, clo), b_hi = __builtin_amdgcn_ds_permute(db << 2, chi);
  const int b_id = __builtin_amdgcn_ds_permute(db << 2, cid);
  const int total = have + nb;
  have = total < k ? total : k;
  if (lane < have) {
    const unsigned long long bits = a_on ? (((unsigned long long)(unsigned)a_hi << 32) | (unsigned)a_lo) : (((unsigned long long)(unsigned)b_hi << 32) | (unsigned)b_lo);
    t.d = __longlong_as_double((long long)bits);
    t.id = a_on ? a_id : b_id;
  } else { t.d = 1.0e300; t.id = 0x7fffffff; }
}
__device__ __forceinline__ double topk_worst(const TopK& t, int k, int have) {   // current k-th distance (inf while not full)
  return have < k ? 1.0e300 : __shfl(t.d, k - 1);
}

// ---- SFF* (devstar.hip, k_star_knn_wg in kernels.hip): is sample i of the committed round accepted, and its rank among them
__device__ __forceinline__ bool star_accepted(const DevForestView& f, int i, int& rank) {
  const unsigned long long w = f.w_acc[i >> 6];
  rank = f.acc_pref[i >> 6] + __popcll(w & ((1ULL << (i & 63)) - 1ULL));
  return (w >> (i & 63)) & 1ULL;
}


// ---- sample + steer of one slot (k_sample_steer; the device engine's k_append_sample runs it for the NEXT round right
// behind the append).  The kernels are latency bound (one thread per sample, a few thousand samples): what they cost is
// the number of DEPENDENT memory levels, so the sample's inputs are fetched in two batches whose loads leave together -
//   1. what the thread index alone addresses: the control-block fields (sample_ctl), the caller's own lists;
//   2. what the expanded node and the sample's index address (sample_fetch): position / flag / tree of the node, the
//      engine words, the host's trig values in libm parity mode -
// and every store comes behind them (sample_finish): a store may alias a later load, which then cannot leave early.
// Out-of-range threads fetch with harmless indices (node 0, sample 0) instead of branching around the loads.
struct SampleCtl {
  int32_t n, halt, act_sel, round, ord_valid, n_slots, act_identity;
  unsigned long long words_base;
};
__device__ __forceinline__ SampleCtl sample_ctl(const DevCtrl* c) {
  SampleCtl K;
  K.n = c->n_act; K.halt = c->halt; K.act_sel = c->act_sel; K.round = c->round; K.ord_valid = c->ord_valid;
  K.n_slots = c->n_slots; K.act_identity = c->act_identity; K.words_base = c->words_base;
  return K;
}
// The end of a batch of loads.  The compiler sinks a load into the branch that uses its value and waits for a value
// where it is first looked at - either way the loads of a batch would leave one after the other again.  These empty
// statements "use" the values: every load written above them has been issued when the first one is reached (they
// count as memory accesses, so no load moves across), and nothing behind them moves up.  join_u: values that came
// through the scalar cache (control-block fields of a kernel that writes none: k_sample_steer; on a value the compiler
// holds in a vector register the "s" constraint does not compile), join_v: values in vector registers.  Call ONE of
// them per batch with every value the batch loads.  Nothing in the suite can see a batch fall apart again: after a
// compiler upgrade look at the kernels' -S output (the batch's loads in front of the first s_waitcnt on any of
// them) and at profiles/kernel_regs.sh.
template <class T> __device__ __forceinline__ void join_one_u(T& x) { asm volatile("" : "+s"(x) : : "memory"); }
template <class T> __device__ __forceinline__ void join_one_v(T& x) { asm volatile("" : "+v"(x) : : "memory"); }
template <class... T> __device__ __forceinline__ void join_u(T&... x) { (join_one_u(x), ...); }
template <class... T> __device__ __forceinline__ void join_v(T&... x) { (join_one_v(x), ...); }
__device__ __forceinline__ void join_ctl_u(SampleCtl& K) {
  join_u(K.n, K.halt, K.act_sel, K.round, K.ord_valid, K.n_slots, K.act_identity, K.words_base);
}
__device__ __forceinline__ void join_ctl_v(SampleCtl& K) {
  join_v(K.n, K.halt, K.act_sel, K.round, K.ord_valid, K.n_slots, K.act_identity, K.words_base);
}
struct SampleIn {
  double c[6];          // the expanded node's position (or the caller's centre)
  uint64_t w[6];        // the sample's engine words
  sffg::SampleTrig trig;
  int32_t tree;         // the node's tree
  uint8_t force;        // its ForceChildren flag
};
// the second batch.  i and par are in range (the caller replaces those of a thread without a sample by 0)
__device__ __forceinline__ SampleIn sample_fetch(int i, int par, const SampleCtl& K, const SampleLaunch& P) {
  const DevRound& dv = P.dv;
  SampleIn S{};
  const double* src = P.center_in ? P.center_in + 6 * (size_t)i : P.node_pos + 6 * (size_t)par;
  for (int k = 0; k < 6; ++k) S.c[k] = src[k];
  if (P.tmp.cnt) S.tree = P.tmp.st.tree[par];
  if (dv.ctrl) {   // the sample's words sit in the engine-word ring, in the reference's draw order
    S.force = dv.nflag[par] & 1;
    const unsigned long long base = K.words_base + (unsigned long long)dv.words_per * (unsigned long long)i;
    for (int k = 0; k < 6; ++k) S.w[k] = k < dv.words_per ? dv.ring[(base + k) & dv.ring_mask] : 0ULL;
    if (dv.trig) {   // libm parity mode: the transcendental values of these words, evaluated by the host's C library
      const double* t0 = dv.trig + 3 * (size_t)(base & dv.ring_mask);
      S.trig.c_phi = t0[0]; S.trig.s_phi = t0[1];
      if (dv.words_per == 6) {
        const double* t1 = dv.trig + 3 * (size_t)((base + 1) & dv.ring_mask);
        const double* t3 = dv.trig + 3 * (size_t)((base + 3) & dv.ring_mask);
        S.trig.c_theta = t1[0]; S.trig.s_theta = t1[1];
        S.trig.acos_u = t3[2];
      }
    }
  } else {
    for (int k = 0; k < 6; ++k) S.w[k] = P.words[6 * (size_t)i + k];
  }
  return S;
}
// everything that stores.  tid = the thread's index in the launch (per-round housekeeping), valid: the thread draws
// sample i from node par with the inputs S; ord_pos >= 0: the wave's first sampling launch - slot tid takes this
// position in the wave's spatial order.
__device__ __forceinline__ void sample_finish(int tid, bool valid, int i, int par, const SampleIn& S, int ord_pos,
                                              const SampleCtl& K, const SampleLaunch& P) {
  using namespace sffg;
  const int n = K.n;
  const double dist = P.dist;
  const int dim = P.dim;
  const SampleParams& prm = P.prm;
  double* __restrict__ out6 = P.out6;
  uint8_t* __restrict__ in_lim = P.in_lim;
  double* __restrict__ parent_dist = P.parent_dist;
  SweepQuery* __restrict__ queries = P.queries;
  const int32_t q_max_base = P.q_max_base;
  const RoundTemps& tmp = P.tmp;
  const DevRound& dv = P.dv;
  if (dv.ctrl) {
    if (tid == 0 && dv.qclk) { dv.qclk[0] = ~0ULL; dv.qclk[1] = 0ULL; }
    if (dv.qclk_sh && tid < 128) dv.qclk_sh[(tid >> 1) * 16 + (tid & 1)] = (tid & 1) ? ~0ULL : 0ULL;
  }
  if (tmp.cnt) {
    // per-round housekeeping folded into this launch: hit counters, the work-list cursor, and NaN
    // placeholders for the store entries between the permanent nodes and the 4-aligned temporaries
    if (tid < n) tmp.cnt[tid] = 0;
    if (tid < 32) tmp.ctrl[tid] = 0;
    if (tmp.sub && tid < SFFK_SUBLISTS) {   // heavy items, the exact kernel's item tickets, light items
      tmp.sub[tid * SFFK_SUB_STRIDE] = 0; tmp.sub[tid * SFFK_SUB_STRIDE + 1] = 0; tmp.sub[tid * SFFK_SUB_STRIDE + 2] = 0;
    }
    if (tid < tmp.base - tmp.n_perm) {
      const float nanv = __int_as_float(0x7fc00000);
      const size_t o = (size_t)tmp.n_perm + tid;
      tmp.st.x[o] = nanv; tmp.st.y[o] = nanv; tmp.st.z[o] = nanv;
      tmp.st.yaw[o] = nanv; tmp.st.pitch[o] = nanv; tmp.st.roll[o] = nanv;
    }
  }
  if (ord_pos >= 0) {
    const int sel = K.act_sel, n_slots = K.n_slots, pos = ord_pos;
    dv.ord.slot_pos[tid] = pos;
    (sel ? dv.ord.lst[1] : dv.ord.lst[0])[pos] = tid < n ? tid : -1;      // (this round: every position holds its slot's sample)
    if ((pos & 63) == 0) (sel ? dv.ord.cnt[1] : dv.ord.cnt[0])[(pos >> 6) * SFFK_ORD_CNT_STRIDE] = n_slots - pos < 64 ? n_slots - pos : 64;
  }
  if (!valid) return;
  double c[6], o[6];
  uint64_t w[6];
  for (int k = 0; k < 6; ++k) { c[k] = S.c[k]; w[k] = S.w[k]; }
  if (dv.ctrl) {
    dv.parent_out[i] = par;
    dv.force_out[i] = S.force;
  }
  if (tmp.center_out) for (int k = 0; k < 6; ++k) tmp.center_out[6 * (size_t)i + k] = c[k];
  bool ok;
  if (dv.ctrl && dv.trig) {
    ok = sample_point_with(w, c, dist, dim, prm.limits, o, S.trig);
  } else if (tmp.preset) {
    for (int k = 0; k < 6; ++k) o[k] = tmp.preset[6 * (size_t)i + k];
    ok = in_limits(o, prm.limits);
  } else {
    ok = sample_point(w, c, dist, dim, prm.limits, o);
  }
  for (int k = 0; k < 6; ++k) out6[6 * (size_t)i + k] = o[k];
  in_lim[i] = ok ? 1 : 0;
  const int tr = S.tree;
  if (tmp.cnt) {
    // the sample becomes temporary store entry base + i (NaN floats when out of limits, so that no query
    // can match it), with the tree of the node it was expanded from
    const float nanv = __int_as_float(0x7fc00000);
    const size_t t = (size_t)tmp.base + i;
    tmp.st.x[t] = ok ? (float)o[0] : nanv;
    tmp.st.y[t] = ok ? (float)o[1] : nanv;
    tmp.st.z[t] = ok ? (float)o[2] : nanv;
    tmp.st.yaw[t] = ok ? (float)o[3] : nanv;
    tmp.st.pitch[t] = ok ? (float)o[4] : nanv;
    tmp.st.roll[t] = ok ? (float)o[5] : nanv;
    for (int k = 0; k < 6; ++k) tmp.st.pos[6 * t + k] = o[k];
    tmp.st.tree[t] = tr;
    if (ok && tmp.tg.cnt) {   // and into the round's own grid, where the later samples of the round look for it
      GridItem it;
      for (int k = 0; k < 6; ++k) it.p[k] = o[k];
      it.id = (int32_t)t;
      it.tree = tr;
      it.pad[0] = it.pad[1] = 0;
      grid_put(tmp.tg, it);
    }
  }
  if (parent_dist) {
    double pd = dist6(c, o);  // parentDistance, src/forest.h:250
    parent_dist[i] = pd;
    if (queries) {
      SweepQuery q;
      q.x = (float)o[0]; q.y = (float)o[1]; q.z = (float)o[2];
      q.yaw = (float)o[3]; q.pitch = (float)o[4]; q.roll = (float)o[5];
      double r = pd > prm.dist_tree ? pd : prm.dist_tree;
      q.r = r;
      double ri = (r + prm.sweep_abs_eps) * (1.0 + 1e-5);
      q.r2f = (float)(ri * ri) * 1.000001f;
      q.tree = -1;
      q.max_id = q_max_base + i;
      q.active = (ok && (prm.world <= 1 || i % prm.world == prm.rank)) ? 1 : 0;
      q.pad = 0;
      queries[i] = q;
      if (tmp.qrec) {
        QRec r;
        r.q[0] = q.x; r.q[1] = q.y; r.q[2] = q.z; r.q[3] = q.yaw; r.q[4] = q.pitch; r.q[5] = q.roll;
        r.r2f = q.r2f; r.max_id = q.max_id; r.q_tree = q.tree;
        r.mine = tr;
        r.evaluate = q.active;
        // the cells the query ball's box touches (the round's own grid has the node grid's cells)
        const GridView& g = tmp.tg;
        const float rf = sqrtf(q.r2f) * 1.000001f;
        const int lx = grid_coord(q.x - rf, g.ox, g.inv_cell, g.nx), hx = grid_coord(q.x + rf, g.ox, g.inv_cell, g.nx);
        const int ly = grid_coord(q.y - rf, g.oy, g.inv_cell, g.ny), hy = grid_coord(q.y + rf, g.oy, g.inv_cell, g.ny);
        const int lz = grid_coord(q.z - rf, g.oz, g.inv_cell, g.nz), hz = grid_coord(q.z + rf, g.oz, g.inv_cell, g.nz);
        r.lx = lx; r.ly = ly; r.lz = lz; r.wx = hx - lx + 1; r.wy = hy - ly + 1;
        r.total = q.active ? r.wx * r.wy * (hz - lz + 1) : 0;
        // the parent edge, isPathFree(expanded, newPoint) (src/forest.h:246): its length is parentDistance
        const double parts0 = pd / 0.1;   // = edge_parts(c, o)
        r.ns0 = edge_samples(parts0);
        // (the edge in cells of the clearance grid: "clearance bits" above)
        const float inv0 = (float)tmp.clear_inv * __frcp_rn((float)parts0);
        for (int k = 0; k < 3; ++k) {
          r.t0[k] = (float)((c[k] - tmp.clear_org[k]) * tmp.clear_inv);
          r.t0[3 + k] = (float)(o[k] - c[k]) * inv0;
        }
        r.pdist = pd; r.qr = q.r;
        r.scratch[0] = r.scratch[1] = r.scratch[2] = r.scratch[3] = 0;
        tmp.qrec[i] = r;
      }
    }
  }
}

// k_sample_steer: thread tid draws sample tid; its node comes from the caller's parent list (host replay), from the
// caller's centres, or - device engine - from its slot.  In the first round of a fresh wave the active list is the
// identity (DevCtrl::act_identity), so the slot's node is asked for in the first batch; otherwise (a resumed wave,
// SFFGPU_NO_FUSED_SAMPLE's later rounds) the slot is looked up in the active list first: one level more.
__device__ __forceinline__ void sample_steer_one(int tid, const SampleLaunch& P) {
  const DevRound& dv = P.dv;
  const int tc = tid < P.n ? tid : P.n - 1;   // (P.n = the launch bound: every per-sample / per-slot array holds that many)
  SampleCtl K{};
  K.n = P.n;
  int par = 0, a0 = 0, a1 = 0, key = 0, rnk = 0;
  if (dv.ctrl) {
    // (spatial order off: any int per slot will do - no branch around two of the batch's loads)
    const int32_t* kp = dv.ord.hist ? dv.ord.slot_key : dv.act_slot;
    const int32_t* rp = dv.ord.hist ? dv.ord.slot_rank : dv.act_slot;
    a0 = dv.act_slot[tc]; a1 = dv.act_slot2[tc];
    par = dv.slot_node[tc];
    key = kp[tc]; rnk = rp[tc];
    K = sample_ctl(dv.ctrl);
    join_ctl_u(K);
    join_v(a0, a1, par, key, rnk);
  } else if (!P.center_in) {
    par = P.parent[tc];
  }
  if (K.halt) return;
  const bool valid = tid < K.n;
  // (not the identity: the first batch's slot_node entry was some other slot's - one level more)
  if (dv.ctrl && !(K.act_identity && K.round == 1)) par = dv.slot_node[valid ? (K.act_sel ? a1 : a0) : 0];
  if (!valid) par = 0;
  // the wave's first sampling launch (sample index == slot): every slot gets its position in the wave's spatial order
  const bool ord_now = dv.ctrl && dv.ord.hist && K.ord_valid && K.round == 1 && tid < K.n_slots;
  const SampleIn S = sample_fetch(valid ? tid : 0, par, K, P);
  const int start = dv.ctrl && dv.ord.hist ? dv.ord.start[ord_now ? key : 0] : 0;   // (with the second batch)
  sample_finish(tid, valid, tid, par, S, ord_now ? start + rnk : -1, K, P);
}

}  // namespace sffk
