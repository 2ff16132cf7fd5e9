// prio_heap_dev.h - one binary heap of the priority-frontier mode (PrioView, kernels.h) in HBM, worked on by ONE wavefront:
// pop / pop at index / remove / push of src/heap.h with the reference's array order.  Shared by the per-heap kernels of
// the round engine (devprio.hip: k_prio_pops, k_prio_end) and by the loop of waves of one slot (kernels.hip:
// seq_waves_body.inc, PRIO instances).  Include behind kernels_dev.h (the debug build's clock); everything lives in sffk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace sffk {

// ---- one heap in HBM, worked on by ONE wavefront (all 64 lanes call these together).
// A launch reads what it has written itself: loads go past the vector L1 (relaxed agent-scope = sc1, served by the L2
// where the stores land); a wavefront's accesses to one address reach the L2 in program order, so an operation sees
// the stores of the one before it without waiting for them.
// What makes a sift slow is one L2 round trip per level.  Both directions fetch their whole neighbourhood at once:
// the sift-down the 62 descendants of the next five levels (lane = position in that sub-heap), the sift-up every
// ancestor up to the root (lane = level) - the walk itself then runs on registers (round 4; 4 us -> ~1 us per pop).
#ifdef SFFK_PRIO_DEBUG
#define PDBG(i_, val_) do { h.dbg[i_] += (long long)(val_); } while (0)
#define PCLK() ((long long)wall_clock64())
#else
#define PDBG(i_, val_) do {} while (0)
#define PCLK() 0LL
#endif
struct HeapRef {
  int32_t* v; double* key; int32_t* pos; int32_t* size_p;
  int n;
#ifdef SFFK_PRIO_DEBUG
  long long dbg[16];
#endif
};
__device__ __forceinline__ int hl_i32(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double hl_f64(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void heap_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// Keys are distances (>= +0, never NaN): their bit patterns order like unsigned integers, so the walks below compare
// and carry them as 64-bit integers in SGPRs - every value of a walk is the same in all lanes, and written this way
// (readfirstlane / readlane) the compiler keeps the whole walk on the scalar unit with uniform branches; as "divergent"
// vector code a level cost ~400 cycles of exec-mask bookkeeping (1 us per five levels, measured).
typedef unsigned long long hkey_t;
__device__ __forceinline__ hkey_t hk_bits(double k) { return (hkey_t)__double_as_longlong(k); }
__device__ __forceinline__ int uni_i32(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ hkey_t uni_u64(hkey_t x) {
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(x & 0xffffffffULL));
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(x >> 32));
  return ((hkey_t)hi << 32) | (hkey_t)lo;
}
__device__ __forceinline__ int lane_i32(int x, int src) { return __builtin_amdgcn_readlane(x, src); }
__device__ __forceinline__ hkey_t lane_u64(hkey_t x, int src) {
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(x & 0xffffffffULL), src);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(x >> 32), src);
  return ((hkey_t)hi << 32) | (hkey_t)lo;
}
// lane ^ 1 (DPP quad_perm [1,0,3,2]: a VALU move, not a trip through the LDS crossbar)
__device__ __forceinline__ int dpp_xor1(int x) { return __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ hkey_t hl_key(const double* p) {
  return __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void heap_put(const HeapRef& h, int i, int node, hkey_t k) {
  h.v[i] = node; reinterpret_cast<unsigned long long*>(h.key)[i] = k; h.pos[node] = i;
}
// the same entry from every lane: one lane stores it (64 lanes on one address are not merged into one request)
__device__ __forceinline__ void heap_put1(const HeapRef& h, int i, int node, hkey_t k) { if ((threadIdx.x & 63) == 0) heap_put(h, i, node, k); }
// ---- the two sifts, each split into "ask for everything it can need" and "decide", so that an operation asks for its
// own entries, the ancestors and the sub-heap below in ONE round trip.
// One wavefront alone issues an instruction every 5-8 cycles, so a walk that compares level after level costs ~250
// cycles per level even as scalar code (measured: 1.9 us for 15 levels with all data in registers).  Instead every lane
// decides for its own entry, all at once.
struct HeapWin { hkey_t kq; int vq; int at; bool have; };    // lane q (2..63) = q-th entry (1-based, level order) below `index`
__device__ __forceinline__ HeapWin win_loads(const HeapRef& h, int index, int n) {
  const int lane = threadIdx.x & 63;
  const int d = 31 - __clz(lane | 1);
  const long long at64 = (((long long)index + 1) << d) - 1 + (lane - (1 << d));
  HeapWin w;
  w.have = lane >= 2 && at64 < n;
  w.at = (int)at64;
  w.kq = w.have ? hl_key(h.key + w.at) : 0ULL;
  w.vq = w.have ? hl_i32(h.v + w.at) : 0;
  return w;
}
// Heap::BubbleDown of (node, k) standing at `index` in a heap of n entries (src/heap.h:122-149: the smaller child, ties
// to the left), w = the window below index.  "I am the smaller child of my parent" (the sibling's key comes from the
// neighbouring lane) "and k is larger than my key" - the reference's two comparisons say exactly that: the element
// moves down to the smaller child, the left one on a tie, while k is larger than that child's key.  The ballot of these
// bits holds the whole path through the window; following it is a shift and a test per level, and the entries on the
// path move up with ONE store per array.
__device__ void down_finish(HeapRef& h, int index, int node, hkey_t k, int n, HeapWin w) {
  const int lane = threadIdx.x & 63;
  while (true) {
    if (2 * (long long)index + 1 >= n) break;
    const hkey_t ks = ((hkey_t)(unsigned int)dpp_xor1((int)(unsigned int)(w.kq >> 32)) << 32) | (hkey_t)(unsigned int)dpp_xor1((int)(unsigned int)(w.kq & 0xffffffffULL));
    const bool sib_have = dpp_xor1(w.have ? 1 : 0) != 0;
    const bool left = (lane & 1) == 0;
    const bool smaller = w.have && (left ? !(sib_have && ks < w.kq) : (w.kq < ks));
    const unsigned long long mv = __ballot(smaller && k > w.kq);   // the element would move down INTO this entry's place
    unsigned long long path = 0ULL;
    int q = 1;
    while (q < 32) {
      const unsigned int two = (unsigned int)(mv >> (2 * q)) & 3u;
      if (!two) break;
      q = 2 * q + (int)(two >> 1);
      path |= 1ULL << q;
    }
    if ((path >> lane) & 1ULL) heap_put(h, (w.at - 1) >> 1, w.vq, w.kq);   // every entry on the path: one level up
    if (q > 1) index = lane_i32(w.at, q);
    if (q < 32) break;
    w = win_loads(h, index, n);
  }
  heap_put1(h, index, node, k);
}
struct HeapAnc { hkey_t kp; int vp; bool have; };            // lane j = the (j + 1)-th ancestor of `index`
__device__ __forceinline__ HeapAnc anc_loads(const HeapRef& h, int index) {
  const int lane = threadIdx.x & 63;
  const unsigned int i1 = (unsigned int)index + 1u;        // 1-based: the j-th ancestor is (i1 >> j) - 1
  const unsigned int mine = lane < 31 ? (i1 >> (lane + 1)) : 0u;
  HeapAnc a;
  a.have = mine != 0u;
  a.kp = a.have ? hl_key(h.key + (mine - 1u)) : 0ULL;
  a.vp = a.have ? hl_i32(h.v + (mine - 1u)) : 0;
  return a;
}
// Heap::BubbleUp of (node, k) standing at `index` (src/heap.h:151-163)
__device__ void up_finish(HeapRef& h, int index, int node, hkey_t k, HeapAnc a) {
  const int lane = threadIdx.x & 63;
  const unsigned int i1 = (unsigned int)index + 1u;
  const unsigned long long stop = __ballot(!(a.have && a.kp > k));   // (lane 31 always stops)
  const int up = __ffsll((long long)stop) - 1;               // ancestors 1 .. up move one level down
  if (lane < up) heap_put(h, (int)(i1 >> lane) - 1, a.vp, a.kp);
  heap_put1(h, (int)(i1 >> up) - 1, node, k);
}
__device__ int heap_pop(HeapRef& h) {                       // Heap::pop()
  [[maybe_unused]] const long long t_a = PCLK();
  const int size = uni_i32(h.n);
  const int last_v = hl_i32(h.v + size - 1);
  const hkey_t last_k = hl_key(h.key + size - 1);
  const int root = hl_i32(h.v);
  const HeapWin w = win_loads(h, 0, size - 1);
  const int mn = uni_i32(root);
  if ((threadIdx.x & 63) == 0) h.pos[mn] = -1;
  h.n = size - 1;
  if (size > 1) down_finish(h, 0, uni_i32(last_v), uni_u64(last_k), size - 1, w);
  PDBG(0, 1); PDBG(1, PCLK() - t_a);
  return mn;
}
// Heap::pop(index), id < size
struct HeapAt { int val, last; hkey_t old_cost, new_cost; HeapAnc a; HeapWin w; };
__device__ __forceinline__ HeapAt pop_at_loads(const HeapRef& h, int id, int size) {
  HeapAt L;
  L.last = hl_i32(h.v + size - 1);
  L.new_cost = hl_key(h.key + size - 1);
  L.val = hl_i32(h.v + id);
  L.old_cost = hl_key(h.key + id);
  L.a = anc_loads(h, id);
  L.w = win_loads(h, id, size - 1);
  return L;
}
__device__ int pop_at_finish(HeapRef& h, int id, int size, const HeapAt& L) {
  const int val = uni_i32(L.val);
  if ((threadIdx.x & 63) == 0) h.pos[val] = -1;
  h.n = size - 1;
  if (id != size - 1) {
    const hkey_t nc = uni_u64(L.new_cost), oc = uni_u64(L.old_cost);
    const int last = uni_i32(L.last);
    if (nc < oc) up_finish(h, id, last, nc, L.a); else down_finish(h, id, last, nc, size - 1, L.w);
  }
  return val;
}
__device__ int heap_pop_at(HeapRef& h, int id) {
  id = uni_i32(id);
  const int size = uni_i32(h.n);
  if (id >= size) return -1;
  const HeapAt L = pop_at_loads(h, id, size);
  return pop_at_finish(h, id, size, L);
}
// `node` leaves the heap (src/forest.h:164-173).  hint = where the position map had it when the chunk was gathered: the
// map is asked again, together with everything a removal at `hint` needs - one round trip when the hint still holds
__device__ void heap_remove(HeapRef& h, int node, int hint) {
  node = uni_i32(node); hint = uni_i32(hint);
  const int size = uni_i32(h.n);
  const int now_v = hl_i32(h.pos + node);
  if (hint >= 0 && hint < size) {
    const HeapAt L = pop_at_loads(h, hint, size);
    const int now = uni_i32(now_v);
    if (now == hint) { (void)pop_at_finish(h, hint, size, L); return; }
    if (now >= 0) (void)heap_pop_at(h, now);
    return;
  }
  const int now = uni_i32(now_v);
  if (now >= 0) (void)heap_pop_at(h, now);
}
__device__ void heap_push(HeapRef& h, int node, hkey_t k) {  // Heap::push
  const int at = uni_i32(h.n);
  h.n = at + 1;
  const HeapAnc a = anc_loads(h, at);
  up_finish(h, at, uni_i32(node), uni_u64(k), a);
}

// the heap `h` of P holding n entries (a caller that keeps the sizes itself; heap_of below reads the size array)
__device__ __forceinline__ HeapRef heap_with(const PrioView& P, int h, int n) {
  HeapRef r;
  r.v = P.v + (size_t)h * P.cap; r.key = P.key + (size_t)h * P.cap; r.pos = P.pos + (size_t)h * P.cap;
  r.size_p = P.size + h;
  r.n = n;
#ifdef SFFK_PRIO_DEBUG
  for (int i = 0; i < 16; ++i) r.dbg[i] = 0;
#endif
  return r;
}

}  // namespace sffk
