// smooth_paths.inc - path smoothing on the device: smoothPaths' walk over ONE path on ONE wavefront (kernels.h:
// SmoothPathArgs), included by kernels.hip behind the session batches' loop, whose edge test it uses as it is:
// sq_edge_clear_fast || sq_path_free = isPathFree by the wavefront, lazy and exact, the reference-equivalent counters
// advanced by first_hit or n_samples.  Reference: SpaceForest::smoothPaths src/forest.h:464-511, RapidExpTree::smoothPaths
// src/rrt.h:354-379; on the host Forest::smooth_paths (paths.cpp) and Rrt::smooth_paths (rrt.cpp), which evaluate every
// candidate of a step in one batch - here, as in the reference, the candidates behind the first free one are never tested.
//
// The walk needs positions only, and only ORIGINAL indices: a step with far end g looks at entries 0 .. g and makes t <= g-1
// the next far end, so what it drops (t+1 .. g-1) lies behind everything a later step reads.  The chosen t of every step goes
// to the path's output row; the host drops the entries and, for a forest, replays the fp64 cost arithmetic from them.
__device__ __forceinline__ void smooth_path_body(const SmoothPathArgs& A) {
  extern __shared__ double lds_d[];
  __shared__ int32_t s_fh, s_ovf;
  SmoothCtrl* c = A.ctrl;
  const int lane = threadIdx.x;
  // ---- the control block, in registers (everything here is the same in every lane)
  int g = c->g, t = c->t_next, n_out = c->n_out;
  // (a finished path of an earlier launch; a block the host has not put right is left alone - the host sees no progress)
  if (g <= 0 || g >= A.len || t < 0 || n_out < 0 || c->status != SFFK_SMOOTH_RAN) return;
  double* rtri = lds_d;
  double* stage = rtri + (size_t)A.rob.n_tri * 9;
  int32_t* ibase = reinterpret_cast<int32_t*>(stage + STAGE_DOUBLES);
  int32_t* stack = ibase;                        // (+ the triangle-grid hash set behind it)
  int32_t* cand = ibase + (STACK_CAP + TG_HASH);
  int32_t* queue = cand + CAND_CAP;
  for (int i = lane; i < A.rob.n_tri * 9; i += 64) rtri[i] = A.rob.tri[i];
  __builtin_amdgcn_wave_barrier();
  fill_robot_boxes(rtri, reinterpret_cast<double*>(queue + QUEUE_CAP), A.rob.n_tri, lane, 64);
  __builtin_amdgcn_wave_barrier();
  unsigned long long cc = c->collide_calls, pf = c->path_free_calls, ex_seg = c->segments, ex_smp = c->samples;
  int status = SFFK_SMOOTH_RAN, edges = 0;
  while (g > 0) {
    double b[6];
    for (int k = 0; k < 6; ++k) b[k] = A.pos[6 * (size_t)g + k];
    bool stop = false;
    while (t < g - 1) {                          // candidates t = 0 .. g-2, the first free one ends the step
      if (edges >= A.max_edges) { stop = true; break; }   // the launch's budget: the next launch tests (t, g) first
      double a[6];
      for (int k = 0; k < 6; ++k) a[k] = A.pos[6 * (size_t)t + k];
      const unsigned long long cc_a = cc, smp_a = ex_smp;
      bool flt = false;
      const bool fr = sq_edge_clear_fast(A.env, a, b, lane, cc, ex_smp) || sq_path_free(A.env, A.rob, rtri, stack, cand, queue, stage, a, b, &s_fh, &s_ovf, lane, cc, ex_smp, flt);
      if (flt) { cc = cc_a; ex_smp = smp_a; status = SFFK_SMOOTH_HOST; stop = true; break; }   // (the edge never happened here)
      pf += 1; ex_seg += 1; ++edges;
      if (fr) break;
      ++t;
    }
    if (stop) break;
    if (lane == 0) A.out[n_out] = t;             // t = g-1: no candidate was free (or there was none)
    ++n_out;
    g = t;
    t = 0;
  }
  if (lane == 0) {
    c->g = g; c->t_next = t; c->n_out = n_out; c->status = status;
    c->collide_calls = cc; c->path_free_calls = pf; c->segments = ex_seg; c->samples = ex_smp;
  }
}

// Workgroup b (one wavefront) walks paths[b].  The path's arguments are read through the uniform pointer (scalar registers,
// like k_seq_waves_batch's); no workgroup ever waits for another one, so any grid size runs - what is not resident at once
// runs when a slot frees up.
__global__ __launch_bounds__(64) void k_smooth_paths(const SmoothPathArgs* __restrict__ paths, int n) {
  if ((int)blockIdx.x >= n) return;
  smooth_path_body(paths[blockIdx.x]);
}

hipError_t launch_smooth_paths(hipStream_t s, const SmoothPathArgs* paths_dev, int n, size_t lds) {
  if (n <= 0) return hipSuccess;
  const hipError_t e = set_dyn_lds(k_smooth_paths, lds, 48 * 1024);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_smooth_paths, dim3(n), dim3(64), lds, s, paths_dev, n);
  return hipGetLastError();
}
