// rrt_seq_batch.inc - session batches: the one-by-one loop of ONE RRT / RRT* / Multi-T-RRT session on ONE wavefront
// (kernels.h: RrtSeqArgs), included by kernels.hip behind the forest's loop, whose building blocks it strings together:
// lemire_pick, sq_knn, pose_exact, sq_edge_clear_fast / sq_path_free, grid_put.  Reference: Solve()'s loop src/rrt.h:93-99 and
// expandNode :128-322; on the host Rrt::run with wave == 1 and Rrt::expand.
//
// Evaluation is lazy exactly like the reference's - an edge is checked when the loop reaches it - so the reference-equivalent
// counters are the executed ones.  An iteration the loop cannot settle exactly is the host's (SFFK_RRT_HOST_ITER): a free edge
// to another live tree (link + merge rewrite tree lists, links and `eaten`), an exact tie of two distances in a tree that has
// eaten another (its list is no longer in id order, and the reference breaks ties by position in the list), a capacity.  The
// tests that can hand an iteration over all come BEFORE its first write: the other live trees are looked at ahead of
// choose-parent / append / rewire (their answer depends on neither), so rolling back means restoring five scalars.

// the k nearest nodes of one tree by a sweep of the store's tree column (lane j = j-th nearest, (distance, id) order): what a
// query for a small or distant tree costs through the grid grows with the cells between the query and the tree, a sweep with
// the number of nodes - four batches of 64 tree ids in flight, positions asked for only where the tree matches
__device__ __attribute__((noinline)) void rrt_knn_sweep(const NodeStoreMut& st, int n, const double* qp, int tree, int k, int lane, TopK& t,
                                                        int& have) {
  t.d = 1.0e300; t.id = 0x7fffffff;
  have = 0;
  if (k <= 0) return;
  for (int base = 0; base < n; base += 256) {
    int tr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = base + 64 * u + lane;
      tr[u] = j < n ? sq_i32(st.tree + j) : -1;
    }
    unsigned long long pw[4][6];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = base + 64 * u + lane;
      if (tr[u] == tree) {
        const unsigned long long* q8 = reinterpret_cast<const unsigned long long*>(st.pos + 6 * (size_t)j);
        for (int q = 0; q < 6; ++q) pw[u][q] = sq_u64(q8 + q);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (base + 64 * u >= n) continue;
      const int j = base + 64 * u + lane;
      const bool cv = tr[u] == tree;
      double d = 1.0e300;
      if (cv) {
        double p6[6];
        for (int q = 0; q < 6; ++q) p6[q] = __longlong_as_double((long long)pw[u][q]);
        d = dist6(p6, qp);
      }
      const double worst = topk_worst(t, k, have);
      const bool cand = cv && (have < k || key_less(d, j, worst, 0x7fffffff));
      topk_merge(t, lane, k, have, cand, d, cv ? j : 0x7fffffff);
    }
  }
}

// LAZY: the member is a lazy edge, LazyTSP::runRRT (src/lazy.h:160-284) - ONE tree from one root, so no tree is drawn (:178-182)
// and nothing of the other-trees step exists; k = (size_t)(2e log10(size + 1)) (:204); the new node within treeDistance of the
// goal ends the edge's search (:262-276, no edge check towards the goal): status SFFK_RRT_SOLVED.  All of it sits behind the
// template parameter - the other two instances are the code they were.
template <bool OPT, bool LAZY>
__device__ __forceinline__ void rrt_seq_body(const RrtSeqArgs& A) {
  extern __shared__ double lds_d[];
  __shared__ int32_t s_fh, s_ovf;
  RrtCtrl* c = A.ctrl;
  const int lane = threadIdx.x;
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
  // ---- the control block, in registers (everything here is the same in every lane)
  int n_nodes = c->n_nodes, iter = c->iter;
  unsigned long long cursor = c->cursor, cc = c->collide_calls, pf = c->path_free_calls, nq = c->nn_queries;
  unsigned long long ex_smp = 0;
  int status = SFFK_RRT_RAN, reason = 0;
  int lazy_last = -1;              // (LAZY) the node that reached the goal
  double lazy_distance = 0;        // (LAZY) distance(goal, that node) + the node's cost: the length of the edge (src/lazy.h:268)
  // (a lazy edge has one tree and never merges: what exists for a tree that has eaten another is dead in its instances)
  auto merged = [&]() { if constexpr (LAZY) return false; else return A.merged != 0; };
  const int n_live = A.n_live;
  // lane i speaks for the i-th live tree (frontier order) in the other-trees step
  const int my_live = lane < n_live ? A.live[lane] : -1;
  const GridView& g = A.g;
  // a nearest-node query goes through the grid or through the sweep, whichever looks cheaper (both are exact): the grid walks
  // the cube of cells up to the tree's typical node spacing - (cells per node of the tree)^(1/3) cells, ^(1/2) in a flat grid -,
  // the sweep every node of the store
  const float g_cells = (float)g.nx * (float)g.ny * (float)g.nz;
  auto knn = [&](const double* qp, int tree, int k, TopK& t, int& have) {
    const int tcnt = sq_i32(A.tree_cnt + tree);
    const float per = g_cells / (float)(tcnt > 0 ? tcnt : 1);
    const float w = 2.0f * (g.nz > 1 ? cbrtf(per) : sqrtf(per)) + 3.0f;
    const float walk = g.nz > 1 ? w * w * w : w * w;
    if (walk < (float)n_nodes) sq_knn(g, qp, tree, k, tcnt, A.cell_edge, A.knn_slack, lane, t, have);
    else rrt_knn_sweep(A.st, n_nodes, qp, tree, k, lane, t, have);
  };
  for (int it = 0; it < A.max_iters && iter < A.iter_limit; ++it) {
    if (n_nodes + 1 > A.node_cap || n_live > 64) { status = SFFK_RRT_HOST_ITER; reason = SFFK_RRT_WHY_CAPACITY; break; }
    if (cursor + 16ULL > A.words_end) break;                                     // out of engine words: the host tops the ring up
    if (sq_i32(g.ovf_cnt) > A.grid_ovf_limit) { status = SFFK_RRT_GRID; break; }  // the grid wants to re-cell itself
    // (iteration-start snapshot: an iteration handed to the host never happened here)
    const unsigned long long cur_a = cursor, cc_a = cc, pf_a = pf, nq_a = nq;
    const int iter_a = iter;
    auto hand_over = [&](int why) { cursor = cur_a; cc = cc_a; pf = pf_a; nq = nq_a; iter = iter_a; status = SFFK_RRT_HOST_ITER; reason = why; };
    // ---- 1. the tree to expand (:95): uniform_int(0, numTrees) over the live-tree list, a rejected word draws again
    // (LAZY: the one tree, no engine word - src/lazy.h:178-182)
    int pick = 0;
    if constexpr (!LAZY) {
      do { pick = lemire_pick(A.ring[cursor & A.ring_mask], (unsigned long long)A.pick_range); ++cursor; } while (pick < 0 && cursor < A.words_end);
      if (pick < 0) { cursor = cur_a; break; }
    }
    ++iter;
    const int mine = A.live[pick];
    // ---- 2. the steering target (:130-134): the goal with probability priorityBias, else randomPointInSpace (Y before X)
    // (LAZY: no goal bias, no word for it)
    double rnd[6];
    bool to_goal = false;
    if constexpr (!LAZY) {
      if (A.priority_bias != 0) { to_goal = uniform_real(A.ring[cursor & A.ring_mask], 0.0, 1.0) <= A.priority_bias; ++cursor; }
    }
    if (to_goal) {
      for (int k = 0; k < 6; ++k) rnd[k] = A.goal[k];
    } else {
      const double y = uniform_real(A.ring[cursor & A.ring_mask], A.limits[2], A.limits[3]);
      const double x = uniform_real(A.ring[(cursor + 1) & A.ring_mask], A.limits[0], A.limits[1]);
      cursor += 2;
      rnd[0] = x; rnd[1] = y; rnd[2] = 0; rnd[3] = rnd[4] = rnd[5] = 0;
      if (A.dim == 6) {
        rnd[2] = uniform_real(A.ring[cursor & A.ring_mask], A.limits[4], A.limits[5]);
        rnd[3] = uniform_real(A.ring[(cursor + 1) & A.ring_mask], -SFFG_PI, SFFG_PI);
        double phi = sffp::pacos(sample_acos_arg(A.ring[(cursor + 2) & A.ring_mask])) + SFFG_PI_2;
        if (uniform_real(A.ring[(cursor + 3) & A.ring_mask], 0.0, 1.0) < 0.5) { if (phi < 0) phi += SFFG_PI; else phi -= SFFG_PI; }
        rnd[4] = phi;
        rnd[5] = uniform_real(A.ring[(cursor + 4) & A.ring_mask], -SFFG_PI, SFFG_PI);
        cursor += 5;
      }
    }
    // ---- 3. nearest node of the tree (:143), getStateInDistance (:148)
    nq += 1;
    TopK nt{1.0e300, 0x7fffffff};
    int n_near = 0;
    knn(rnd, mine, merged() ? 2 : 1, nt, n_near);
    if (n_near < 1) { hand_over(SFFK_RRT_WHY_CAPACITY); break; }                  // (a live tree always holds its root)
    if constexpr (!LAZY) {
      if (n_near >= 2 && __shfl(nt.d, 0) == __shfl(nt.d, 1)) { hand_over(SFFK_RRT_WHY_TIE); break; }
    }
    int nearest = __shfl(nt.id, 0);
    double cpos[6], qp[6];
    for (int k = 0; k < 6; ++k) cpos[k] = sq_f64(A.st.pos + 6 * (size_t)nearest + k);
    steer(cpos, rnd, A.sampling_dist, qp);
    bool nan = false;
    for (int k = 0; k < 6; ++k) nan = nan || !(qp[k] == qp[k]);
    if (nan) { hand_over(SFFK_RRT_WHY_DEGENERATE); break; }
    // ---- 4. Collide(newPoint) and isPathFree(nearest, newPoint) (:149-151)
    cc += 1;
    bool hit = false;
    if (A.env.n_tri != 0 && !surely_clear(A.env, qp)) {
      double Rm[9], c3[3];
      if (qp[3] == 0 && qp[4] == 0 && qp[5] == 0) { Rm[0] = Rm[4] = Rm[8] = 1; Rm[1] = Rm[2] = Rm[3] = Rm[5] = Rm[6] = Rm[7] = 0; }
      else rotation(qp, Rm);
      xform(Rm, qp, A.rob.center, c3);
      hit = pose_exact(A.env, A.rob, rtri, stack, cand, stage, qp, Rm, c3, lane);
    }
    if (hit) continue;
    bool flt = false;
    pf += 1;
    if (!(sq_edge_clear_fast(A.env, cpos, qp, lane, cc, ex_smp) || sq_path_free(A.env, A.rob, rtri, stack, cand, queue, stage, cpos, qp, &s_fh, &s_ovf, lane, cc, ex_smp, flt))) continue;
    // ---- 8. the other live trees (:219-319), ahead of choose-parent / append / rewire (see above): per tree its nearest node,
    // which only matters inside treeDistance - every node of another tree in that ball, from the cells its box touches
    if constexpr (!LAZY) if (n_live > 1) {
      nq += (unsigned long long)(n_live - 1);
      const double r = A.dist_tree;
      double bd = 1.0e300;         // lane i: the nearest node of live tree i seen so far, and whether another one ties with it
      int bid = 0x7fffffff;
      bool btie = false;
      grid_ball_items(g, qp, ball_box_radius(r, A.sweep_abs_eps), lane, [&](bool valid, const GridItem* src) {   // one candidate per lane -> the lane of its tree
        bool h = false;
        double d = 0;
        int id = 0, tr = 0;
        if (valid) {
          double p6[6];
          grid_item_load(src, p6, id, tr);
          d = dist6(p6, qp);
          h = tr != mine && d < r;                               // :231 (no TOLERANCE here)
        }
        unsigned long long hm = __ballot(h);
        while (hm) {
          const int src_lane = __ffsll((long long)hm) - 1;
          hm &= hm - 1;
          const double sd = __shfl(d, src_lane);
          const int sid = __shfl(id, src_lane), str = __shfl(tr, src_lane);
          if (my_live == str) {
            if (sd == bd) btie = true;
            if (key_less(sd, sid, bd, bid)) { if (sd < bd) btie = false; bd = sd; bid = sid; }
          }
        }
      });
      // the trees that have a node in the ball, in frontier order (:219): tie -> host, edge (:231), free -> link + merge -> host
      unsigned long long todo = __ballot(bid != 0x7fffffff);
      int why = 0;
      while (todo && !why) {
        const int src_lane = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        if (merged() && __shfl((int)btie, src_lane)) { why = SFFK_RRT_WHY_TIE; break; }
        const int nb = __shfl(bid, src_lane);
        double np6[6];
        for (int k = 0; k < 6; ++k) np6[k] = sq_f64(A.st.pos + 6 * (size_t)nb + k);
        pf += 1;
        if (sq_edge_clear_fast(A.env, qp, np6, lane, cc, ex_smp) || sq_path_free(A.env, A.rob, rtri, stack, cand, queue, stage, qp, np6, &s_fh, &s_ovf, lane, cc, ex_smp, flt))
          why = SFFK_RRT_WHY_LINK;
      }
      if (why) { hand_over(why); break; }
    }
    // ---- 5. RRT* (:156-201): the k nearest of the tree around the new point, choose-parent in list order
    int par_new = nearest;
    double dcl_new, best;
    TopK mt{1.0e300, 0x7fffffff};
    int n_mem = 0;
    double m_droot = 0;
    if (OPT) {
      dcl_new = dist6(qp, cpos);
      best = dcl_new + sq_f64(A.d_root + nearest);
      // (size_t)(2e log10 N), :160; LAZY: N = size + 1 (src/lazy.h:204) - k is 1 when only the root exists
      const int k = __popcll(__ballot(lane > 0 && lane <= SFFK_STAR_KMAX + 1 && A.ktab[lane] <= n_nodes + (LAZY ? 1 : 0)));
      if (k > SFFK_STAR_KMAX) { hand_over(SFFK_RRT_WHY_CAPACITY); break; }
      nq += 1;                                                                              // :166 knnSearch
      if (k > 0) {
        knn(qp, mine, merged() ? k + 1 : k, mt, n_mem);
        if (merged()) {
          // (the list with one entry more: a tie inside it or at its boundary is the host's)
          const double dn = __shfl_down(mt.d, 1);
          if (__any(lane + 1 < n_mem && mt.d == dn)) { hand_over(SFFK_RRT_WHY_TIE); break; }
          if (n_mem > k) n_mem = k;
        }
        if (lane < n_mem) m_droot = sq_f64(A.d_root + mt.id);
        for (int m = 0; m < n_mem; ++m) {                                                   // :168-175
          const double nd = __shfl(mt.d, m) + __shfl(m_droot, m);
          if (nd < best - SFFG_TOL) {
            const int idm = __shfl(mt.id, m);
            double mp[6];
            for (int q = 0; q < 6; ++q) mp[q] = sq_f64(A.st.pos + 6 * (size_t)idm + q);
            pf += 1;
            if (sq_edge_clear_fast(A.env, qp, mp, lane, cc, ex_smp) || sq_path_free(A.env, A.rob, rtri, stack, cand, queue, stage, qp, mp, &s_fh, &s_ovf, lane, cc, ex_smp, flt)) {
              best = nd; par_new = idm; dcl_new = __shfl(mt.d, m);
            }
          }
        }
      }
    } else {                                                                                // :203
      dcl_new = A.sampling_dist;
      best = sq_f64(A.d_root + nearest) + A.sampling_dist;
    }
    // ---- 7. the new node (:205-215): store, records, grid
    const int idn = n_nodes;
    const int root_new = sq_i32(A.root_tree + par_new);
    if (lane == 0) {
      const size_t o = (size_t)idn;
      A.st.x[o] = (float)qp[0]; A.st.y[o] = (float)qp[1]; A.st.z[o] = (float)qp[2];
      A.st.yaw[o] = (float)qp[3]; A.st.pitch[o] = (float)qp[4]; A.st.roll[o] = (float)qp[5];
      for (int k = 0; k < 6; ++k) A.st.pos[6 * o + k] = qp[k];
      A.st.tree[o] = mine;
      A.parent[o] = par_new;
      A.root_tree[o] = root_new;
      A.d_closest[o] = dcl_new;
      A.d_root[o] = best;
      A.iter[o] = (uint32_t)iter;
      atomicAdd(A.tree_cnt + mine, 1);
      GridItem gi;
      for (int k = 0; k < 6; ++k) gi.p[k] = qp[k];
      gi.id = idn; gi.tree = mine; gi.pad[0] = gi.pad[1] = 0;
      grid_put(g, gi);
    }
    sq_drain();
    ++n_nodes;
    if (OPT) {
      // ---- rewire (:181-201): a neighbour the new node's cost improves, if the edge neighbour -> new is free
      for (int m = 0; m < n_mem; ++m) {
        const double dm = __shfl(mt.d, m), drm = __shfl(m_droot, m);
        const double proposed = best + dm;
        if (proposed < drm - SFFG_TOL) {
          const int idm = __shfl(mt.id, m);
          double mp[6];
          for (int q = 0; q < 6; ++q) mp[q] = sq_f64(A.st.pos + 6 * (size_t)idm + q);
          pf += 1;
          if (sq_edge_clear_fast(A.env, mp, qp, lane, cc, ex_smp) || sq_path_free(A.env, A.rob, rtri, stack, cand, queue, stage, mp, qp, &s_fh, &s_ovf, lane, cc, ex_smp, flt)) {
            if (lane == 0) { A.parent[idm] = idn; A.root_tree[idm] = root_new; A.d_closest[idm] = dm; A.d_root[idm] = proposed; }
          }
        }
      }
      sq_drain();
    }
    if constexpr (LAZY) {
      // ---- the goal test (src/lazy.h:262-276), behind the rewires as in the reference (none of them touches the new node's cost)
      const double gd = dist6(A.goal, qp);
      if (gd < A.dist_tree) { status = SFFK_RRT_SOLVED; lazy_last = idn; lazy_distance = gd + best; break; }
    }
  }
  if (lane == 0) {
    c->n_nodes = n_nodes; c->iter = iter;
    c->status = status; c->reason = reason;
    c->grid_ovf = sq_i32(g.ovf_cnt);
    c->cursor = cursor; c->collide_calls = cc; c->path_free_calls = pf; c->nn_queries = nq;
    if constexpr (LAZY) { c->lazy_last = lazy_last; c->lazy_distance = lazy_distance; }
  }
}

// Session batches: workgroup b (one wavefront) runs the loop of members[b], an independent session with a store, a grid, a
// ring and a control block of its own.  The member's arguments are read through the uniform pointer (scalar registers, like
// k_seq_waves_batch's); no workgroup ever waits for another one, so any grid size runs - what is not resident at once runs when a
// slot frees up.
template <bool OPT, bool LAZY>
__global__ __launch_bounds__(64) void k_rrt_seq_batch(const RrtSeqArgs* __restrict__ members, int n) {
  if ((int)blockIdx.x >= n) return;
  rrt_seq_body<OPT, LAZY>(members[blockIdx.x]);
}

template <bool OPT, bool LAZY>
static hipError_t launch_rrt_seq_batch_as(hipStream_t s, const RrtSeqArgs* members_dev, int n, size_t lds) {
  const hipError_t e = set_dyn_lds(k_rrt_seq_batch<OPT, LAZY>, lds, 48 * 1024);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_rrt_seq_batch<OPT, LAZY>), dim3(n), dim3(64), lds, s, members_dev, n);
  return hipGetLastError();
}
hipError_t launch_rrt_seq_batch(hipStream_t s, const RrtSeqArgs* members_dev, int n, bool optimize, bool lazy, size_t lds) {
  if (n <= 0) return hipSuccess;
  if (lazy) return optimize ? launch_rrt_seq_batch_as<true, true>(s, members_dev, n, lds) : launch_rrt_seq_batch_as<false, true>(s, members_dev, n, lds);
  return optimize ? launch_rrt_seq_batch_as<true, false>(s, members_dev, n, lds) : launch_rrt_seq_batch_as<false, false>(s, members_dev, n, lds);
}
