// seq_waves_body.inc - the loop of ONE forest of waves of one slot on ONE wavefront (kernels.h: SeqArgs): the body of
// seq_waves_body<OPT, PRIO, GOAL>(const SeqArgs& A) in kernels.hip, included there once.  k_seq_waves_batch, the loop's only
// entry, calls it on the workgroup's member of the argument array; a single forest is a batch of one.  It stays a function
// the kernel calls, not text in the kernel: through the function the SFF* instance spills 366 scalars, as included text 517
// (- 11 %, measured).  Nothing in here looks at the workgroup's index.
// lemire_pick, the sq_* loads and the one-slot idioms (grid_ball_items, nb_rank, border_*, trees_connected) are kernels_dev.h's.
// PRIO (the template parameter beside OPT): the priority-frontier mode of a forest without a goal (src/forest.h:126-147,
// 160-181, 360-363; PrioView).  The wave's node comes from a heap of a tree (pop / pop at a drawn index), an accepted node
// is pushed onto every heap of its tree at once, an exhausted node leaves the tree's other heaps, an expanded one goes back
// onto its own - the heap routines of prio_heap_dev.h, on this one wavefront.  Heap sizes and, per tree, the number of
// non-empty heaps are kept in LDS (and written through to PrioView::size); the frontier list is not used.  Everything of
// the mode stands in `if constexpr (PRIO)`: the instances without it compile to what they were.
// GOAL (the third template parameter): Problem::hasGoal, the single-query mode (src/forest.h:91-109,
// 196-201, 283-299, 369-372; f.goal_id = the goal's node, the one node of tree R - 1, never on the frontier or the closed
// list).  A qualifying neighbour of another tree rejects the attempt without an edge check unless it is the goal; the goal
// costs one isPathFree(newPoint, goal), and a free one makes the attempt the solving one: it is appended like any accepted
// attempt (SFF*: choose parent and rewires as usual), one border (new node, goal) is written behind it, solved ends the
// loop.  Nothing else solves a goal forest: the connectivity test at a wave's end does not run.  Everything of the mode
// stands in `if constexpr (GOAL)`.
// PRIO && GOAL: the two compose.  A start tree has ONE heap, keyed by the distance to the goal (src/forest.h:104-108); the
// goal's tree R - 1 has none (PrioView::base[R - 1] == base[R], p_tne[R - 1] stays 0), so a tree draw - over all R trees,
// :128 - that lands on it is redrawn like any tree whose heaps are empty, and the heap draw, randomIntMinMax(0, 0), still
// takes its engine word (lemire_pick(word, 1) is 0 for every word).  The neighbour loop and the solving attempt are GOAL's,
// the pick, the pushes and the wave's end PRIO's: empty_frontier is "every heap empty", with every heap empty the picks are
// closed-list picks (w_heap < 0, prio_wave 0) whose children fill the heaps again, and a list fault - the goal's edge check
// included - leaves the wave as PRIO leaves it, for the host-replay engine, which knows both modes.  Only one thing is
// particular to the pair, an `if constexpr (!GOAL)` inside PRIO's wave end: an exhausted node has no other heap to leave.
  extern __shared__ double lds_d[];
  __shared__ int32_t s_fh, s_ovf;
  __shared__ int32_t h_id[64], h_tree[64];
  __shared__ double h_d[64], h_pos[64 * 6];
  const DevForestView& f = A.f;
  DevCtrl* c = f.ctrl;
  const int lane = threadIdx.x;
  if (c->halt || c->in_wave) return;            // (a wave the host left half done goes through the round engine)
  __shared__ int32_t p_size[PRIO ? SFFK_PRIO_MAX_HEAPS : 1];   // PRIO: entries per heap
  __shared__ int32_t p_tne[PRIO ? 64 : 1];                     // PRIO: per tree, its non-empty heaps
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
  int n_nodes = c->n_nodes, iter = c->iter, fn = c->frontier_n, cn = c->closed_n, nb = c->n_borders;
  int solved = c->solved, empty_frontier = c->empty_frontier, terminated = c->terminated;
  const int front_sel = c->front_sel;
  unsigned long long cursor = c->cursor, cc = c->collide_calls, pf = c->path_free_calls, nq = c->nn_queries;
  unsigned long long ex_pose = c->poses_executed, ex_seg = c->segments_executed, ex_smp = c->samples_executed;
  unsigned long long waves = c->waves, rounds = c->rounds, rnodes = c->round_nodes, rqueries = c->round_queries, redraws = 0;
  int32_t* frontier = front_sel ? f.frontier2 : f.frontier;
  const int TM = f.threshold_misses, WP = f.words_per, R = f.n_trees;
  int fault = 0, w_round = 0, w_node = 0, w_pos = 0, w_closed = 0, in_wave = 0;
  unsigned long long st_rounds = 0, st_members = 0, st_rewires = 0;
  // phase clocks (10 ns ticks): pick + node, sample, pose, parent edge, neighbour query, neighbour loop, append, wave end
  uint64_t pre_w[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long pre_at = ~0ULL;
  [[maybe_unused]] int total_ne = 0, w_tree = 0, w_heap = -1;   // PRIO: non-empty heaps; the heap the wave's node came from (-1: none)
  if constexpr (PRIO) {
    const PrioView& P = f.prio;
    for (int h = lane; h < P.n_heaps; h += 64) p_size[h] = sq_i32(P.size + h);
    __builtin_amdgcn_wave_barrier();
    if (lane < R) {
      int ne = 0;
      for (int h = P.base[lane]; h < P.base[lane + 1]; ++h) ne += p_size[h] > 0 ? 1 : 0;
      p_tne[lane] = ne;
    }
    __builtin_amdgcn_wave_barrier();
    for (int t = 0; t < R; ++t) total_ne += uni_i32(p_tne[t]);
  }
  // PRIO: heap h holds n entries from here on (LDS, and the size array the host and the round engine read)
  [[maybe_unused]] auto p_resize = [&](int t, int h, int was, int n) {
    if (lane == 0) { p_size[h] = n; f.prio.size[h] = n; }
    if ((was > 0) != (n > 0)) {
      if (lane == 0) p_tne[t] += n > 0 ? 1 : -1;
      total_ne += n > 0 ? 1 : -1;
    }
    __builtin_amdgcn_wave_barrier();
  };
  const bool clk = A.f.profile != 0;   // (a clock read is a scalar memory round trip)
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tq = clk ? wall_clock64() : 0ULL;
  auto lap = [&](int k) { if (!clk) return; const unsigned long long t = wall_clock64(); ph[k] += t - tq; tq = t; };
  for (int wv = 0; wv < A.max_waves && !terminated && !fault; ++wv) {
    // ---- what the round engine checks before a round (round_begin_scalars), and what this launch has to leave to the host
    if (n_nodes + 1 > f.node_cap - 8 || nb + TM > f.border_cap) { fault = SFFK_FAULT_CAPACITY; break; }
    if ((unsigned long long)(nb + TM) * 2ULL > f.bt_mask + 1ULL) { fault = SFFK_FAULT_BORDER_TABLE; break; }
    if (cursor + 8ULL + (unsigned long long)(TM * WP) > A.words_end) break;      // out of engine words: the host tops the ring up
    if (sq_i32(A.grid_ovf_src) > A.grid_ovf_limit) break;                         // the grid wants to re-cell itself
    [[maybe_unused]] int hp_node = -1;
    if constexpr (PRIO) {
      if (n_nodes + 1 > f.prio.cap) { fault = SFFK_FAULT_INTERNAL; break; }     // (never: a heap holds what the forest can, dev_prio_upload)
      // ---- node selection, priority frontier (src/forest.h:126-147): a tree with a non-empty heap, a non-empty heap of
      // it, the coin - every draw checks the word supply (the redraws are not bounded); nothing is popped, and the cursor
      // stays, unless the whole pick and the wave's attempts have their words
      w_heap = -1;
      if (!empty_frontier && total_ne > 0) {
        const PrioView& P = f.prio;
        unsigned long long at = cursor;
        bool dry = false;
        auto draw = [&](int range) -> int {      // RandGen::randomIntMinMax(0, range - 1); -1 = redraw (or out of words)
          if (at >= A.words_end) { dry = true; return -1; }
          const int v = lemire_pick(f.ring[at & f.ring_mask], (unsigned long long)range);
          ++at;
          return v;
        };
        int t = -1, hp = -1, idx = -1, b0 = 0, size = 0;
        while (!dry && (t < 0 || uni_i32(p_tne[t]) == 0)) t = draw(R);
        if (!dry) {
          b0 = P.base[t];
          const int nh = P.base[t + 1] - b0;
          while (!dry && (hp < 0 || uni_i32(p_size[b0 + hp]) == 0)) hp = draw(nh);
        }
        if (!dry) {
          size = uni_i32(p_size[b0 + hp]);
          if (at >= A.words_end) dry = true;
          else {
            const bool top = uniform_real(f.ring[at & f.ring_mask], 0.0, 1.0) <= P.bias;   // :143-147
            ++at;
            while (!top && !dry && idx < 0) idx = draw(size);
          }
        }
        if (dry || at + (unsigned long long)(TM * WP) > A.words_end) break;
        cursor = at;
        HeapRef hr = heap_with(P, b0 + hp, size);
        hp_node = idx < 0 ? heap_pop(hr) : heap_pop_at(hr, idx);
        p_resize(t, b0 + hp, size, size - 1);
        w_tree = t; w_heap = b0 + hp;
      }
    }
    // ---- node selection (src/forest.h:136-151)
    const int use_closed = (PRIO && w_heap >= 0) ? 0 : (cn > 0 && empty_frontier);
    const int pool = use_closed ? cn : fn;
    int pick = 0, node;
    if (PRIO && w_heap >= 0) node = hp_node;
    else {
      if (pool < 1) { terminated = 1; break; }
      do { pick = lemire_pick(f.ring[cursor & f.ring_mask], (unsigned long long)pool); ++cursor; if (pick < 0) ++redraws; } while (pick < 0);
      node = sq_i32((use_closed ? f.closed : frontier) + pick);
    }
    ++waves;
    double cpos[6];
    for (int k = 0; k < 6; ++k) cpos[k] = sq_f64(A.st.pos + 6 * (size_t)node + k);
    const int mine = sq_i32(A.st.tree + node);
    const double droot_ex = sq_f64(f.d_root + node);
    const bool force = (sq_u8(f.nflag + node) & 1) != 0;
    bool failing = true;
    w_node = node; w_pos = pick; w_closed = use_closed;
    lap(0);
    for (int rd = 0; rd < TM && failing && iter < f.max_iterations; ++rd) {
      // (attempt-start snapshot: a fault rolls exactly this attempt back)
      const int iter_a = iter;
      const unsigned long long cur_a = cursor, cc_a = cc, pf_a = pf, nq_a = nq, xp_a = ex_pose, xs_a = ex_seg, xm_a = ex_smp;
      bool flt = false;
      // (the words of this attempt were asked for while the previous one ran, whenever the stream position was the
      // expected one; the next attempt's are asked for now)
      uint64_t w[6];
      if (pre_at == cursor) { for (int k = 0; k < 6; ++k) w[k] = pre_w[k]; }
      else { for (int k = 0; k < 6; ++k) w[k] = k < WP ? f.ring[(cursor + k) & f.ring_mask] : 0ULL; }
      pre_at = cursor + (unsigned long long)WP;
      for (int k = 0; k < 6; ++k) pre_w[k] = k < WP ? f.ring[(pre_at + k) & f.ring_mask] : 0ULL;
      SampleTrig ht{};
      if (A.trig) {
        const double* t0 = A.trig + 3 * (size_t)(cursor & f.ring_mask);
        ht.c_phi = t0[0]; ht.s_phi = t0[1];
        if (WP == 6) {
          const double* t1 = A.trig + 3 * (size_t)((cursor + 1) & f.ring_mask);
          const double* t3 = A.trig + 3 * (size_t)((cursor + 3) & f.ring_mask);
          ht.c_theta = t1[0]; ht.s_theta = t1[1]; ht.acos_u = t3[2];
        }
      }
      cursor += (unsigned long long)WP;
      ++iter;
      ++rounds; rnodes += (unsigned long long)(n_nodes + 1); ++rqueries;
      double qp[6];
      if (!A.trig) {
        // the five transcendental values of the sample, two at a time: lanes 0 / 1 evaluate the same function on phi / theta
        // (one instruction stream whatever the lane count; the same portable routines, so the same bits as sample_point)
        const double ang = sample_angle(lane == 1 ? w[1] : w[0]);
        const double sv = sffp::psin(ang), cv = sffp::pcos(ang);
        ht.s_phi = __shfl(sv, 0); ht.c_phi = __shfl(cv, 0);
        ht.s_theta = __shfl(sv, 1); ht.c_theta = __shfl(cv, 1);
        ht.acos_u = WP == 6 ? sffp::pacos(sample_acos_arg(w[3])) : 0.0;
      }
      const bool ok = sample_point_with(w, cpos, A.sampling_dist, A.dim, A.limits, qp, ht);
      lap(1);
      if (!ok) continue;                                           // :246 !result
      // ---- Environment::Collide(newPoint)
      cc += 1; ex_pose += 1;
      bool hit = false;
      if (A.env.n_tri != 0 && !surely_clear(A.env, qp)) {
        double Rm[9], c3[3];
        if (qp[3] == 0 && qp[4] == 0 && qp[5] == 0) { Rm[0] = Rm[4] = Rm[8] = 1; Rm[1] = Rm[2] = Rm[3] = Rm[5] = Rm[6] = Rm[7] = 0; }
        else rotation(qp, Rm);
        xform(Rm, qp, A.rob.center, c3);
        hit = pose_exact(A.env, A.rob, rtri, stack, cand, stage, qp, Rm, c3, lane);
      }
      lap(2);
      if (hit) continue;
      // ---- isPathFree(expanded, newPoint)
      pf += 1; ex_seg += 1;
      const bool free0 = (sq_edge_clear_fast(A.env, cpos, qp, lane, cc, ex_smp) || sq_path_free(A.env, A.rob, rtri, stack, cand, queue, stage, cpos, qp, &s_fh, &s_ovf, lane, cc, ex_smp, flt));
      bool reject = !free0;
      lap(3);
      const double pdist = dist6(cpos, qp);                        // parentDistance, :250
      int n_hit = 0;
      [[maybe_unused]] bool solving = false;                       // GOAL: this attempt saw the goal over a free edge (:287)
      [[maybe_unused]] double gpos[6] = {0, 0, 0, 0, 0, 0};
      if (!flt && !reject) {
        nq += (unsigned long long)R;                               // :262-267 one radiusSearch per tree
        // ---- the neighbours: exact 6-D ball of radius max(parentDistance, treeDistance) from the cells its box touches
        const double r = pdist > A.dist_tree ? pdist : A.dist_tree;
        grid_ball_items(A.g, qp, ball_box_radius(r, A.sweep_abs_eps), lane, [&](bool valid, const GridItem* src) {   // one candidate per lane -> the hit list in LDS
          bool h = false;
          double d = 0, p6[6];
          int id = 0, tr = 0;
          if (valid) {
            grid_item_load(src, p6, id, tr);
            d = dist6(p6, qp);
            h = d < r;
          }
          const unsigned long long hm = __ballot(h);
          if (h) {
            const int at = n_hit + __popcll(hm & ((1ULL << lane) - 1ULL));
            if (at < 64) { h_id[at] = id; h_tree[at] = tr; h_d[at] = d; for (int k = 0; k < 6; ++k) h_pos[6 * at + k] = p6[k]; }
          }
          n_hit += __popcll(hm);
        });
        if (n_hit > A.hit_cap || n_hit > 64) flt = true;
      }
      lap(4);
      if (!flt && !reject) {
        // ---- the neighbour loop (:270-300) in the reference's order: tree id, then distance, then id; an edge is only
        // checked when the loop reaches it
        __builtin_amdgcn_wave_barrier();
        const bool have = lane < n_hit;
        const int id = have ? h_id[lane] : 0x7fffffff;
        const int t = have ? h_tree[lane] : 0x7fffffff;
        const double d = have ? h_d[lane] : 0.0;
        const bool same = t == mine;
        const bool qk = have && (same ? (!force && d < pdist - SFFG_TOL) : (d < A.dist_tree - SFFG_TOL));   // :276 / :283
        const int rank = nb_rank(n_hit, t, d, id, qk);
        const int n_q = __popcll(__ballot(qk));
        for (int rk = 0; rk < n_q && !reject && !flt; ++rk) {
          const unsigned long long sel = __ballot(qk && rank == rk);
          const int src = __ffsll((long long)sel) - 1;
          const int s_same = __shfl((int)same, src), s_id = __shfl(id, src), s_tree = __shfl(t, src);
          double np6[6];
          for (int k = 0; k < 6; ++k) np6[k] = h_pos[6 * src + k];
          if constexpr (GOAL) {
            if (!s_same) {                                         // :283-299 with a goal: no border list, no edge but the goal's
              if (s_id != f.goal_id) { reject = true; break; }
              pf += 1; ex_seg += 1;
              const bool fr = (sq_edge_clear_fast(A.env, qp, np6, lane, cc, ex_smp) || sq_path_free(A.env, A.rob, rtri, stack, cand, queue, stage, qp, np6, &s_fh, &s_ovf, lane, cc, ex_smp, flt));
              // :296 not rejected: the walk goes on (and ends here: the goal's tree is the last one and holds this one node)
              if (fr && !flt) { solving = true; for (int k = 0; k < 6; ++k) gpos[k] = np6[k]; }
              else reject = true;
              continue;
            }
          }
          pf += 1; ex_seg += 1;
          if (s_same) {
            const bool fr = (sq_edge_clear_fast(A.env, np6, qp, lane, cc, ex_smp) || sq_path_free(A.env, A.rob, rtri, stack, cand, queue, stage, np6, qp, &s_fh, &s_ovf, lane, cc, ex_smp, flt));
            if (fr) reject = true;                                 // :276-280 overcrowded
          } else {
            const bool fr = (sq_edge_clear_fast(A.env, cpos, np6, lane, cc, ex_smp) || sq_path_free(A.env, A.rob, rtri, stack, cand, queue, stage, cpos, np6, &s_fh, &s_ovf, lane, cc, ex_smp, flt));
            if (fr && !flt) {                                      // :288-294 border entry unless the pair has one
              const int a = s_id < node ? s_id : node, b = s_id < node ? node : s_id;
              const unsigned long long key = border_key(a, b);
              size_t h;
              if (border_probe<true>(f, key, h)) {
                if (lane == 0) {
                  f.bt_key[h] = key;
                  f.bt_val[h] = c->epoch << 32;
                  f.b_n1[nb] = a; f.b_n2[nb] = b;
                  f.b_ta[nb] = s_tree < mine ? s_tree : mine; f.b_tb[nb] = s_tree < mine ? mine : s_tree;
                  f.b_dist[nb] = sq_f64(f.d_root + s_id) + droot_ex + dist6(np6, cpos);
                  f.pair[(size_t)s_tree * R + mine] = 1;
                  f.pair[(size_t)mine * R + s_tree] = 1;
                }
                sq_drain();
                ++nb;
              }
            }
            reject = true;                                         // :296-299
          }
        }
      }
      lap(5);
      if (flt) {
        // a bounded list overflowed (hits, triangle candidates): this attempt never happened - the host finishes the wave
        iter = iter_a; cursor = cur_a; cc = cc_a; pf = pf_a; nq = nq_a; ex_pose = xp_a; ex_seg = xs_a; ex_smp = xm_a;
        --rounds; rnodes -= (unsigned long long)(n_nodes + 1); --rqueries;
        fault = SFFK_FAULT_LISTS; w_round = rd; in_wave = 1;
        break;
      }
      if (reject) continue;
      // ---- SFF* (:307-351): the k nearest of the tree, choose parent, (the node), rewire - each edge checked when its turn comes
      int par_new = node;
      double dcl_new = pdist, best = pdist + droot_ex;
      TopK mt{1.0e300, 0x7fffffff};
      int n_mem = 0;
      double m_droot = 0;
      if (OPT) {
        const int k = __popcll(__ballot(lane > 0 && lane <= SFFK_STAR_KMAX + 1 && A.ktab[lane] <= n_nodes));   // (size_t)(2e log10 N), :309
        if (k > SFFK_STAR_KMAX) flt = true;
        else {
          nq += 1;                                                                          // :317 knnSearch
          sq_knn(A.g, qp, mine, k, sq_i32(A.tree_cnt + 16 * mine), A.cell_edge, A.knn_slack, lane, mt, n_mem);
          if (lane < n_mem) m_droot = sq_f64(f.d_root + mt.id);
          for (int m = 0; m < n_mem && !flt; ++m) {                                         // :320-327
            const double nd = __shfl(mt.d, m) + __shfl(m_droot, m);
            if (nd < best - SFFG_TOL) {
              const int idm = __shfl(mt.id, m);
              double mp[6];
              for (int q = 0; q < 6; ++q) mp[q] = sq_f64(A.st.pos + 6 * (size_t)idm + q);
              pf += 1; ex_seg += 1;
              if ((sq_edge_clear_fast(A.env, qp, mp, lane, cc, ex_smp) || sq_path_free(A.env, A.rob, rtri, stack, cand, queue, stage, qp, mp, &s_fh, &s_ovf, lane, cc, ex_smp, flt)) && !flt) {
                best = nd; par_new = idm; dcl_new = __shfl(mt.d, m);
              }
            }
          }
        }
        if (flt) {
          iter = iter_a; cursor = cur_a; cc = cc_a; pf = pf_a; nq = nq_a; ex_pose = xp_a; ex_seg = xs_a; ex_smp = xm_a;
          --rounds; rnodes -= (unsigned long long)(n_nodes + 1); --rqueries;
          fault = SFFK_FAULT_LISTS; w_round = rd; in_wave = 1;
          break;
        }
      }
      // ---- the new node (:329, :353-367)
      const int idn = n_nodes;
      if (lane == 0) {
        const size_t o = (size_t)idn;
        A.st.x[o] = (float)qp[0]; A.st.y[o] = (float)qp[1]; A.st.z[o] = (float)qp[2];
        A.st.yaw[o] = (float)qp[3]; A.st.pitch[o] = (float)qp[4]; A.st.roll[o] = (float)qp[5];
        for (int k = 0; k < 6; ++k) A.st.pos[6 * o + k] = qp[k];
        A.st.tree[o] = mine;
        f.parent[o] = par_new;
        f.d_closest[o] = dcl_new;
        f.d_root[o] = best;
        f.iter[o] = (uint32_t)iter;
        f.nflag[o] = PRIO ? 0 : 2;                 // (PRIO: no frontier list - the tree's heaps, below)
        if (!PRIO) frontier[fn] = idn;
        if (OPT) {
          atomicAdd(A.tree_cnt + 16 * mine, 1);
          if (A.hist) {
            const int at = atomicAdd(A.hist_ctl, 1);
            if (at < A.hist_cap) { A.hist[3 * (size_t)at] = idn; A.hist[3 * (size_t)at + 1] = par_new; A.hist[3 * (size_t)at + 2] = iter; }
            else A.hist_ctl[1] = 1;
          }
        }
        GridItem it;
        for (int k = 0; k < 6; ++k) it.p[k] = qp[k];
        it.id = idn; it.tree = mine; it.pad[0] = it.pad[1] = 0;
        grid_put(A.g, it);
      }
      sq_drain();
      ++n_nodes;
      if (!PRIO) ++fn;
      failing = false;
      if constexpr (PRIO) {   // :360-363 onto every heap of its tree, in heap order
        const PrioView& P = f.prio;
        for (int h = P.base[mine]; h < P.base[mine + 1]; ++h) {
          double ref[6];
          for (int k = 0; k < 6; ++k) ref[k] = P.ref[6 * (size_t)h + k];
          const int was = uni_i32(p_size[h]);
          HeapRef hr = heap_with(P, h, was);
          heap_push(hr, idn, hk_bits(dist6(qp, ref)));
          p_resize(mine, h, was, was + 1);
        }
        sq_drain();
      }
      if (OPT) {
        // rewire (:332-350): a member the new node's cost improves, if the edge member -> new is free
        ++st_rounds; st_members += (unsigned long long)n_mem;
        for (int m = 0; m < n_mem; ++m) {
          const double dm = __shfl(mt.d, m), drm = __shfl(m_droot, m);
          const double proposed = best + dm;
          if (proposed < drm - SFFG_TOL) {
            const int idm = __shfl(mt.id, m);
            double mp[6];
            for (int q = 0; q < 6; ++q) mp[q] = sq_f64(A.st.pos + 6 * (size_t)idm + q);
            pf += 1; ex_seg += 1;
            bool f2 = false;
            const bool fr = (sq_edge_clear_fast(A.env, mp, qp, lane, cc, ex_smp) || sq_path_free(A.env, A.rob, rtri, stack, cand, queue, stage, mp, qp, &s_fh, &s_ovf, lane, cc, ex_smp, f2));
            if (fr) {
              if (lane == 0) {
                f.parent[idm] = idn; f.d_closest[idm] = dm; f.d_root[idm] = proposed;
                if (A.hist) {
                  const int at = atomicAdd(A.hist_ctl, 1);
                  if (at < A.hist_cap) { A.hist[3 * (size_t)at] = idm; A.hist[3 * (size_t)at + 1] = idn; A.hist[3 * (size_t)at + 2] = iter; }
                  else A.hist_ctl[1] = 1;
                }
              }
              ++st_rewires;
            }
          }
        }
        sq_drain();
      }
      if constexpr (GOAL) {
        if (solving) {   // :369-372 the one border of a goal forest: (new node, goal), cost after choose-parent
          const int gid = f.goal_id;
          const int a = gid < idn ? gid : idn, b = gid < idn ? idn : gid;
          const unsigned long long key = border_key(a, b);
          size_t h;
          (void)border_probe<true>(f, key, h);                     // (the new node has no entry yet: the first free slot)
          if (lane == 0) {
            f.bt_key[h] = key;
            f.bt_val[h] = c->epoch << 32;
            f.b_n1[nb] = a; f.b_n2[nb] = b;
            f.b_ta[nb] = mine; f.b_tb[nb] = R - 1;
            f.b_dist[nb] = best + dist6(qp, gpos);
            f.pair[(size_t)(R - 1) * R + mine] = 1;
            f.pair[(size_t)mine * R + (R - 1)] = 1;
          }
          sq_drain();
          ++nb;
          solved = 1;
        }
      }
      lap(6);
    }
    if (fault) break;
    // ---- the slot is exhausted: its node leaves the frontier for the closed list (:160-178; the erase keeps the order)
    if constexpr (PRIO) {
      // (:160-181) a node that came from a heap: exhausted, it leaves the tree's OTHER heaps - where it stands in each comes
      // from the position maps, a lane per heap - and joins the closed list; expanded, it goes back onto its own heap,
      // behind the new node's push
      if (w_heap >= 0) {
        const PrioView& P = f.prio;
        if (failing) {
          if constexpr (!GOAL) {
          const int b0 = P.base[w_tree], nh = P.base[w_tree + 1] - b0;
          const int at_v = lane < nh ? hl_i32(P.pos + (size_t)(b0 + lane) * P.cap + node) : -1;
          for (int j = 0; j < nh; ++j) {
            const int hint = lane_i32(at_v, j);
            if (b0 + j == w_heap || hint < 0) continue;
            const int was = uni_i32(p_size[b0 + j]);
            HeapRef hr = heap_with(P, b0 + j, was);
            heap_remove(hr, node, hint);
            p_resize(w_tree, b0 + j, was, hr.n);
          }
          }   // (GOAL: the tree's one heap is the one the node was popped from - nothing to leave, :165-175)
          const int fl = sq_u8(f.nflag + node);
          if (!(fl & 1)) {
            if (lane == 0) { f.nflag[node] = (uint8_t)((fl & ~2) | 1); f.closed[cn] = node; }
            ++cn;
          }
        } else {
          double ref[6];
          for (int k = 0; k < 6; ++k) ref[k] = P.ref[6 * (size_t)w_heap + k];
          const int was = uni_i32(p_size[w_heap]);
          HeapRef hr = heap_with(P, w_heap, was);
          heap_push(hr, node, hk_bits(dist6(cpos, ref)));
          p_resize(w_tree, w_heap, was, was + 1);
        }
      }
    } else if (failing && !use_closed) {
      const int fl = sq_u8(f.nflag + node);
      if (fl & 2) {
        if (lane == 0) { f.nflag[node] = (uint8_t)((fl & ~2) | 1); f.closed[cn] = node; }
        ++cn;
        for (int j0 = pick; j0 < fn - 1; j0 += 256) {
          int v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) { const int j = j0 + 64 * u + lane; v[u] = j < fn - 1 ? sq_i32(frontier + j + 1) : 0; }
#pragma unroll
          for (int u = 0; u < 4; ++u) { const int j = j0 + 64 * u + lane; if (j < fn - 1) frontier[j] = v[u]; }
          sq_drain();
        }
        --fn;
      }
    }
    sq_drain();
    // ---- termination (:184-201)
    empty_frontier = PRIO ? (total_ne == 0 ? 1 : 0) : (fn == 0 ? 1 : 0);   // (PRIO: every heap of every tree is empty, :184-191)
    bool conn_test = !solved && empty_frontier;
    if constexpr (GOAL) conn_test = false;   // :198 with a goal only reaching it solves
    if (conn_test) {
      if (R <= 64) solved = trees_connected(f.pair, R, lane) ? 1 : 0;   // maxConnected() == numRoots
      else fault = SFFK_FAULT_LISTS;   // (more trees than lanes: the round engine's serial walk)
    }
    const bool budget = f.node_budget > 0 && n_nodes >= f.node_budget;
    terminated = (solved || iter >= f.max_iterations || budget) ? 1 : 0;
    if (A.trace && wv < A.trace_cap && lane == 0) {
      int32_t* t = A.trace + 8 * (size_t)wv;
      t[0] = node; t[1] = pick; t[2] = iter; t[3] = (int32_t)(cursor & 0x7fffffffULL); t[4] = failing ? TM : 0; t[5] = n_nodes; t[6] = fn; t[7] = cn;
    }
    lap(7);
  }
  if (lane == 0) {
    for (int k = 0; k < 8; ++k) c->wprof[k] += ph[k];
    c->n_nodes = n_nodes; c->iter = iter; c->frontier_n = fn; c->closed_n = cn; c->n_borders = nb;
    c->solved = solved; c->empty_frontier = empty_frontier; c->terminated = terminated;
    c->cursor = cursor; c->collide_calls = cc; c->path_free_calls = pf; c->nn_queries = nq;
    c->poses_executed = ex_pose; c->segments_executed = ex_seg; c->samples_executed = ex_smp;
    c->waves = waves; c->rounds = rounds; c->round_nodes = rnodes; c->round_queries = rqueries;
    c->redraws += (int)redraws;
    c->star_rounds += st_rounds; c->star_passes += st_rounds; c->star_members += st_members; c->star_rewires += st_rewires;
    c->n_act = 0; c->app_n = 0; c->compact_from = 0;
    c->grid_ovf = sq_i32(A.grid_ovf_src); c->tgrid_ovf = 0;
    c->fault = fault;
    c->halt = (terminated || fault) ? 1 : 0;
    c->in_wave = in_wave;
    if constexpr (PRIO) {   // (the loop pushes at acceptance: nothing is pending at any wave's end, or in a wave half done)
      c->prio_n0 = n_nodes; c->prio_all_empty = total_ne == 0 ? 1 : 0;
      c->prio_wave = (in_wave && w_heap >= 0) ? 1 : 0;
      if (in_wave && w_heap >= 0) { f.prio.slot_tree[0] = w_tree; f.prio.slot_heap[0] = w_heap - f.prio.base[w_tree]; }
    }
    if (in_wave) {   // the state the host engine resumes the wave from: its one slot, still failing, w_round rounds done
      c->round = w_round; c->n_slots = 1; c->use_closed = w_closed; c->act_sel = 0; c->act_cnt = 1;
      f.slot_node[0] = w_node; f.slot_pos[0] = w_pos; f.act_slot[0] = 0;
    } else c->round = 0;
  }
