// paths_rules.h — the two decision rules of post-loop path extraction, written once for the host and the gfx950 kernel
// (devpaths.hip): plain IEEE-754 double arithmetic in a fixed order (sff_geom.h; build with -ffp-contract=off).
//
//   border pick   SpaceForest::getPaths (src/forest.h:420-462; Forest::get_paths in paths.cpp): the borders of a pair of trees
//                 are taken in list order; the first is taken, a later one only if it is smaller by MORE than the tolerance.
//                 Not an argmin: of two borders 6e-10 apart the first stays.
//   join          Solver::getAllPaths (src/problemStruct.h:184-253; Forest::get_all_paths): the paths tree1 -> tree3 and
//                 tree2 -> tree3 are oriented to END in tree3, their shared tail is stripped, the last shared node joins
//                 what is left of the first with what is left of the second reversed, the cost is the sum of dist6 over the
//                 joined plan from left to right (the order of the additions is part of the result), and the join replaces
//                 the pair's row only if it is shorter by MORE than the tolerance; the lower node id is stored first.
#pragma once
#include "sff_geom.h"

namespace sffr {

// ---- border pick.  best = -1: no border of the pair has been taken yet (costs are >= 0)
SFF_HD bool border_takes(double best, double dist) { return best == -1 || dist < best - SFFG_TOL; }
// DistanceHolder::UpdateDistance (src/primitives.h:652-654), in this association
SFF_HD double border_dist(double d_root1, double d_root2, const double* pos1, const double* pos2) {
  return d_root1 + d_root2 + sffg::dist6(pos1, pos2);
}

// ---- join.  A stored plan read in either direction
struct PlanView {
  const int32_t* ids;
  int len;
  bool fwd;        // false: read from the back (std::reverse of the copy)
  SFF_HD int at(int q) const { return ids[fwd ? q : len - 1 - q]; }
};
struct Join {
  int shared;      // entries of the shared tail (0: the plans do not end in the same node - no join)
  int keep1, keep2;// entries left of each plan
  int last;        // the last node stripped (first of the shared tail)
  int len;         // entries of the joined plan: keep1 + 1 + keep2
  double dist;     // its cost
};
// entry q of the joined plan: plan1's rest, the joint, plan2's rest reversed
SFF_HD int join_at(const PlanView& p1, const PlanView& p2, const Join& j, int q) {
  if (q < j.keep1) return p1.at(q);
  if (q == j.keep1) return j.last;
  return p2.at(j.keep2 - 1 - (q - j.keep1 - 1));
}
// pos(node) -> const double* of its six coordinates.  False: nothing shared (a forest's plans towards one tree all end in
// that tree's root, so this does not happen there; the reference would read node -1)
template <class Pos>
SFF_HD bool join_plans(const PlanView& p1, const PlanView& p2, Pos pos, Join& j) {
  int s = 0;
  while (s < p1.len && s < p2.len && p1.at(p1.len - 1 - s) == p2.at(p2.len - 1 - s)) ++s;
  j.shared = s;
  if (s == 0) return false;
  j.keep1 = p1.len - s;
  j.keep2 = p2.len - s;
  j.last = p1.at(p1.len - s);
  j.len = j.keep1 + 1 + j.keep2;
  double d = 0;                                   // Solver::computeDistance (:170-181)
  int prev = join_at(p1, p2, j, 0);
  for (int q = 1; q < j.len; ++q) {
    const int cur = join_at(p1, p2, j, q);
    d += sffg::dist6(pos(prev), pos(cur));
    prev = cur;
  }
  j.dist = d;
  return true;
}
SFF_HD bool join_accepts(double dist, double current) { return dist < current - SFFG_TOL; }   // :244-246
// stored lower node id first: true = the joined plan as it is (node1 is its first tree's border node), false = reversed
SFF_HD bool join_stored_forward(int node1, int node2) { return node1 < node2; }

}  // namespace sffr
