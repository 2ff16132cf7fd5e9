// The two decision rules of path extraction (space_filling_forest_star_amd/csrc/paths_rules.h) under the host compiler, on
// synthetic inputs: prints one line per case, tests/test_paths_rules.py compares them.  Stand-alone (its own main, no HIP): it
// may also be built with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <vector>

#include "paths_rules.h"

namespace {

// nodes on the x axis: node i at x = i, except what a case moves
std::vector<double> g_pos;
const double* pos_of(int node) { return g_pos.data() + 6 * (size_t)node; }
void line_world(int n) {
  g_pos.assign((size_t)n * 6, 0.0);
  for (int i = 0; i < n; ++i) g_pos[6 * (size_t)i] = (double)i;
}

// the pick among borders in list order: index of the one that stays
int pick(const std::vector<double>& d) {
  double best = -1;
  int at = -1;
  for (size_t i = 0; i < d.size(); ++i)
    if (sffr::border_takes(best, d[i])) { best = d[i]; at = (int)i; }
  return at;
}

void print_join(const char* name, const std::vector<int>& a, bool fa, const std::vector<int>& b, bool fb, double current) {
  const sffr::PlanView p1{a.data(), (int)a.size(), fa}, p2{b.data(), (int)b.size(), fb};
  sffr::Join j;
  if (!sffr::join_plans(p1, p2, pos_of, j)) {
    printf("%s shared=%d none\n", name, j.shared);
    return;
  }
  printf("%s shared=%d last=%d len=%d dist=%.17g accept=%d plan=", name, j.shared, j.last, j.len, j.dist,
         (int)sffr::join_accepts(j.dist, current));
  for (int q = 0; q < j.len; ++q) printf("%s%d", q ? "," : "", sffr::join_at(p1, p2, j, q));
  printf("\n");
}

}  // namespace

int main() {
  // ---- border pick
  printf("pick2=%d\n", pick({1.0, 1.0 - 6e-10}));
  printf("pick3=%d\n", pick({1.0, 1.0 - 6e-10, 1.0 - 1.5e-9}));
  printf("pick_first_zero=%d\n", pick({0.0, 0.0}));
  printf("pick_exact_tol=%d\n", pick({2.0, 2.0 - 1e-9}));          // (2 - 1e-9 is not below 2 - 1e-9)
  {
    const double a[6] = {0, 0, 0, 0, 0, 0}, b[6] = {1, 0, 0, 0, 0, 0};
    printf("border_dist=%.17g\n", sffr::border_dist(9007199254740992.0, 1.0, a, b));   // (2^53 + 1) + 1, in this association
  }
  // ---- joins.  Both plans end in tree 3's root (node 9)
  line_world(16);
  print_join("tail0", {0, 1, 2}, true, {5, 6, 7}, true, 1e300);
  print_join("tail1", {0, 1, 9}, true, {5, 6, 9}, true, 1e300);
  print_join("tail3", {0, 1, 7, 8, 9}, true, {5, 6, 7, 8, 9}, true, 1e300);
  // the same two paths stored the other way round (lower node id first: the plan starts in tree 3)
  print_join("tail3_rev1", {9, 8, 7, 1, 0}, false, {5, 6, 7, 8, 9}, true, 1e300);
  print_join("tail3_rev2", {0, 1, 7, 8, 9}, true, {9, 8, 7, 6, 5}, false, 1e300);
  print_join("tail3_rev12", {9, 8, 7, 1, 0}, false, {9, 8, 7, 6, 5}, false, 1e300);
  // one plan is the other's tail: nothing is left of it but the joint
  print_join("whole", {7, 8, 9}, true, {5, 6, 7, 8, 9}, true, 1e300);
  // acceptance: the join 0,1,9,6,5 costs 1 + 8 + 3 + 1 = 13
  print_join("shorter_by_less", {0, 1, 9}, true, {5, 6, 9}, true, 13.0 + 5e-10);
  print_join("shorter_by_more", {0, 1, 9}, true, {5, 6, 9}, true, 13.0 + 2e-9);
  print_join("equal", {0, 1, 9}, true, {5, 6, 9}, true, 13.0);
  // the sum runs left to right: 2^53 + 1 + 1 loses both ones, 1 + 1 + 2^53 keeps them.  Node 1 far out on x, nodes 2 and 3
  // one and two steps beside it on y
  line_world(16);
  const double far = 9007199254740992.0;
  g_pos[6 * 1] = far;
  g_pos[6 * 2] = far; g_pos[6 * 2 + 1] = 1.0;
  g_pos[6 * 3] = far; g_pos[6 * 3 + 1] = 2.0;
  print_join("order_long_first", {0, 1, 2}, true, {3, 2}, true, 1e300);      // 0 -> 1 -> 2 -> 3: 2^53, 1, 1
  print_join("order_long_last", {3, 2}, true, {0, 1, 2}, true, 1e300);       // 3 -> 2 -> 1 -> 0: 1, 1, 2^53
  printf("stored_forward=%d%d%d\n", (int)sffr::join_stored_forward(3, 7), (int)sffr::join_stored_forward(7, 3),
         (int)sffr::join_stored_forward(4, 4));
  return 0;
}
