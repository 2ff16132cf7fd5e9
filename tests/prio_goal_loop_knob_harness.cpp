// Prints Knobs::prio_goal_loop as Knobs::from_env() reads it (tests/test_prio_goal_loop_knob.py compiles this file together
// with space_filling_forest_star_amd/csrc/knobs.cpp using the host compiler alone).
#include <cstdio>

#include "knobs.h"

int main() {
  const sff::Knobs k = sff::Knobs::from_env();
  printf("prio_goal_loop=%d prio_loop=%d goal_loop=%d\n", (int)k.prio_goal_loop, (int)k.prio_loop, (int)k.goal_loop);
  return 0;
}
