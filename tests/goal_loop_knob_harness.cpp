// Prints Knobs::goal_loop as Knobs::from_env() reads it (tests/test_goal_loop_knob.py compiles this file together with
// space_filling_forest_star_amd/csrc/knobs.cpp using the host compiler alone).
#include <cstdio>

#include "knobs.h"

int main() {
  const sff::Knobs k = sff::Knobs::from_env();
  printf("goal_loop=%d\n", (int)k.goal_loop);
  return 0;
}
