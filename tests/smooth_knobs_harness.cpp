// Prints Knobs::smooth_loop and Knobs::smooth_edges as Knobs::from_env() reads them (tests/test_smooth_knobs.py compiles this
// file together with space_filling_forest_star_amd/csrc/knobs.cpp using the host compiler alone).
#include <cstdio>

#include "knobs.h"

int main() {
  const sff::Knobs k = sff::Knobs::from_env();
  printf("smooth_loop=%d smooth_edges=%d\n", (int)k.smooth_loop, k.smooth_edges);
  return 0;
}
