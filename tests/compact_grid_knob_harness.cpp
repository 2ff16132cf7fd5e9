// Prints Knobs::compact_grid and Knobs::test_grid_pool as Knobs::from_env() reads them (tests/test_compact_grid_knob.py
// compiles this file together with space_filling_forest_star_amd/csrc/knobs.cpp using the host compiler alone).
#include <cstdio>

#include "knobs.h"

int main() {
  const sff::Knobs k = sff::Knobs::from_env();
  printf("compact_grid=%d test_grid_pool=%d\n", (int)k.compact_grid, k.test_grid_pool);
  return 0;
}
