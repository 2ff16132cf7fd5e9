// Prints Knobs::paths_dev and Knobs::test_paths_cap as Knobs::from_env() reads them (tests/test_paths_knobs.py compiles this
// file together with space_filling_forest_star_amd/csrc/knobs.cpp using the host compiler alone).
#include <cstdio>

#include "knobs.h"

int main() {
  const sff::Knobs k = sff::Knobs::from_env();
  printf("paths_dev=%d test_paths_cap=%d\n", (int)k.paths_dev, k.test_paths_cap);
  return 0;
}
