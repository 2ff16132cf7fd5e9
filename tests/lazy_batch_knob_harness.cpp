// Prints Knobs::lazy_batch as Knobs::from_env() reads it (tests/test_lazy_batch_knob.py compiles this file together with
// space_filling_forest_star_amd/csrc/knobs.cpp using the host compiler alone).
#include <cstdio>

#include "knobs.h"

int main() {
  const sff::Knobs k = sff::Knobs::from_env();
  printf("lazy_batch=%d\n", (int)k.lazy_batch);
  return 0;
}
