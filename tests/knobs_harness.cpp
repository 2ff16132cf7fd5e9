// Prints Knobs::from_env() as `field=value` lines (tests/test_knobs.py compiles this file together with
// space_filling_forest_star_amd/csrc/knobs.cpp using the host compiler alone: no HIP in either).
#include <cstdio>

#include "knobs.h"

int main() {
  const sff::Knobs k = sff::Knobs::from_env();
#define I(f) printf(#f "=%d\n", (int)k.f)
#define D(f) printf(#f "=%.17g\n", k.f)
  I(timer_stride); I(profile); I(no_cand); I(no_clearance); D(clear_cells); D(clear_hdiv); I(no_trigrid); D(tg_div);
  I(test_grid_bk); I(test_grid_bkmax); I(test_grid_ovf);
  I(query); I(share); I(seg_blocks); I(cull_blocks); I(seg_listcap); I(star_knn);
  I(engine); I(prio_device); I(prio_seq); I(no_order); I(order_min_wave); I(test_hitcap); I(test_nbcap); I(test_star_passes);
  I(test_exchange_self); I(star_tail); I(star_tail_wgs); I(test_star_stall); I(test_star_items); I(test_border_cap);
  I(no_graph); I(profiler_preloaded); I(no_wave_ahead); I(no_fused_sample); I(no_zc_status); I(fallback_whole_wave);
  I(kc_trace); I(digest); I(no_seq); I(spec); I(spec_depth); I(spec_sets); I(spec_pipe); I(test_spec_stall); I(no_dev_trig);
  printf("seq_trace=%s\n", k.seq_trace.c_str());
  I(rrt_chain); I(rrt_fork); I(rrt_repair); I(rrt_dry); I(rrt_one_chain); I(rrt_split); I(rrt_small); I(rrt_grow);
  I(rrt_no_grid); I(rrt_no_chain_conn);
  return 0;
}
