"""bench.py's wave_sweep legs at waves of 64 and 512 slots on the library SFFGPU_LIB names, without the rest of
`bench.py --full`: the same scene (dense3d), the same 10 roots (seed 1, drawn with the GPU collision kernel as bench.py
does), the same forest arguments and iteration counts (150 000 / 1 000 000) as its small_wave_leg - the figures compare
with recorded wave_sweep legs.  One JSON line {"lib", "wave_64", "wave_512"} with iterations/s.  A warm-up forest per wave
size comes first (code object load, graph capture)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import common                                  # noqa: E402
import space_filling_forest_star_amd as S      # noqa: E402

sc = common.scenario("dense3d")
ctx = S.Context(0)
ctx.upload_env(sc["env"])
ctx.upload_robot(sc["robot"])
roots = common.free_roots(lambda p: int(ctx.collide_poses(p[None, :])[0]), sc["limits"], 10, seed=1)
out = {"lib": os.environ.get("SFFGPU_LIB", "libsffgpu.so")}
for wave, iters in ((64, 150000), (512, 1000000)):
    for n in (iters // 10, iters):
        f = S.Forest(ctx, roots, sc["limits"], dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=6,
                     max_iterations=n, node_budget=0, wave=wave, seed=1)
        t0 = time.perf_counter()
        f.run()
        dt = time.perf_counter() - t0
        st, dev = f.stats(), bool(f.device_engine())
        f.close()
    out["wave_%d" % wave] = {"iterations_per_s": st["iterations"] / dt, "iterations": st["iterations"], "nodes": st["n_nodes"],
                             "device_engine": dev, "seconds": dt}
print(json.dumps(out), flush=True)
