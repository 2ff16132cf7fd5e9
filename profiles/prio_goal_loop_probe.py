"""A forest with both a goal and a priority bias in the loop of waves of one slot (SFFGPU_PRIO_GOAL_LOOP=1) against what such a
forest ran on before it, the host-replay engine: two jobs of tests/test_gpu_prio_goal_loop.py - `triang` (the scenario's
first 2 start points, goal = first start point + [57, -5, -20]) and `building` (1 start point, the far goal, + [88, 57, 92]),
priority bias 0.95, wave 1, ThresholdMisses 5, max_iterations 6 000, plain SFF - over seeds 1..64.

Legs (every repeat of every leg is a child process of its own under a time limit, legs alternated inside one command):
  a  ONE forest at a time created under the knob, Forest.run, seeds 1..N one after another (k_seq_waves<false, true, true>) - this build
  b  S.run_batch of B forests created under the knob, B contexts (k_seq_waves_batch<false, true, true>)                 - this build
  y  the yardstick: the same seeds one after another through Forest.run, no knob                            - the PARENT commit's build

The parent's build is a libsffgpu.so made from `git archive <parent>` in a directory outside git; --parent-lib names it (it
is loaded through SFFGPU_LIB; the knob is unknown there, so leg y is the host-replay engine).  Every seed that ran on both
sides must have the same fingerprint on both, or the command fails.  Contexts, mesh uploads and forest creation are outside
the timed region; every leg warms up on forests of other seeds; the clock is the host's, around calls that end in a
synchronisation.  Appends to profiles/prio_goal_loop_probe.jsonl.

  python profiles/prio_goal_loop_probe.py --parent-lib /path/to/parent/libsffgpu.so [--jobs triang,building] [--batch-sizes 8,32,64]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "prio_goal_loop_probe.jsonl")
JOBS = {"triang": dict(n_roots=2, offset=[57, -5, -20]), "building": dict(n_roots=1, offset=[88, 57, 92])}
ITERS = 6000
BIAS = 0.95


def child(a):
    import numpy as np
    import common
    import space_filling_forest_star_amd as S
    sc = common.scenario(a.job)
    n_ctx = a.B if a.leg == "b" else 1
    ctxs = []
    for _ in range(n_ctx):
        c = S.Context(0)
        c.upload_env(sc["env"])
        c.upload_robot(sc["robot"])
        ctxs.append(c)
    roots = sc["xml_points"][:JOBS[a.job]["n_roots"]]
    goal = roots[0].copy()
    goal[:3] += np.array(JOBS[a.job]["offset"], dtype=np.float64)

    def forest(ctx, seed):
        return S.Forest(ctx, roots, sc["limits"], dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=sc["dim"],
                        max_iterations=ITERS, wave=1, seed=seed, goal=goal, priority_bias=BIAS)

    stats, fps, on_device = [], [], []
    if a.leg == "b":
        warm = [forest(c, 1000 + i) for i, c in enumerate(ctxs)]
        S.run_batch(warm)
        for f in warm:
            f.close()
        fs = [forest(c, 1 + i) for i, c in enumerate(ctxs)]
        t = time.perf_counter()
        S.run_batch(fs)
        dt = time.perf_counter() - t
        stats = [f.stats() for f in fs]
        fps = [f.fingerprint() for f in fs]
        on_device = [f.device_engine() for f in fs]
    else:
        f = forest(ctxs[0], 1000)
        f.run()
        f.close()
        dt = 0.0
        for i in range(a.B):
            f = forest(ctxs[0], 1 + i)
            t = time.perf_counter()
            f.run()
            dt += time.perf_counter() - t
            stats.append(f.stats())
            fps.append(f.fingerprint())
            on_device.append(f.device_engine())
            f.close()
    # the loop: the device engine without a wave graph or a speculative step; the yardstick: not the device engine at all
    in_loop = all(d and s["graph_launches"] == 0 and s["spec_steps"] == 0 for d, s in zip(on_device, stats))
    assert in_loop == (a.leg != "y") and (a.leg != "y" or not any(on_device)), ("path taken", a.leg, on_device)
    its = sum(s["iterations"] for s in stats)
    print("RESULT " + json.dumps({
        "job": a.job, "leg": a.leg, "build": a.build, "B": a.B, "repeat": a.repeat, "seconds": dt, "iterations": its,
        "solved": sum(s["solved"] for s in stats), "iterations_per_s": its / dt, "forests_per_s": a.B / dt,
        "launches": max(s.get("batch_launches", 0) for s in stats),
        "host_fallback_waves": sum(s["host_fallback_waves"] for s in stats),
        "host_share": (sum(s["host_ms"] for s in stats) / max(1e-9, sum(s["total_ms"] for s in stats))),
        "fingerprints": ["%016x" % x for x in fps]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--job", default="triang")
    ap.add_argument("--leg", default="a")
    ap.add_argument("--build", default="new")
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=0)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--jobs", default="triang,building")
    ap.add_argument("--batch-sizes", default="8,32,64")
    ap.add_argument("--seeds", type=int, default=64, help="forests of the one-after-another legs (a and y)")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: a libsffgpu.so built from the parent commit (git archive <parent> | tar -x -C <dir>; make -C <dir>/space_filling_forest_star_amd/csrc)")
    sizes = [int(x) for x in a.batch_sizes.split(",") if x]
    legs = [("a", "new", a.seeds)] + [("b", "new", B) for B in sizes] + [("y", "parent", a.seeds)]
    for job in [j for j in a.jobs.split(",") if j]:
        by_seed = {}   # seed -> {side: fingerprint}
        for rep in range(a.repeats):
            for leg, build, B in legs:
                env = dict(os.environ)
                for k in ("SFFGPU_LIB", "SFFGPU_PRIO_GOAL_LOOP", "SFFGPU_GOAL_LOOP", "SFFGPU_PRIO_LOOP", "SFFGPU_ENGINE", "SFFGPU_SPEC", "SFFGPU_NO_SEQ",
                          "SFFGPU_PRIO_DEVICE"):
                    env.pop(k, None)
                if build == "parent":
                    env["SFFGPU_LIB"] = os.path.abspath(a.parent_lib)
                else:
                    env["SFFGPU_PRIO_GOAL_LOOP"] = "1"
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--job", job, "--leg", leg, "--build", build,
                       "--B", str(B), "--repeat", str(rep)]
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not lines:
                    print(p.stdout[-4000:])
                    sys.exit("%s, leg %s (%s, B = %d) ended with status %d: nothing more is started" % (job, leg, build, B, p.returncode))
                rec = json.loads(lines[0][7:])
                with open(a.out, "a") as fp:
                    fp.write(json.dumps(rec) + "\n")
                print("%-8s leg %s %-6s B %3d rep %d: %7.3f s  %9.0f it/s  %7.1f forests/s  solved %d  launches %d  host share %.3f  host waves %d" % (
                    job, leg, build, B, rep, rec["seconds"], rec["iterations_per_s"], rec["forests_per_s"], rec["solved"],
                    rec["launches"], rec["host_share"], rec["host_fallback_waves"]), flush=True)
                for i, fp_ in enumerate(rec["fingerprints"]):
                    sides = by_seed.setdefault(1 + i, {})
                    side = "parent" if build == "parent" else "new"
                    if sides.setdefault(side, fp_) != fp_ or len(set(sides.values())) > 1:
                        sys.exit("%s, seed %d: fingerprints differ (%s; leg %s gave %s)" % (job, 1 + i, sides, leg, fp_))
        both = [s for s, v in by_seed.items() if len(v) == 2]
        print("%s: fingerprints equal on both sides for %d seeds" % (job, len(both)))


if __name__ == "__main__":
    main()
