"""The priority frontier in the loop of waves of one slot (SFFGPU_PRIO_LOOP=1) against what such a forest ran on before it,
the host-replay engine: wave-1 priority forests of the bench's job shape (dense_3D, 6-DoF, 10 roots, priorityBias 0.95, the
scenario's tree / sampling distances, ThresholdMisses 5, node_budget 20 000, seeds 1..B).

Legs (every repeat of every leg is a child process of its own under a time limit, legs alternated inside one command):
  a  ONE forest created under the knob, Forest.run (k_seq_waves<false, true>)                    - this build
  b  S.run_batch of B forests created under the knob, B contexts (k_seq_waves_batch<false, true>) - this build
  y  the yardstick: forests of the same seeds one after another through Forest.run, no knob      - the PARENT commit's build

The parent's build is a libsffgpu.so made from `git archive <parent>` in a directory outside git; --parent-lib names it (it
is loaded through SFFGPU_LIB; the knob is unknown there, so leg y is the host-replay engine).  The yardstick's rate does not
depend on how many forests it runs, and it runs them at ~10 s each: --seq-size bounds their number (default: the largest
B); every seed that ran on both sides must have the same fingerprint on both, or the command fails.
Contexts, mesh uploads and forest creation are outside the timed region; the knob legs warm up on forests of other seeds;
the clock is the host's, around calls that end in a synchronisation.  Appends to profiles/prio_loop_probe.jsonl.

  python profiles/prio_loop_probe.py --parent-lib /path/to/parent/libsffgpu.so [--batch-sizes 8,32,64] [--seq-size 64]
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
OUT = os.path.join(ROOT, "profiles", "prio_loop_probe.jsonl")
BIAS = 0.95


def child(a):
    import common
    import space_filling_forest_star_amd as S
    sc = common.scenario("dense3d")
    n_ctx = a.B if a.leg == "b" else 1
    ctxs = []
    for _ in range(n_ctx):
        c = S.Context(0)
        c.upload_env(sc["env"])
        c.upload_robot(sc["robot"])
        ctxs.append(c)
    roots = common.free_roots(lambda p: int(ctxs[0].collide_poses(p[None, :])[0]), sc["limits"], 10, seed=1)

    def forest(ctx, seed, budget):
        return S.Forest(ctx, roots, sc["limits"], dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=6,
                        max_iterations=2 ** 31 - 1, node_budget=budget, wave=1, seed=seed, priority_bias=BIAS)

    stats, fps, engines = [], [], []
    if a.leg == "b":
        warm = [forest(c, 1000 + i, 1500) for i, c in enumerate(ctxs)]
        S.run_batch(warm)
        for f in warm:
            f.close()
        fs = [forest(c, 1 + i, a.budget) for i, c in enumerate(ctxs)]
        engines = [f.device_engine() for f in fs]
        t = time.perf_counter()
        S.run_batch(fs)
        dt = time.perf_counter() - t
        stats = [f.stats() for f in fs]
        fps = [f.fingerprint() for f in fs]
    else:
        f = forest(ctxs[0], 1000, 1500)
        f.run()
        f.close()
        dt = 0.0
        for i in range(a.B):
            f = forest(ctxs[0], 1 + i, a.budget)
            engines.append(f.device_engine())
            t = time.perf_counter()
            f.run()
            dt += time.perf_counter() - t
            stats.append(f.stats())
            fps.append(f.fingerprint())
            f.close()
    want_device = a.leg != "y"
    assert all(bool(e) == want_device for e in engines), ("engine choice", a.leg, engines)
    its = sum(s["iterations"] for s in stats)
    nodes = sum(s["n_nodes"] - 10 for s in stats)
    print("RESULT " + json.dumps({
        "leg": a.leg, "build": a.build, "B": a.B, "repeat": a.repeat, "seconds": dt, "iterations": its, "nodes": nodes,
        "iterations_per_s": its / dt, "nodes_per_s": nodes / dt,
        "launches": max(s.get("batch_launches", 0) for s in stats), "spec_steps": sum(s["spec_steps"] for s in stats),
        "host_fallback_waves": sum(s["host_fallback_waves"] for s in stats),
        "host_share": (sum(s["host_ms"] for s in stats) / max(1e-9, sum(s["total_ms"] for s in stats))),
        "fingerprints": ["%016x" % x for x in fps]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", default="a")
    ap.add_argument("--build", default="new")
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=0)
    ap.add_argument("--budget", type=int, default=20000)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch-sizes", default="8,32,64")
    ap.add_argument("--seq-size", type=int, default=0, help="forests of the yardstick leg (0 = the largest batch size)")
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: a libsffgpu.so built from the parent commit (git archive <parent> | tar -x -C <dir>; make -C <dir>/space_filling_forest_star_amd/csrc)")
    sizes = [int(x) for x in a.batch_sizes.split(",") if x]
    n_seq = a.seq_size if a.seq_size > 0 else max(sizes + [1])
    legs = [("a", "new", 1)] + [("b", "new", B) for B in sizes] + [("y", "parent", n_seq)]
    by_seed = {}   # seed -> {side: fingerprint}
    for rep in range(a.repeats):
        for leg, build, B in legs:
            env = dict(os.environ)
            for k in ("SFFGPU_LIB", "SFFGPU_PRIO_LOOP", "SFFGPU_ENGINE", "SFFGPU_SPEC", "SFFGPU_NO_SEQ"):
                env.pop(k, None)
            if build == "parent":
                env["SFFGPU_LIB"] = os.path.abspath(a.parent_lib)
            else:
                env["SFFGPU_PRIO_LOOP"] = "1"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", leg, "--build", build, "--B", str(B),
                   "--repeat", str(rep), "--budget", str(a.budget)]
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                print(p.stdout[-4000:])
                sys.exit("leg %s (%s, B = %d) ended with status %d: nothing more is started" % (leg, build, B, p.returncode))
            rec = json.loads(lines[0][7:])
            with open(a.out, "a") as fp:
                fp.write(json.dumps(rec) + "\n")
            print("leg %s %-6s B %3d rep %d: %7.3f s  %9.0f it/s  %8.0f nodes/s  launches %d  host share %.3f  host waves %d" % (
                leg, build, B, rep, rec["seconds"], rec["iterations_per_s"], rec["nodes_per_s"], rec["launches"],
                rec["host_share"], rec["host_fallback_waves"]), flush=True)
            for i, fp_ in enumerate(rec["fingerprints"]):
                sides = by_seed.setdefault(1 + i, {})
                side = "parent" if build == "parent" else "new"
                if sides.setdefault(side, fp_) != fp_ or len(set(sides.values())) > 1:
                    sys.exit("seed %d: fingerprints differ (%s; leg %s gave %s)" % (1 + i, sides, leg, fp_))
    both = [s for s, v in by_seed.items() if len(v) == 2]
    print("fingerprints equal on both sides for %d seeds (of %d run under the knob)" % (len(both), len(by_seed)))


if __name__ == "__main__":
    main()
