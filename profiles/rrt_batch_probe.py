"""Session batches against what a user could do before them: B independent RRT / RRT* / Multi-T-RRT sessions of the
bench's job shape (dense_3D, 6-DoF, the scenario's tree / sampling distances, the iteration budget of the bench's RRT legs,
seeds 1..B; 1 root for RRT and RRT*, 10 roots for Multi-T-RRT; `lazy` / `lazy_star`: lazy edges - LazyTSP::runRRT, one root,
goal = the second of the job's free points, sessions created under SFFGPU_LAZY_BATCH=1 - which end when they reach the goal).

Legs (every repeat of every leg is a child process of its own, legs alternated inside one command):
  a  S.run_rrt_batch of the B sessions (B contexts)                                     - this build (--a-builds new,parent:
                                                                                          and the parent's, alternated)
  b  the B sessions one after another through Rrt.run with wave = 0 (speculative waves) - the PARENT commit's build

The parent's build is a libsffgpu.so made from `git archive <parent>` in a directory outside git; --parent-lib names it
(it is loaded through SFFGPU_LIB; its statistics struct is 16 bytes shorter, the two batch fields read 0 there).
Contexts, mesh uploads and session creation are outside the timed region; every child warms up on sessions of other
seeds; the clock is the host's, around calls that end in a synchronisation.  A session's result fingerprint is a hash of
its node arrays, links and reference-equivalent counters: all B of them must be equal on both sides.
Appends to profiles/rrt_batch_probe.jsonl.

  python profiles/rrt_batch_probe.py --parent-lib /path/to/parent/libsffgpu.so [--kinds rrt,star,multi] [--repeats 3]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "rrt_batch_probe.jsonl")
KINDS = {"rrt": (1, False, False), "star": (1, True, False), "multi": (10, False, False),   # roots, optimize, lazy_edge
         "lazy": (1, False, True), "lazy_star": (1, True, True)}
KEYS = ("iterations", "solved", "n_nodes", "n_live_trees", "merges", "n_links", "collide_calls", "path_free_calls", "nn_queries",
        "rng_draws")


def fingerprint(r):
    h = hashlib.sha256()
    st = r.stats()
    h.update(json.dumps([st[k] for k in KEYS]).encode())
    n, l = r.nodes(), r.links()
    for k in sorted(n):
        h.update(n[k].tobytes())
    for k in sorted(l):
        h.update(l[k].tobytes())
    if r.lazy_edge:
        h.update(json.dumps([st["lazy_distance"]]).encode())
        h.update(r.lazy_plan().tobytes())
    return h.hexdigest()[:16]


def child(a):
    import common
    import space_filling_forest_star_amd as S
    sc = common.scenario("dense3d")
    n_roots, optimize, lazy = KINDS[a.kind]
    n_ctx = a.B if a.leg == "a" else 1
    ctxs = []
    for _ in range(n_ctx):
        c = S.Context(0)
        c.upload_env(sc["env"])
        c.upload_robot(sc["robot"])
        ctxs.append(c)
    roots = common.free_roots(lambda p: int(ctxs[0].collide_poses(p[None, :])[0]), sc["limits"], 10, seed=1)
    goal = roots[1] if lazy else None
    roots = roots[:n_roots]

    def session(ctx, seed, iters):
        return S.Rrt(ctx, roots, sc["limits"], dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=6,
                     max_iterations=iters, wave=0, seed=seed, optimize=optimize, goal=goal, lazy_edge=lazy)

    stats, fps = [], []
    if a.leg == "a":
        warm = [session(c, 1000 + i, 2000) for i, c in enumerate(ctxs)]
        S.run_rrt_batch(warm)
        for r in warm:
            r.close()
        rs = [session(c, 1 + i, a.iters) for i, c in enumerate(ctxs)]
        t = time.perf_counter()
        S.run_rrt_batch(rs)
        dt = time.perf_counter() - t
        t = time.perf_counter()
        stats = [r.stats() for r in rs]          # (the first getter brings the host mirror up to date: part of the price)
        dt_sync = time.perf_counter() - t
        fps = [fingerprint(r) for r in rs]
    else:
        r = session(ctxs[0], 1000, 2000)
        r.run()
        r.close()
        dt, dt_sync = 0.0, 0.0
        for i in range(a.B):
            r = session(ctxs[0], 1 + i, a.iters)
            t = time.perf_counter()
            r.run()
            dt += time.perf_counter() - t
            stats.append(r.stats())
            fps.append(fingerprint(r))
            r.close()
    its = sum(s["iterations"] for s in stats)
    print("RESULT " + json.dumps({
        "leg": a.leg, "build": a.build, "kind": a.kind, "B": a.B, "repeat": a.repeat, "seconds": dt, "mirror_seconds": dt_sync,
        "iterations": its, "nodes": sum(s["n_nodes"] for s in stats), "solved": sum(s["solved"] for s in stats),
        "iterations_per_s": its / (dt + dt_sync),
        "launches": max(s.get("batch_launches", 0) for s in stats),
        "batch_host_iterations": sum(s.get("batch_host_iterations", 0) for s in stats), "merges": sum(s["merges"] for s in stats),
        "waves": sum(s["waves"] for s in stats), "fingerprints": fps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", default="a")
    ap.add_argument("--build", default="new")
    ap.add_argument("--kind", default="rrt")
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=0)
    ap.add_argument("--iters", type=int, default=150000)   # bench.py's RRT legs
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--kinds", default="rrt,star,multi")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch-sizes", default="1,8,32,64")
    ap.add_argument("--seq-sizes", default="")             # leg b; default: the batch sizes (the same B sessions on both sides)
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--a-builds", default="new")           # leg a; "new,parent": the parent's run_rrt_batch too (a parent that has one)
    ap.add_argument("--child-timeout", type=int, default=900)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: a libsffgpu.so built from the parent commit (git archive <parent> | tar -x -C <dir>; make -C <dir>/space_filling_forest_star_amd/csrc)")
    sizes_a = [int(x) for x in a.batch_sizes.split(",")]
    sizes_b = [int(x) for x in a.seq_sizes.split(",")] if a.seq_sizes else sizes_a
    for kind in a.kinds.split(","):
        legs = []
        for B in sorted(set(sizes_a) | set(sizes_b)):      # legs alternated: batch, yardstick, batch, ...
            legs += [("a", build, B) for build in a.a_builds.split(",")] if B in sizes_a else []
            legs += [("b", "parent", B)] if B in sizes_b else []
        legs = [l for l in legs if l[0] in a.legs.split(",")]
        seen = {}
        for rep in range(a.repeats):
            for leg, build, B in legs:
                env = dict(os.environ)
                env.pop("SFFGPU_LIB", None)
                env.pop("SFFGPU_LAZY_BATCH", None)
                if KINDS[kind][2]:
                    env["SFFGPU_LAZY_BATCH"] = "1"      # (read when a session is created; a build from before the knob ignores it)
                if build == "parent":
                    env["SFFGPU_LIB"] = os.path.abspath(a.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", leg, "--build", build, "--kind", kind, "--B", str(B),
                       "--repeat", str(rep), "--iters", str(a.iters)]
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not lines:
                    print(p.stdout[-4000:])
                    sys.exit("leg %s (%s, %s, B = %d) ended with status %d: nothing more is started" % (leg, build, kind, B, p.returncode))
                rec = json.loads(lines[0][7:])
                # the same seeds on both sides: member i's fingerprint is the same in every leg and every repeat
                for i, fp in enumerate(rec["fingerprints"]):
                    if seen.setdefault(i, fp) != fp:
                        sys.exit("leg %s (%s, %s, B = %d): member %d differs from the other legs" % (leg, build, kind, B, i))
                rec["fingerprints_equal"] = True
                with open(a.out, "a") as fp:
                    fp.write(json.dumps(rec) + "\n")
                print("%-5s leg %s %-6s B %3d rep %d: %8.3f s (+ %.3f s mirror)  %9.0f it/s  launches %d  host iterations %d  merges %d" % (
                    kind, leg, build, B, rep, rec["seconds"], rec["mirror_seconds"], rec["iterations_per_s"], rec["launches"],
                    rec["batch_host_iterations"], rec["merges"]), flush=True)


if __name__ == "__main__":
    main()
