"""Forest batches against what a user could do before them: B independent wave-1 forests of the bench's job shape
(dense_3D, 6-DoF, 10 roots, the scenario's tree / sampling distances, ThresholdMisses 5, node_budget 20 000, seeds 1..B).

Legs (every repeat of every leg is a child process of its own, legs alternated inside one command):
  a  S.run_batch of the B forests (B contexts)                                         - this build (--a-builds new,parent:
                                                                                          and the parent's, alternated)
  b  the B forests one after another through Forest.run (k_spec_waves)                 - the PARENT commit's build
                                                                                          (--b-builds new,parent: and this one)
  c  as b with SFFGPU_SPEC=0 (the single wavefront: a batch of one on this build)       - the parent's build AND this one

The parent's build is a libsffgpu.so made from `git archive <parent>` in a directory outside git; --parent-lib names it
(it is loaded through SFFGPU_LIB; its statistics struct is 8 bytes shorter, batch_launches reads 0 there).
Contexts, mesh uploads and forest creation are outside the timed region; every child warms up on forests of other
seeds; the clock is the host's, around calls that end in a synchronisation.  Appends to profiles/batch_probe.jsonl.

  python profiles/batch_probe.py --parent-lib /path/to/parent/libsffgpu.so [--kinds sff,star] [--repeats 3]
  python profiles/batch_probe.py --parent-lib ... --legs a --a-builds new,parent --batch-sizes 64    (one build against another)
  python profiles/batch_probe.py --parent-lib ... --legs a --a-builds new,parent --batch-sizes 64,128 --share-env
      (member contexts: on THIS build context 0 uploads and the others are made with sffgpu_create_member; a parent build,
       which has no such entry point, sets every context up in full as before)

  python profiles/batch_probe.py --parent-lib ... --legs a --a-builds new,compact --batch-sizes 64,128,256 --share-env
      (the compact node grid: build "compact" is this build with its members created under SFFGPU_COMPACT_GRID=1, alternated
       with the dense members of "new"; --compact makes the members of "new" compact too)

Every record of leg a also carries the set-up: setup_seconds = the wall time of the contexts (first sffgpu_create to the
last context ready) + that of creating the measured forests, and - a build that has sffgpu_ctx_get_memory - memory_member_1,
Context.memory() of member 1 after the run.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "batch_probe.jsonl")


def free_bytes():
    hip = C.CDLL("libamdhip64.so")
    fr, tot = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
    return fr.value


def child(a):
    import common
    import space_filling_forest_star_amd as S
    sc = common.scenario("dense3d")
    n_ctx = a.B if a.leg == "a" else 1
    t_setup = time.perf_counter()
    ctx0 = S.Context(0)
    ctx0.upload_env(sc["env"])
    ctx0.upload_robot(sc["robot"])
    setup_ctx = time.perf_counter() - t_setup
    roots = common.free_roots(lambda p: int(ctx0.collide_poses(p[None, :])[0]), sc["limits"], 10, seed=1)
    mem0 = free_bytes()
    ctxs = [ctx0]
    t_setup = time.perf_counter()
    for _ in range(n_ctx - 1):
        if a.share_env:
            if a.compact:   # (sffgpu_create_member reads the knob, and nothing after it does)
                os.environ["SFFGPU_COMPACT_GRID"] = "1"
            c = ctx0.member()
            os.environ.pop("SFFGPU_COMPACT_GRID", None)
        else:
            c = S.Context(0)
            c.upload_env(sc["env"])
            c.upload_robot(sc["robot"])
        ctxs.append(c)
    setup_ctx += time.perf_counter() - t_setup

    def forest(ctx, seed, budget):
        return S.Forest(ctx, roots, sc["limits"], dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=6,
                        max_iterations=2 ** 31 - 1, node_budget=budget, wave=1, seed=seed, optimize=bool(a.optimize))

    stats, fps = [], []
    setup_forests = None
    if a.leg == "a":
        warm = [forest(c, 1000 + i, 1500) for i, c in enumerate(ctxs)]
        S.run_batch(warm)
        for f in warm:
            f.close()
        t = time.perf_counter()
        fs = [forest(c, 1 + i, a.budget) for i, c in enumerate(ctxs)]
        setup_forests = time.perf_counter() - t
        t = time.perf_counter()
        S.run_batch(fs)
        dt = time.perf_counter() - t
        stats = [f.stats() for f in fs]
        fps = [f.fingerprint() for f in fs]
        mem1 = free_bytes()
    else:
        f = forest(ctx0, 1000, 1500)
        f.run()
        f.close()
        dt = 0.0
        for i in range(a.B):
            f = forest(ctx0, 1 + i, a.budget)
            t = time.perf_counter()
            f.run()
            dt += time.perf_counter() - t
            stats.append(f.stats())
            fps.append(f.fingerprint())
            f.close()
        mem1 = free_bytes()
    its = sum(s["iterations"] for s in stats)
    nodes = sum(s["n_nodes"] - 10 for s in stats)
    print("RESULT " + json.dumps({
        "leg": a.leg, "build": a.build, "kind": "SFF*" if a.optimize else "SFF", "B": a.B, "repeat": a.repeat, "seconds": dt,
        "iterations": its, "nodes": nodes, "iterations_per_s": its / dt, "nodes_per_s": nodes / dt,
        "launches": max(s["batch_launches"] for s in stats), "spec_steps": sum(s["spec_steps"] for s in stats),
        "host_share": (sum(s["host_ms"] for s in stats) / max(1e-9, sum(s["total_ms"] for s in stats))),
        "device_bytes_per_member": (mem0 - mem1) / max(1, n_ctx - 1) if n_ctx > 1 else None,
        "device_bytes_first_member_forest": (mem0 - mem1) if n_ctx == 1 else None,
        "share_env": bool(a.share_env), "setup_contexts_seconds": setup_ctx, "setup_forests_seconds": setup_forests,
        "setup_seconds": None if setup_forests is None else setup_ctx + setup_forests,
        "memory_member_1": ctxs[1].memory() if n_ctx > 1 and hasattr(S.lib(), "sffgpu_ctx_get_memory") else None,
        "compact": bool(a.compact), "grid_rebuilds": sum(s["grid_rebuilds"] for s in stats),
        "members_still_compact": (sum(c.grid_compact() for c in ctxs[1:]) if a.compact else None),
        "fingerprints": ["%016x" % x for x in fps]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", default="a")
    ap.add_argument("--build", default="new")
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--optimize", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=0)
    ap.add_argument("--budget", type=int, default=20000)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--kinds", default="sff,star")
    ap.add_argument("--repeats", type=int, default=3)
    # leg a; default 1,8,32,64,128 (SFF) / 1,32,64 (SFF*).  A member of this job takes ~1.4 GB of device memory (the node grid
    # over the dense_3D limits and the round engine's second grid, which Ctx::grid_setup allocates with it): 256 do not fit
    ap.add_argument("--batch-sizes", default="")
    ap.add_argument("--seq-sizes", default="")        # leg b; default 1,8,64 (SFF) / 1,64 (SFF*): the rate does not depend on B
    ap.add_argument("--c-size", type=int, default=8)  # leg c
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--a-builds", default="new")      # leg a; "new,parent": the parent's run_batch too (a parent that has one)
    ap.add_argument("--b-builds", default="parent")   # leg b; "new,parent": this build's Forest.run too, alternated
    ap.add_argument("--share-env", action="store_true")   # leg a, this build: contexts 1.. are members of context 0
    ap.add_argument("--compact", action="store_true")     # with --share-env: the members are created under SFFGPU_COMPACT_GRID=1
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: a libsffgpu.so built from the parent commit (git archive <parent> | tar -x -C <dir>; make -C <dir>/space_filling_forest_star_amd/csrc)")
    for kind in a.kinds.split(","):
        opt = 1 if kind == "star" else 0
        sizes_a = [int(x) for x in a.batch_sizes.split(",")] if a.batch_sizes else ([1, 32, 64] if opt else [1, 8, 32, 64, 128])
        sizes_b = [int(x) for x in a.seq_sizes.split(",")] if a.seq_sizes else ([1, 64] if opt else [1, 8, 64])
        legs = [("a", build, B) for B in sizes_a for build in a.a_builds.split(",")] + \
               [("b", build, B) for B in sizes_b for build in a.b_builds.split(",")]
        if a.c_size > 0:
            legs += [("c", "parent", a.c_size), ("c", "new", a.c_size)]
        legs = [l for l in legs if l[0] in a.legs.split(",")]
        for rep in range(a.repeats):
            for leg, build, B in legs:
                env = dict(os.environ)
                env.pop("SFFGPU_LIB", None)
                env.pop("SFFGPU_SPEC", None)
                env.pop("SFFGPU_COMPACT_GRID", None)
                if build == "parent":
                    env["SFFGPU_LIB"] = os.path.abspath(a.parent_lib)
                if leg == "c":
                    env["SFFGPU_SPEC"] = "0"
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", leg, "--build", build, "--B", str(B),
                       "--optimize", str(opt), "--repeat", str(rep), "--budget", str(a.budget)]
                if a.share_env and leg == "a" and build in ("new", "compact"):
                    cmd.append("--share-env")
                    if a.compact or build == "compact":
                        cmd.append("--compact")
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not lines:
                    print(p.stdout[-4000:])
                    sys.exit("leg %s (%s, B = %d) ended with status %d: nothing more is started" % (leg, build, B, p.returncode))
                rec = json.loads(lines[0][7:])
                with open(a.out, "a") as fp:
                    fp.write(json.dumps(rec) + "\n")
                print("%-4s leg %s %-6s B %3d rep %d: %7.3f s  %9.0f it/s  %8.0f nodes/s  launches %d  host share %.3f" % (
                    rec["kind"], leg, build, B, rep, rec["seconds"], rec["iterations_per_s"], rec["nodes_per_s"], rec["launches"],
                    rec["host_share"]), flush=True)
                if leg == "a" and B > 1:
                    print("     set-up %.2f s (contexts %.2f, forests %.2f)  device memory per member %.3f GB%s" % (
                        rec["setup_seconds"], rec["setup_contexts_seconds"], rec["setup_forests_seconds"],
                        rec["device_bytes_per_member"] / 1e9, "  (members of context 0)" if rec["share_env"] else ""), flush=True)


if __name__ == "__main__":
    main()
