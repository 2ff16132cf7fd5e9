"""Path smoothing on the device against what a user could do before it: B planners with their paths extracted, smoothed

  a  together by S.smooth_batch / S.smooth_rrt_batch (k_smooth_paths, one wavefront per path)      - this build
  b  one after another by sffgpu_forest_smooth_paths / sffgpu_rrt_smooth_paths (Forest.smooth)      - the PARENT commit's build

Forests: dense3d_coarse, 6-DoF, 10 seeded roots, wave 1, run until the frontier is empty (the trees meet: the probe asserts
that every member has paths), seeds 1..B, B = 1, 8, 64.  Sessions: 64 Multi-T-RRT sessions on triang (4 XML roots, 1 500
iterations, seeds 1..64).  Every member lives on a context of its own in both legs.

Every repeat of every leg is a child process of its own, legs alternated.  A child grows its planners, extracts their paths,
smooths once untimed (warm-up: code objects, buffers), calls paths() again - which restores the raw plans - and smooths
timed: the host's clock around calls that end in a synchronisation.  Matrices and plans are fingerprinted; the two legs of a
size must agree.  The parent's build is a libsffgpu.so made from `git archive <parent>`, loaded through SFFGPU_LIB
(--parent-lib, a path relative to the package directory or absolute).  Appends to profiles/smooth_probe.jsonl: one record
per child and, per size, a summary with the medians, leg b's spread and whether the slowest a beat the fastest b.

  python profiles/smooth_probe.py --parent-lib /path/to/parent/libsffgpu.so [--sizes 1,8,64] [--repeats 3]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "smooth_probe.jsonl")


def child(a):
    import numpy as np
    import common
    import space_filling_forest_star_amd as S
    forest = a.kind == "forest"
    sc = common.scenario("dense3d_coarse" if forest else "triang")
    ctxs = []
    for _ in range(a.B):
        c = S.Context(0)
        c.upload_env(sc["env"])
        c.upload_robot(sc["robot"])
        ctxs.append(c)
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=6)
    if forest:
        roots = common.free_roots(lambda p: int(ctxs[0].collide_poses(p[None, :])[0]), sc["limits"], 10, seed=1)
        ps = [S.Forest(c, roots, sc["limits"], max_iterations=2 ** 31 - 1, wave=1, seed=1 + i, **kw) for i, c in enumerate(ctxs)]
        S.run_batch(ps)
        extract = lambda: [p.paths()[0] for p in ps]
    else:
        roots = sc["xml_points"][:4]
        ps = [S.Rrt(c, roots, sc["limits"], max_iterations=1500, seed=1 + i, wave=0, **kw) for i, c in enumerate(ctxs)]
        for p in ps:
            p.run()
        extract = lambda: [p.paths(4)[0] for p in ps]

    def smooth():
        if a.leg == "a":
            return S.smooth_batch(ps) if forest else S.smooth_rrt_batch(ps)
        return [p.smooth() for p in ps]

    raw = extract()
    if forest:
        for i, d in enumerate(raw):
            off = d[~np.eye(len(d), dtype=bool)]
            assert np.any(off < 1e300), "member %d has no path" % i
    smooth()                                  # warm-up
    extract()                                 # the raw plans again
    pf0 = sum(p.stats()["path_free_calls"] for p in ps)
    t = time.perf_counter()
    res = smooth()
    dt = time.perf_counter() - t
    edges = sum(p.stats()["path_free_calls"] for p in ps) - pf0
    h = hashlib.sha256()
    n_paths = 0
    for p, r in zip(ps, res):
        if forest:
            h.update(np.ascontiguousarray(r).tobytes())
            for i in range(len(r)):
                for j in range(i + 1, len(r)):
                    plan = p.plan(i, j)
                    n_paths += int(len(plan) > 0)
                    h.update(np.ascontiguousarray(plan).tobytes())
        else:
            n_paths += len(r)
            for plan in r:
                h.update(np.ascontiguousarray(plan).tobytes())
    rec = {"kind": a.kind, "leg": a.leg, "build": a.build, "B": a.B, "repeat": a.repeat, "seconds": dt, "paths": n_paths,
           "edges": edges, "nodes": sum(p.stats()["n_nodes"] for p in ps), "fingerprint": h.hexdigest()[:16]}
    if a.leg == "a":
        sm = [p.smooth_stats() for p in ps]
        rec["launches_timed"] = max(s["launches"] for s in sm) // 2      # (warm-up and timed call launch alike)
        rec["host_edges"] = sum(s["host_edges"] for s in sm)
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", default="forest")
    ap.add_argument("--leg", default="a")
    ap.add_argument("--build", default="new")
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=0)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--sizes", default="1,8,64")
    ap.add_argument("--rrt-sizes", default="64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    pkg = os.path.join(ROOT, "space_filling_forest_star_amd")
    if not a.parent_lib or not os.path.exists(os.path.join(pkg, a.parent_lib)):
        sys.exit("--parent-lib: a libsffgpu.so built from the parent commit (git archive <parent> | tar -x -C <dir>; make -C <dir>/space_filling_forest_star_amd/csrc)")
    jobs = [("forest", int(x)) for x in a.sizes.split(",") if x] + [("rrt", int(x)) for x in a.rrt_sizes.split(",") if x]
    for kind, B in jobs:
        recs = {"a": [], "b": []}
        for rep in range(a.repeats):
            for leg, build in (("a", "new"), ("b", "parent")):
                env = dict(os.environ)
                env.pop("SFFGPU_LIB", None)
                for k in ("SFFGPU_SMOOTH_LOOP", "SFFGPU_SMOOTH_EDGES"):
                    env.pop(k, None)
                if build == "parent":
                    env["SFFGPU_LIB"] = a.parent_lib
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--kind", kind, "--leg", leg, "--build", build, "--B", str(B),
                       "--repeat", str(rep)]
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not lines:
                    print(p.stdout[-4000:])
                    sys.exit("%s leg %s (B = %d) ended with status %d: nothing more is started" % (kind, leg, B, p.returncode))
                rec = json.loads(lines[0][7:])
                recs[leg].append(rec)
                with open(a.out, "a") as fp:
                    fp.write(json.dumps(rec) + "\n")
                print("%-6s leg %s %-6s B %3d rep %d: %9.3f ms  %5d paths %7d edges  %s" % (
                    kind, leg, build, B, rep, 1e3 * rec["seconds"], rec["paths"], rec["edges"], rec["fingerprint"]), flush=True)
        fps = {r["fingerprint"] for leg in recs for r in recs[leg]}
        ta, tb = [r["seconds"] for r in recs["a"]], [r["seconds"] for r in recs["b"]]
        summary = {"summary": kind, "B": B, "a_median_ms": 1e3 * statistics.median(ta), "a_min_ms": 1e3 * min(ta), "a_max_ms": 1e3 * max(ta),
                   "b_median_ms": 1e3 * statistics.median(tb), "b_min_ms": 1e3 * min(tb), "b_max_ms": 1e3 * max(tb),
                   "speedup_of_medians": statistics.median(tb) / statistics.median(ta), "slowest_a_beats_fastest_b": max(ta) < min(tb),
                   "paths": recs["a"][0]["paths"], "edges": recs["a"][0]["edges"], "launches": recs["a"][0].get("launches_timed"),
                   "results_equal": len(fps) == 1}
        with open(a.out, "a") as fp:
            fp.write(json.dumps(summary) + "\n")
        print("SUMMARY " + json.dumps(summary), flush=True)
        if len(fps) != 1:
            sys.exit("%s B = %d: the two legs disagree: %s" % (kind, B, sorted(fps)))


if __name__ == "__main__":
    main()
