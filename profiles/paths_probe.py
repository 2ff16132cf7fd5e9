"""Path extraction for forests together against what a user could do before it: B freshly grown forests, never downloaded,

  a  extracted together by S.paths_batch (k_paths_batch, one workgroup per forest)                 - this build
  b  one after another by sffgpu_forest_paths (Forest.paths: sync_host, then the host's walk)      - the PARENT commit's build

Forests: smooth_probe.py's - dense3d_coarse, 6-DoF, 10 seeded roots, wave 1, grown by run_batch until the frontier is empty,
seeds 1..B.  B = 1, 8, 64 on dense contexts of their own, and 256 compact members (context 0 uploads, the others are made by
sffgpu_create_member under SFFGPU_COMPACT_GRID=1), in both legs.

Every repeat of every leg is a child process of its own, legs alternated.  A child first grows ONE extra forest (seed 1000)
and extracts its paths the leg's way, untimed (code objects, the call's buffers), then grows the B members and times the
extraction: the host's clock around calls that end in a synchronisation.  So every timed forest is freshly grown and has
never been downloaded.  Matrices, connected sets and plans are fingerprinted; the two legs of a size must agree.  `--e2e B`
adds one line per leg for run_batch + paths + smooth_batch as a whole.  The parent's build is a libsffgpu.so made from
`git archive <parent>`, loaded through SFFGPU_LIB (--parent-lib).  Appends to profiles/paths_probe.jsonl: one record per
child and, per size, a summary with the medians, both spreads, the bytes each leg copies down and whether the slowest a beat
the fastest b.

  python profiles/paths_probe.py --parent-lib /path/to/parent/libsffgpu.so [--sizes 1,8,64] [--compact-sizes 256] [--e2e 64]
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
OUT = os.path.join(ROOT, "profiles", "paths_probe.jsonl")
HEAD_BYTES = 288          # sffk::PathsHead
CTRL_BYTES = 512          # sffk::DevCtrl, rounded


def child(a):
    import numpy as np
    import common
    import space_filling_forest_star_amd as S
    sc = common.scenario("dense3d_coarse")
    c0 = S.Context(0)
    c0.upload_env(sc["env"])
    c0.upload_robot(sc["robot"])
    ctxs = [c0]
    for _ in range(a.B):      # (one more than B: the warm-up forest's)
        if a.compact:
            os.environ["SFFGPU_COMPACT_GRID"] = "1"
            c = c0.member()
            os.environ.pop("SFFGPU_COMPACT_GRID", None)
        else:
            c = S.Context(0)
            c.upload_env(sc["env"])
            c.upload_robot(sc["robot"])
        ctxs.append(c)
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=6, max_iterations=2 ** 31 - 1, wave=1)
    roots = common.free_roots(lambda p: int(c0.collide_poses(p[None, :])[0]), sc["limits"], 10, seed=1)

    def extract(fs):
        if a.leg == "a":
            return S.paths_batch(fs)
        return [f.paths() for f in fs]

    warm = S.Forest(ctxs[0], roots, sc["limits"], seed=1000, **kw)
    S.run_batch([warm])
    extract([warm])
    if a.e2e:
        S.smooth_batch([warm])
    fs = [S.Forest(c, roots, sc["limits"], seed=1 + i, **kw) for i, c in enumerate(ctxs[1:])]
    t_all = time.perf_counter()
    S.run_batch(fs)
    t = time.perf_counter()
    res = extract(fs)
    dt = time.perf_counter() - t
    if a.e2e:
        S.smooth_batch(fs)
    dt_all = time.perf_counter() - t_all
    h = hashlib.sha256()
    n_paths = entries = 0
    for f, (d, conn) in zip(fs, res):
        assert np.any(d[~np.eye(len(d), dtype=bool)] < 1e300), "a member has no path"
        if not a.e2e:
            h.update(np.ascontiguousarray(d).tobytes())
        h.update(np.ascontiguousarray(conn).tobytes())
        for i in range(len(d)):
            for j in range(i + 1, len(d)):
                plan = f.plan(i, j)
                n_paths += int(len(plan) > 0)
                entries += len(plan)
                h.update(np.ascontiguousarray(plan).tobytes())
    st = [f.stats() for f in fs]
    nodes, borders = sum(s["n_nodes"] for s in st), sum(s["n_borders"] for s in st)
    rec = {"leg": a.leg, "build": a.build, "B": a.B, "compact": bool(a.compact), "e2e": bool(a.e2e), "repeat": a.repeat,
           "seconds": dt_all if a.e2e else dt, "paths_seconds": dt, "paths": n_paths, "entries": entries, "nodes": nodes,
           "borders": borders, "fingerprint": h.hexdigest()[:16]}
    if a.leg == "a":
        ps = [f.paths_stats() for f in fs]
        rec["device_calls"] = sum(p["device_calls"] for p in ps)
        rec["host_syncs"] = sum(p["host_syncs"] for p in ps)
        rec["fallbacks"] = sum(p["fallbacks"] for p in ps)
        # the two copies of the call: the headers, then the packed rows, ids (padded to 8 bytes) and positions
        rec["bytes_down"] = sum(HEAD_BYTES + 32 * p["pairs"] + ((4 * p["entries"] + 7) & ~7) + 48 * p["entries"] for p in ps)
    else:
        # Forest::sync_host by the code: 80 B and a flag byte per node, the frontier and closed lists, 24 B per border, the block
        rec["bytes_down"] = sum(81 * s["n_nodes"] + 4 * (s["frontier_size"] + s["closed_size"]) + 24 * s["n_borders"] + CTRL_BYTES
                                for s in st)
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", default="a")
    ap.add_argument("--build", default="new")
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--compact", type=int, default=0)
    ap.add_argument("--e2e", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=0)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--sizes", default="1,8,64")
    ap.add_argument("--compact-sizes", default="256")
    ap.add_argument("--e2e-sizes", default="64")
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
    jobs = [(int(x), 0, 0) for x in a.sizes.split(",") if x] + [(int(x), 1, 0) for x in a.compact_sizes.split(",") if x] + \
           [(int(x), 0, 1) for x in a.e2e_sizes.split(",") if x]
    for B, compact, e2e in jobs:
        recs = {"a": [], "b": []}
        for rep in range(a.repeats):
            for leg, build in (("a", "new"), ("b", "parent")):
                env = dict(os.environ)
                for k in ("SFFGPU_LIB", "SFFGPU_PATHS_DEV", "SFFGPU_TEST_PATHS_CAP", "SFFGPU_COMPACT_GRID", "SFFGPU_SMOOTH_LOOP"):
                    env.pop(k, None)
                if build == "parent":
                    env["SFFGPU_LIB"] = a.parent_lib
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", leg, "--build", build, "--B", str(B),
                       "--compact", str(compact), "--e2e", str(e2e), "--repeat", str(rep)]
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not lines:
                    print(p.stdout[-4000:])
                    sys.exit("leg %s (B = %d) ended with status %d: nothing more is started" % (leg, B, p.returncode))
                rec = json.loads(lines[0][7:])
                recs[leg].append(rec)
                with open(a.out, "a") as fp:
                    fp.write(json.dumps(rec) + "\n")
                print("leg %s %-6s B %3d%s%s rep %d: %10.3f ms  %5d paths %7d entries %9d bytes down  %s" % (
                    leg, build, B, " compact" if compact else "", " e2e" if e2e else "", rep, 1e3 * rec["seconds"], rec["paths"],
                    rec["entries"], rec["bytes_down"], rec["fingerprint"]), flush=True)
        fps = {r["fingerprint"] for leg in recs for r in recs[leg]}
        ta, tb = [r["seconds"] for r in recs["a"]], [r["seconds"] for r in recs["b"]]
        summary = {"summary": "e2e" if e2e else "paths", "B": B, "compact": bool(compact),
                   "a_median_ms": 1e3 * statistics.median(ta), "a_min_ms": 1e3 * min(ta), "a_max_ms": 1e3 * max(ta),
                   "b_median_ms": 1e3 * statistics.median(tb), "b_min_ms": 1e3 * min(tb), "b_max_ms": 1e3 * max(tb),
                   "speedup_of_medians": statistics.median(tb) / statistics.median(ta), "slowest_a_beats_fastest_b": max(ta) < min(tb),
                   "paths": recs["a"][0]["paths"], "entries": recs["a"][0]["entries"], "nodes": recs["a"][0]["nodes"],
                   "a_bytes_down": recs["a"][0]["bytes_down"], "b_bytes_down": recs["b"][0]["bytes_down"],
                   "a_device_calls": recs["a"][0].get("device_calls"), "a_host_syncs": recs["a"][0].get("host_syncs"),
                   "a_fallbacks": recs["a"][0].get("fallbacks"), "results_equal": len(fps) == 1}
        with open(a.out, "a") as fp:
            fp.write(json.dumps(summary) + "\n")
        print("SUMMARY " + json.dumps(summary), flush=True)
        if len(fps) != 1:
            sys.exit("B = %d: the two legs disagree: %s" % (B, sorted(fps)))


if __name__ == "__main__":
    main()
