"""The jobs of tests/test_gpu_smooth_batch.py: for each, the smallest planner found at which a part of k_smooth_paths has
something to decide, and its CPU-oracle reference - computed once, shared by the cases, never advanced again.

  T    triang, 6 roots, wave 1: short edges, the inline clearance path decides the free ones
  D2   dense2d, wave 16: long edges (many rounds of four chunks, the flat grid), steps with no free candidate
  D3   dense3d_coarse
  E    triang, the 5 XML points: no two trees meet, no path
  TS   SFF* (optimize) on triang
  R1   Multi-T-RRT on triang (the first case of test_rrt_identical), R2 on dense2d

The oracle's collide_calls belongs to its World, so every reference gets a World of its own, and nothing else is asked of
that World between run() and the last figure taken here."""
import numpy as np

import common
import oracle_lib as O


def _near_roots(w, sc, n, seed, reach):
    """XML point 0 and n - 1 seeded offsets of it within +-reach, drawn in sequence, those that do not collide kept"""
    rs = np.random.RandomState(seed)
    roots = [sc["xml_points"][0].copy()]
    while len(roots) < n:
        p = sc["xml_points"][0].copy()
        p[:3] += rs.uniform(-reach, reach, 3)
        if not w.collide(p):
            roots.append(p)
    return np.array(roots)


FORESTS = {
    # name: (scenario, roots(w, sc), wave, iterations, seed, optimize)
    "T": ("triang", lambda w, sc: _near_roots(w, sc, 6, 9, 25.0), 1, 8000, 9, False),
    "D2": ("dense2d", lambda w, sc: sc["xml_points"][:4], 16, 3000, 3, False),
    "D3": ("dense3d_coarse", lambda w, sc: common.free_roots(w.collide, sc["limits"], 5, seed=2), 1, 3000, 2, False),
    "E": ("triang", lambda w, sc: sc["xml_points"][:5], 1, 3000, 4, False),
    "TS": ("triang", lambda w, sc: _near_roots(w, sc, 4, 7, 15.0), 1, 4000, 7, True),
}
SESSIONS = {
    # name: (scenario, roots, iterations, seed)
    "R1": ("triang", 4, 1500, 3),
    "R2": ("dense2d", 3, 800, 3),
}

_ref = {}


def _plans(f, n):
    return {(i, j): f.plan(i, j) for i in range(n) for j in range(i + 1, n)}


def forest_job(name):
    """(scenario dict, roots, constructor keywords) of a forest shape"""
    scn, roots_of, wave, iters, seed, optimize = FORESTS[name]
    sc = common.scenario(scn)
    w = O.World(sc["env"], sc["robot"], O.TRIG_PORTABLE)
    roots = roots_of(w, sc)
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=sc["dim"], max_iterations=iters, wave=wave,
              seed=seed, optimize=optimize)
    return sc, roots, kw


def forest_ref(name):
    """the oracle's forest of a shape: raw matrix and plans, and after smooth() once and twice the matrix, the plans, the two
    reference-equivalent counters and how many isPathFree calls the smoothing made"""
    if name in _ref:
        return _ref[name]
    sc, roots, kw = forest_job(name)
    w = O.World(sc["env"], sc["robot"], O.TRIG_PORTABLE)      # (its own: _near_roots / free_roots asked another one)
    fo = O.Forest(w, roots, sc["limits"], **kw)
    fo.run()
    n = len(roots)
    ref = dict(scenario=FORESTS[name][0], sc=sc, roots=roots, kw=kw, n=n, n_nodes=fo.stats()["n_nodes"], raw=fo.paths(),
               raw_plans=_plans(fo, n), stages=[], pos=fo.nodes()["pos"])
    pf = fo.stats()["path_free_calls"]
    for _ in range(2):
        d = fo.smooth()
        st = fo.stats()
        ref["stages"].append(dict(dist=d, plans=_plans(fo, n), path_free_calls=st["path_free_calls"],
                                  collide_calls=st["collide_calls"], edges=st["path_free_calls"] - pf))
        pf = st["path_free_calls"]
    ref["keep"] = (fo, w)
    _ref[name] = ref
    return ref


def session_job(name):
    scn, n_roots, iters, seed = SESSIONS[name]
    sc = common.scenario(scn)
    roots = sc["xml_points"][:n_roots]
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=sc["dim"], optimize=False, goal=None,
              priority_bias=0.0, max_iterations=iters, seed=seed)
    return sc, roots, kw


def session_ref(name):
    if name in _ref:
        return _ref[name]
    sc, roots, kw = session_job(name)
    w = O.World(sc["env"], sc["robot"], O.TRIG_PORTABLE)
    ro = O.Rrt(w, roots, sc["limits"], **kw)
    ro.run()
    nt = len(roots)
    d, k = ro.paths(nt)
    pf = ro.stats()["path_free_calls"]
    plans = ro.smooth()
    st = ro.stats()
    ref = dict(scenario=SESSIONS[name][0], sc=sc, roots=roots, kw=kw, nt=nt, dist=d, plans=plans,
               path_free_calls=st["path_free_calls"], collide_calls=st["collide_calls"], edges=st["path_free_calls"] - pf,
               keep=(ro, w))
    _ref[name] = ref
    return ref


def walk_figures(name):
    """smoothPaths' walk over the raw plans of a forest shape, replayed with World.path_free on a World of its own (the
    reference's figures are not touched): steps, steps without a free candidate, and per tested edge (free, first hit,
    samples)"""
    ref = forest_ref(name)
    w = O.World(ref["sc"]["env"], ref["sc"]["robot"], O.TRIG_PORTABLE)
    pos = ref["pos"]
    steps = none_free = 0
    edges = []
    for ij in sorted(ref["raw_plans"]):
        plan = ref["raw_plans"][ij]
        g = len(plan) - 1
        while g > 0:
            t, found = 0, False
            while t < g - 1:
                free, fh, ns = w.path_free(pos[plan[t]], pos[plan[g]])
                edges.append((bool(free), fh, ns))
                if free:
                    found = True
                    break
                t += 1
            steps += 1
            none_free += int(g > 1 and not found)
            g = t
    return dict(steps=steps, none_free=none_free, edges=edges)
