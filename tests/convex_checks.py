"""What the CPU and the GPU tests of the convexity clusters share (include/vlsat_convex.h): an independent restatement of the rule with
plain loops and scalars (one rounded operation per line, a breadth-first search for the components, nothing of the vectorised
restatement's indexing and not its union-find), the cases with their settings, and the numpy restatement's answers computed once per
process."""
import functools

import numpy as np

from cloud_checks import assert_bit_equal, bits  # noqa: F401

PARTS = ("labels", "n_clusters", "cluster_size", "state")


def scalar_c(xi, ni, xj, nj):
    """rule 2 on one entry, np.float32 scalars, one operation per line -> c"""
    f = np.float32
    with np.errstate(all="ignore"):
        dx, dy, dz = f(f(xj[0]) - f(xi[0])), f(f(xj[1]) - f(xi[1])), f(f(xj[2]) - f(xi[2]))
        p, q, r = f(f(ni[0]) * dx), f(f(ni[1]) * dy), f(f(ni[2]) * dz)
        a = f(p + q)
        a = f(a + r)
        p, q, r = f(f(nj[0]) * dx), f(f(nj[1]) * dy), f(f(nj[2]) * dz)
        b = f(p + q)
        b = f(b + r)
        return f(a - b)


def scalar_concave(c, tau, q):
    f = np.float32
    with np.errstate(all="ignore"):
        cc = f(f(c) * f(c))
        tt = f(f(tau) * f(tau))
        return bool(c > 0) and bool(cc > f(tt * f(q)))


def brute_convex(points, normals, knn_index, knn_sqdist, mask, link_sq_dist, concavity, min_points=1, absorb_rounds=8):
    """the whole rule, one point and one entry at a time -> (labels, n_clusters, cluster_size, state) as the restatement returns them"""
    p, n = np.asarray(points, dtype=np.float32), np.asarray(normals, dtype=np.float32)
    index, sqdist = np.asarray(knn_index), np.asarray(knn_sqdist, dtype=np.float32)
    v, k = index.shape
    link, tau = np.float32(link_sq_dist), np.float32(concavity)
    on = [bool(m) for m in np.asarray(mask).reshape(-1)]
    eligible = [on[i] and all(np.isfinite(c) for c in p[i]) for i in range(v)]
    oriented = [eligible[i] and all(np.isfinite(c) for c in n[i]) and any(c != 0 for c in n[i]) for i in range(v)]
    boundary = [False] * v
    for i in range(v):
        for s in range(k):
            j, q = int(index[i, s]), sqdist[i, s]
            if not (0 <= j < v) or j == i or not (oriented[i] and oriented[j]) or not (np.isfinite(q) and q >= 0):
                continue
            if scalar_concave(scalar_c(p[i], n[i], p[j], n[j]), tau, q):
                boundary[i] = boundary[j] = True
    core = [oriented[i] and not boundary[i] for i in range(v)]
    adj = [set() for _ in range(v)]
    for i in range(v):
        for s in range(k):
            j = int(index[i, s])
            if 0 <= j < v and j != i and core[i] and core[j] and sqdist[i, s] <= link:
                adj[i].add(j)
                adj[j].add(i)
    label = [0] * v                                    # the final number, 0 = unlabelled: the kept components are met at their lowest point
    seen = [False] * v
    dissolved = [False] * v
    kept = 0
    for i in range(v):
        if seen[i] or not core[i]:
            continue
        comp, todo = [i], [i]
        seen[i] = True
        while todo:
            for j in adj[todo.pop()]:
                if not seen[j]:
                    seen[j] = True
                    comp.append(j)
                    todo.append(j)
        if len(comp) >= min_points:
            kept += 1
            for x in comp:
                label[x] = kept
        else:
            for x in comp:
                dissolved[x] = True
    state = [0 if not eligible[i] else 2 if boundary[i] else 3 if not oriented[i] else 4 if dissolved[i] else 1 for i in range(v)]
    for _ in range(absorb_rounds):
        before = list(label)
        for i in range(v):
            if before[i] or not eligible[i]:
                continue
            for s in range(k):
                j = int(index[i, s])
                if 0 <= j < v and j != i and before[j]:
                    label[i] = before[j]
                    break
    size = np.zeros(v, dtype=np.int32)
    for x in label:
        if x:
            size[x - 1] += 1
    return np.asarray(label, dtype=np.int32), np.asarray([kept], dtype=np.int32), size, np.asarray(state, dtype=np.int32)


def assert_same(got, want, what=""):
    got, want = list(got), list(want)
    assert len(got) == len(want) == 4
    for g, w, part in zip(got, want, PARTS):
        assert_bit_equal(np.asarray(g), np.asarray(w), (what, part))


# ---- the clouds -------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng([seed, 0xC0117E8])


def _sq(x):
    return float(np.float32(x) ** 2)


def knn(points, k, radius):
    from vlsat_amd import prep
    return prep.knn_points_host(points, k, _sq(radius))


def hand():
    """ten points made by hand, K = 4: a floor line z = 0 (points 0..3 and 9, normal up) and a wall line x = 0 (4..6, normal +x) that
    meet in a concave junction between 0 and 4; 7 has a zero normal, 8 a NaN coordinate.  The rows hold pads, entries out of range,
    self entries and NaN / inf / negative distances.  -> (points, normals, index, sqdist)"""
    nan, inf = np.nan, np.inf
    p = np.array([[1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0], [0, 0, 1], [0, 0, 2], [0, 0, 3], [0.5, 0, 0.5], [nan, 0, 0], [5, 0, 0]], dtype=np.float32)
    n = np.array([[0, 0, 1]] * 4 + [[1, 0, 0]] * 3 + [[0, -0.0, 0], [0, 0, 1], [0, 0, 1]], dtype=np.float32)
    index = np.array([[4, 1, 0, -1], [0, 2, 99, 7], [1, 3, -5, 1 << 30], [2, 9, 3, -1], [0, 5, 7, -1], [4, 6, -1, -1], [5, 4, -1, -1],
                      [0, 4, 8, -1], [0, 1, 2, 3], [3, -1, -1, -1]], dtype=np.int32)
    sqdist = np.array([[2, 1, 0, inf], [1, 1, 0, 0.5], [1, 1, 0, 0], [1, 1, 0, inf], [nan, 1, 0.5, inf], [1, 1, inf, inf], [1, 4, inf, inf],
                       [0.5, 0.5, nan, inf], [1, 4, 9, 16], [1, inf, inf, inf]], dtype=np.float32)
    return p, n, index, sqdist


def hand_wild():
    """the same ten points with a table that means nothing: every kind of entry in every place, distances that are NaN, inf, negative
    or huge, and normals that are NaN, inf or zero"""
    p, n, index, sqdist = hand()
    g = _rng(11)
    index = g.choice(np.array([-1, -7, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 99, 1 << 30, -(1 << 31)], dtype=np.int64), (10, 5)).astype(np.int32)
    sqdist = g.choice(np.array([0, -0.0, 0.25, 1, 2, 9, np.nan, np.inf, -np.inf, -1, 3e38], dtype=np.float32), (10, 5))
    n = np.array(n)
    n[2], n[5], n[9] = (np.nan, 0, 1), (0, np.inf, 0), (3e38, 3e38, -3e38)
    return p, n, index, sqdist


@functools.lru_cache(maxsize=None)
def plates():
    """synth.make_plates(0.05, 0.002, 1): 861 points, the table of 16 within 0.15 -> (points f32, table)"""
    from vlsat_amd import synth
    p = synth.make_plates(0.05, 0.002, 1)["points"].astype(np.float32)
    p.setflags(write=False)
    return p, knn(p, 16, 0.15)


PLATES_OUTSIDE = (-1.0, 0.5, -1.0)     # the L seen from behind both plates (x < 0 and z < 0): the crease is the CONVEX edge of a box
PLATES_INSIDE = (1.0, 0.5, 1.0)        # seen from between them, as a floor and a wall are from inside the room: a CONCAVE junction


@functools.lru_cache(maxsize=None)
def stacked():
    """synth.make_stacked_boxes() with the table of 16 within 0.06 and the normals estimated over it, turned to its viewpoint
    -> (points f32, scene, table, estimated normals, exact normals f32)"""
    from vlsat_amd import prep, synth
    scene = synth.make_stacked_boxes()
    p = scene["points"].astype(np.float32)
    p.setflags(write=False)
    table = knn(p, 16, 0.06)
    est = prep.cloud_normals_host(p, table.index, table.count, 5, scene["viewpoint"])[0]
    return p, scene, table, est, scene["normals"].astype(np.float32)


def _random_cloud(v, k, seed):
    """v points in a slab with random unit normals, every ninth normal zero or NaN; the table of k within 0.5"""
    g = _rng(seed)
    p = (g.uniform(0, 1, (v, 3)) * np.array([1.0, 1.0, 0.2])).astype(np.float32)
    n = g.standard_normal((v, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    n[4::9] = 0
    n[8::18, 1] = np.nan
    return p, n, knn(p, k, 0.5)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> the arguments of prep.convex_clusters as a dict"""
    from vlsat_amd import prep

    def args(p, n, index, sqdist, mask=None, link=0.03, tau=0.17, min_points=1, rounds=8):
        mask = np.ones(len(p), dtype=np.int32) if mask is None else np.asarray(mask, dtype=np.int32)
        return dict(points=p, normals=n, knn_index=index, knn_sqdist=sqdist, mask=mask, link_sq_dist=_sq(link), concavity=tau,
                    min_points=min_points, absorb_rounds=rounds)

    if name.startswith("hand_r"):                      # absorb_rounds 0, 1, 2, 8, 64
        return args(*hand(), link=1.25, tau=0.5, rounds=int(name[6:]))
    if name == "hand_min3":                            # the wall's two cores are dissolved, and absorbed by the floor through the junction
        return args(*hand(), link=1.25, tau=0.5, min_points=3)
    if name == "hand_masks":                           # masks 0, 7 and -1: point 1 is out, the floor falls apart
        return args(*hand(), mask=[7, 0, -1, 1, 1, 1, 1, 1, 1, 1], link=1.25, tau=0.5)
    if name == "hand_tau0":                            # tau = 0: every positive c is concave
        return args(*hand(), link=np.inf, tau=0.0)
    if name == "hand_tau1":                            # tau = 1: c^2 > q never holds for unit normals at these distances but 2^2 > 2
        return args(*hand(), link=1.25, tau=1.0)
    if name == "hand_wild":
        return args(*hand_wild(), mask=[1, 1, 1, 1, 1, 1, -1, 7, 1, 0], link=2.0, tau=0.3, rounds=3)
    if name.startswith("v"):                           # v<V>_k<K>: V in {1, 2, 64, 65, 257}, K in {1, 16, 32}
        v, k = (int(x) for x in name[1:].split("_k"))
        p, n, t = _random_cloud(v, k, v * 100 + k)
        return args(p, n, t.index, t.sqdist, link=0.3, tau=0.5, min_points=2 if v > 2 else 1, rounds=4)
    if name in ("plates_convex", "plates_concave"):
        p, t = plates()
        n = prep.cloud_normals_host(p, t.index, t.count, 5, PLATES_OUTSIDE if name == "plates_convex" else PLATES_INSIDE)[0]
        return args(p, n, t.index, t.sqdist, link=0.075, min_points=20)
    if name.startswith("stacked"):
        p, scene, t, est, exact = stacked()
        if name == "stacked":                          # the prototype's setting
            return args(p, est, t.index, t.sqdist, min_points=20)
        if name == "stacked_exact":
            return args(p, exact, t.index, t.sqdist, min_points=20)
        if name == "stacked_min1":
            return args(p, est, t.index, t.sqdist, min_points=1)
        if name.startswith("stacked_r"):               # absorb_rounds 0, 1, 64
            return args(p, est, t.index, t.sqdist, min_points=20, rounds=int(name[9:]))
        if name == "stacked_masked":                   # the mask removes a body: the box between the table's two other boxes
            return args(p, est, t.index, t.sqdist, mask=(scene["instances"] != 5), min_points=20)
        if name == "stacked_nonfinite":                # every seventh row has a NaN or inf coordinate, every eleventh a NaN or inf normal
            p, n = np.array(p), np.array(est)
            bad = np.arange(0, len(p), 7)
            p[bad, bad % 3] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[(bad // 7) % 3]
            bad = np.arange(3, len(p), 11)
            n[bad, bad % 3] = np.array([np.nan, np.inf], dtype=np.float32)[(bad // 11) % 2]
            return args(p, n, t.index, t.sqdist, min_points=20)
    raise KeyError(name)


HAND_CASES = ("hand_r0", "hand_r1", "hand_r2", "hand_r8", "hand_r64", "hand_min3", "hand_masks", "hand_tau0", "hand_tau1", "hand_wild")
SIZE_CASES = tuple(f"v{v}_k{k}" for v in (1, 2, 64, 65, 257) for k in (1, 16, 32))
PLATE_CASES = ("plates_convex", "plates_concave")
STACKED_CASES = ("stacked", "stacked_exact", "stacked_min1", "stacked_r0", "stacked_r1", "stacked_r64", "stacked_masked", "stacked_nonfinite")
CASES = HAND_CASES + SIZE_CASES + PLATE_CASES + STACKED_CASES


@functools.lru_cache(maxsize=None)
def host(name):
    from vlsat_amd import prep
    return prep.convex_clusters_host(**case(name))


def floor_scene():
    """the stacked boxes standing on a floor: make_stacked_boxes' points plus a grid z = 0 of spacing 0.02 over [-0.5, 1.9] x [-0.5, 1.5]
    where no body stands, with N(0, 0.0008) -> (points f64, viewpoint)"""
    from vlsat_amd import synth
    scene = synth.make_stacked_boxes()
    x, y = (a.ravel() for a in np.meshgrid(np.arange(-25, 96) * 0.02, np.arange(-25, 76) * 0.02, indexing="ij"))
    free = ~(((x > -0.001) & (x < 1.001) & (y > -0.001) & (y < 1.001)) | ((x > 0.999) & (x < 1.401) & (y > 0.199) & (y < 0.601)))
    floor = np.stack([x[free], y[free], np.zeros(int(free.sum()))], 1) + _rng(5).normal(0, 0.0008, (int(free.sum()), 3))
    return np.concatenate([scene["points"], floor]), scene["viewpoint"]
