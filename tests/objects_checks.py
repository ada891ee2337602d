"""What the CPU and the GPU tests of the object segmenter share (include/vlsat_objects.h): an independent restatement of the plane rule
with plain loops and scalars (one rounded operation per line, nothing of the vectorised restatement's broadcasting), a breadth-first
search for the clusters, the generated clouds with their settings, and the numpy restatement's answers computed once per process."""
import functools

import numpy as np

from cloud_checks import assert_bit_equal, bits  # noqa: F401

M64 = (1 << 64) - 1


def draw(seed, k, n):
    """splitmix64 of (seed, k), the top 32 bits scaled to n, in Python integers"""
    z = (seed + 0x9E3779B97F4A7C15 * (k + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def scalar_plane(a, b, c):
    """rule 3 on three points, np.float64 scalars, one operation per line -> (nx, ny, nz, d) as np.float32, or None when void"""
    f = np.float64
    with np.errstate(all="ignore"):
        ax, ay, az = f(a[0]), f(a[1]), f(a[2])
        ux, uy, uz = f(b[0]) - ax, f(b[1]) - ay, f(b[2]) - az
        vx, vy, vz = f(c[0]) - ax, f(c[1]) - ay, f(c[2]) - az
        p, q = uy * vz, uz * vy
        mx = p - q
        p, q = uz * vx, ux * vz
        my = p - q
        p, q = ux * vy, uy * vx
        mz = p - q
        xx, yy, zz = mx * mx, my * my, mz * mz
        s = xx + yy
        l2 = s + zz
        if not (l2 > 0 and np.isfinite(l2)):
            return None
        length = np.sqrt(l2)
        n = [mx / length, my / length, mz / length]
        big = n[0]
        for comp in n[1:]:
            if abs(comp) > abs(big):
                big = comp
        if big < 0:
            n = [-x for x in n]
        p, q, r = n[0] * ax, n[1] * ay, n[2] * az
        s = p + q
        d = -(s + r)
    return tuple(np.float32(x) for x in (*n, d))


def scalar_score(plane, point):
    f = np.float32
    with np.errstate(all="ignore"):
        p, q, r = f(plane[0] * f(point[0])), f(plane[1] * f(point[1])), f(plane[2] * f(point[2]))
        s = f(p + q)
        s = f(s + r)
        return f(s + plane[3])


def brute_planes(points, n_hyp, max_planes, dist, min_inliers, outside_ppm, seed=0):
    """the whole rule, one point and one hypothesis at a time -> (plane_id, planes, counts, n_planes) as the restatement returns them"""
    p = np.asarray(points, dtype=np.float32)
    dist = np.float32(dist)
    alive = [bool(np.isfinite(row).all()) for row in p]
    plane_id = np.zeros(len(p), dtype=np.int32)
    planes = np.zeros((max_planes, 4), dtype=np.float32)
    counts = np.zeros((max_planes, 3), dtype=np.int32)
    found = 0
    for r in range(max_planes):
        idx = [i for i in range(len(p)) if alive[i]]
        n = len(idx)
        if n < 3:
            break
        best = None
        for h in range(n_hyp):
            a, b, c = (p[idx[draw(seed, (r * n_hyp + h) * 3 + j, n)]] for j in range(3))
            plane = scalar_plane(a, b, c)
            if plane is None:
                continue
            inl = abv = 0
            members = []
            for i in idx:
                s = scalar_score(plane, p[i])
                if abs(s) <= dist:
                    inl += 1
                    members.append(i)
                elif s > dist:
                    abv += 1
            below = n - inl - abv
            if inl >= min_inliers and min(abv, below) <= (n * outside_ppm) // 1000000 and (best is None or inl > best[0]):
                best = (inl, abv, below, plane, members)
        if best is None:
            break
        planes[r], counts[r] = best[3], best[:3]
        for i in best[4]:
            plane_id[i], alive[i] = r + 1, False
        found = r + 1
    return plane_id, planes, counts, np.asarray([found], dtype=np.int32)


def brute_clusters(index, sqdist, mask, max_sq_dist, min_points):
    """breadth-first search over the undirected edges of the table -> (labels, n_clusters, cluster_size)"""
    index, sqdist = np.asarray(index), np.asarray(sqdist, dtype=np.float32)
    v, k = index.shape
    on = [bool(m) for m in np.asarray(mask).reshape(-1)]
    adj = [set() for _ in range(v)]
    for i in range(v):
        for s in range(k):
            j = int(index[i, s])
            if 0 <= j < v and j != i and on[i] and on[j] and sqdist[i, s] <= np.float32(max_sq_dist):
                adj[i].add(j)
                adj[j].add(i)
    labels = np.zeros(v, dtype=np.int32)
    seen = [False] * v
    sizes = []
    for i in range(v):                                 # ascending: a component is met at its lowest point
        if seen[i] or not on[i]:
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
            sizes.append(len(comp))
            labels[comp] = len(sizes)
    size = np.zeros(v, dtype=np.int32)
    size[:len(sizes)] = sizes
    return labels, np.asarray([len(sizes)], dtype=np.int32), size


# ---- the clouds -------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng([seed, 0x0B1EC7])


@functools.lru_cache(maxsize=None)
def boxes():
    """synth.make_box_mesh(3, 0.1, 1) without faces, every coordinate jittered by N(0, 0.002): 11 245 points, no multiple of any tile"""
    from vlsat_amd import synth
    room = synth.make_box_mesh(3, 0.1, 1)
    p = (room["points"] + _rng(1).normal(0, 0.002, room["points"].shape)).astype(np.float32)
    p.setflags(write=False)
    return p, room


@functools.lru_cache(maxsize=None)
def big_boxes():
    """the issue's end-to-end room: synth.make_box_mesh(12, 0.05, 3) without faces plus N(0, 0.002): 59 429 points"""
    from vlsat_amd import synth
    room = synth.make_box_mesh(12, 0.05, 3)
    return room["points"] + _rng(2).normal(0, 0.002, room["points"].shape), room


@functools.lru_cache(maxsize=None)
def walled():
    """synth.make_walled_room(3, 0.1, 3, 2.0, (3, 3)) plus N(0, 0.002): a floor, four walls and three boxes, one with a top of 100 points"""
    from vlsat_amd import synth
    room = synth.make_walled_room(3, 0.1, 3, height=2.0, extent=(3.0, 3.0))
    p = room["points"] + _rng(3).normal(0, 0.002, room["points"].shape)
    return p, room


def _flat(v, seed):
    """v points on the plane z = 0.5 at dyadic x, y (fp32 is exact), every fifth lifted off it"""
    g = _rng(seed)
    p = np.concatenate([g.integers(-64, 64, (v, 2)) / 16.0, np.full((v, 1), 0.5)], 1).astype(np.float32)
    p[4::5, 2] += np.float32(1.0) + (np.arange(len(p[4::5])) % 3).astype(np.float32)
    return p


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (points f32 [V,3], dict of the arguments of cloud_planes after the points)"""
    from vlsat_amd import synth
    if name.startswith("boxes_h"):                     # H in {1, 65, 256, 300}: a lone lane, one block and a tail, one block, two per thread
        return boxes()[0], dict(n_hyp=int(name[7:]), max_planes=3, dist=0.02, min_inliers=225, outside_ppm=10000, seed=int(name[7:]))
    if name == "boxes_one_plane":
        return boxes()[0], dict(n_hyp=65, max_planes=1, dist=0.02, min_inliers=225, outside_ppm=10000, seed=2)
    if name == "boxes_tops":                           # half of the rest may lie outside: box tops and sides follow the floor
        return boxes()[0], dict(n_hyp=300, max_planes=6, dist=0.02, min_inliers=40, outside_ppm=500000, seed=5)
    if name == "plates":                               # two perpendicular plates, both structural; max_planes beyond them: an early stop
        p = synth.make_plates(0.05, 0.002, 1)["points"].astype(np.float32)
        return p, dict(n_hyp=65, max_planes=5, dist=0.01, min_inliers=100, outside_ppm=10000, seed=3)
    if name == "walled":
        p = walled()[0].astype(np.float32)
        return p, dict(n_hyp=256, max_planes=8, dist=0.02, min_inliers=60, outside_ppm=10000, seed=0)
    if name.startswith("v"):                           # V in {3, 64, 65, 257}: the wave and block edges of the scan
        v = int(name[1:])
        p = np.array([[0, 0, 0.5], [1, 0, 0.5], [0, 1, 0.5]], dtype=np.float32) if v == 3 else _flat(v, v)
        return p, dict(n_hyp=8 if v == 3 else 40, max_planes=3, dist=0.125, min_inliers=3, outside_ppm=250000, seed=v)
    if name == "nonfinite":                            # every seventh row has a NaN, +inf or -inf in one coordinate
        p = np.array(boxes()[0][::3])
        bad = np.arange(0, len(p), 7)
        p[bad, bad % 3] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[(bad // 7) % 3]
        return p, dict(n_hyp=65, max_planes=3, dist=0.02, min_inliers=70, outside_ppm=10000, seed=9)
    if name == "coincident":
        return np.full((70, 3), 0.25, dtype=np.float32), dict(n_hyp=40, max_planes=3, dist=0.125, min_inliers=3, outside_ppm=500000, seed=1)
    if name == "huge":                                 # coordinates near the largest fp32: d overflows to inf and every score is inf or NaN
        p = (_rng(4).uniform(-1, 1, (200, 3)) * 3e38).astype(np.float32)
        return p, dict(n_hyp=40, max_planes=2, dist=1e30, min_inliers=3, outside_ppm=500000, seed=4)
    raise KeyError(name)


PLANE_CASES = ("boxes_h1", "boxes_h65", "boxes_h256", "boxes_h300", "boxes_one_plane", "boxes_tops", "plates", "walled", "v3", "v64", "v65",
               "v257", "nonfinite", "coincident", "huge")
SMALL_CASES = ("v3", "v64", "v65", "coincident")      # small enough for brute_planes


@functools.lru_cache(maxsize=None)
def host_planes(name):
    from vlsat_amd import prep
    p, kw = case(name)
    return prep.cloud_planes_host(p, **kw)


def assert_same_planes(got, want, what=""):
    for g, w, part in zip(got, want, ("plane_id", "planes", "counts", "n_planes")):
        assert_bit_equal(np.asarray(g), np.asarray(w), (what, part))


def assert_same_clusters(got, want, what=""):
    for g, w, part in zip(got, want, ("labels", "n_clusters", "cluster_size")):
        assert_bit_equal(np.asarray(g), np.asarray(w), (what, part))


# ---- cluster tables made by hand ------------------------------------------------------------------------------------------------------
def blobs(bridge_mask):
    """two blobs of 30 points on a line at spacing 0.1, 1.0 apart, and ONE bridge point half-way, 0.5 from the nearest end
    of each -> (points, mask); the radius of the cases is 0.6, so the blobs meet only through the bridge"""
    x = np.concatenate([np.arange(30) * 0.1, 3.9 + np.arange(30) * 0.1, [3.4]])
    p = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1).astype(np.float32)
    mask = np.ones(len(p), dtype=np.int32)
    mask[-1] = bridge_mask
    return p, mask


def knn(points, k, radius):
    from vlsat_amd import prep
    return prep.knn_points_host(points, k, float(np.float32(radius) ** 2))
