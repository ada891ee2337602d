"""What the CPU and the GPU tests of the point-cloud front end share (include/vlsat_cloud.h): a brute-force neighbour search written
with plain loops and without the restatement's key, the generated clouds, and the host restatement's answers computed once per process."""
import functools

import numpy as np

KS = (1, 8, 9, 16, 32)


def brute_knn(points, k, max_sq_dist):
    """O(V^2), one pair at a time: for every valid point the valid others within max_sq_dist, ordered by (distance, index) as a tuple,
    cut to k -> (index [V,k] padded with -1, sqdist [V,k] padded with +inf, count [V]).  The distance is computed in fp32 scalars,
    one rounded operation per line."""
    p = np.asarray(points, dtype=np.float32)
    v, limit = len(p), np.float32(max_sq_dist)
    index = np.full((v, k), -1, dtype=np.int32)
    sqdist = np.full((v, k), np.inf, dtype=np.float32)
    count = np.zeros(v, dtype=np.int32)
    valid = [bool(np.isfinite(row).all()) for row in p]
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(v):
            if not valid[i]:
                continue
            found = []
            for j in range(v):
                if j == i or not valid[j]:
                    continue
                dx = np.float32(p[i, 0] - p[j, 0])
                dy = np.float32(p[i, 1] - p[j, 1])
                dz = np.float32(p[i, 2] - p[j, 2])
                xx = np.float32(dx * dx)
                yy = np.float32(dy * dy)
                zz = np.float32(dz * dz)
                s = np.float32(xx + yy)
                d2 = np.float32(s + zz)
                if d2 <= limit:
                    found.append((float(d2), j))
            found.sort()
            count[i] = min(len(found), k)
            for slot, (d2, j) in enumerate(found[:k]):
                index[i, slot] = j
                sqdist[i, slot] = np.float32(d2)
    return index, sqdist, count


def _rng(seed):
    return np.random.default_rng([seed, 0xC10D])


def grid_cloud():
    """a regular 12 x 12 x 6 lattice of spacing 1/8 (exact in fp32): distance ties everywhere, several cells per axis at radius 3/16"""
    i, j, k = (x.ravel() for x in np.meshgrid(np.arange(12), np.arange(12), np.arange(6), indexing="ij"))
    return (np.stack([i, j, k], 1) * 0.125).astype(np.float32), 0.1875


def duplicate_cloud():
    """300 random points, each three times, shuffled: coincident points are each other's nearest neighbours at distance 0"""
    g = _rng(1)
    p = np.repeat(g.uniform(0, 1, (300, 3)), 3, axis=0)
    return p[g.permutation(len(p))].astype(np.float32), 0.2


def nonfinite_cloud():
    """500 random points of which every seventh row has a NaN, +inf or -inf in one coordinate"""
    g = _rng(2)
    p = g.uniform(-1, 1, (500, 3)).astype(np.float32)
    bad = np.arange(0, 500, 7)
    p[bad, bad % 3] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[(bad // 7) % 3]
    return p, 0.3


def single_cloud():
    return np.array([[0.25, -1.5, 3.0]], dtype=np.float32), 1.0


def v257_cloud():
    """one more point than a block of threads"""
    return _rng(3).uniform(0, 1, (257, 3)).astype(np.float32), 0.25


def density_cloud():
    """a dense ball (far more than 32 points within the radius), a sparse shell (a few) and far-away loners (none) in one cloud"""
    g = _rng(4)
    dense = g.normal(0, 0.03, (400, 3))
    sparse = g.uniform(-2, 2, (300, 3))
    lone = np.array([[50.0, 0, 0], [0, 60.0, 0], [0, 0, -70.0], [40.0, 40.0, 40.0]])
    p = np.concatenate([dense, sparse, lone])
    return p[g.permutation(len(p))].astype(np.float32), 0.2


def radius0_cloud():
    """radius 0: only coincident points are neighbours"""
    return duplicate_cloud()[0][:450], 0.0


def one_cell_cloud():
    """a radius larger than the extent: the grid is one cell and every point a candidate of every other"""
    return _rng(5).uniform(0, 1, (400, 3)).astype(np.float32), 10.0


def many_cells_cloud():
    """a thin slab, 40 x 25 x 3 cells at radius 0.05"""
    g = _rng(6)
    return (g.uniform(0, 1, (3000, 3)) * np.array([2.0, 1.25, 0.15])).astype(np.float32), 0.05


CLOUDS = {"grid": grid_cloud, "duplicates": duplicate_cloud, "nonfinite": nonfinite_cloud, "single": single_cloud, "v257": v257_cloud,
          "density": density_cloud, "radius0": radius0_cloud, "one_cell": one_cell_cloud, "many_cells": many_cells_cloud}


@functools.lru_cache(maxsize=None)
def cloud(name):
    """(points f32 [V,3], max_sq_dist as the float32 the callers pass on)"""
    p, radius = CLOUDS[name]()
    p.setflags(write=False)
    return p, float(np.float32(radius) ** 2)


@functools.lru_cache(maxsize=None)
def host_knn(name, k):
    from vlsat_amd import prep
    p, m = cloud(name)
    return prep.knn_points_host(p, k, m)


VIEWPOINT = (0.4, 0.3, 5.0)


@functools.lru_cache(maxsize=None)
def host_normals(name, k, with_viewpoint):
    from vlsat_amd import prep
    t = host_knn(name, k)
    return prep.cloud_normals_host(cloud(name)[0], t.index, t.count, 5, VIEWPOINT if with_viewpoint else None)


@functools.lru_cache(maxsize=None)
def small_room():
    """synth.make_box_mesh(3, 0.1, 1, extent=(3, 3)): 2005 vertices, the room the header's sweep counts were measured on"""
    from vlsat_amd import synth
    return synth.make_box_mesh(3, 0.1, 1, extent=(3, 3))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def assert_bit_equal(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    same = bits(got) == bits(want)
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:5].tolist())
