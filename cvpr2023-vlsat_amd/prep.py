"""Input preparation on the GPU: host-side mirror of the per-object part of
``SSGDatasetGraph.data_preparation`` (reference ``src/dataset/dataset_3dssg.py:279-294``), of the
fully-connected edge list (``:264-266``) and of ``collate_fn_mmg`` (``src/dataset/DataLoader.py:153-176``).
The selection of an object's points (``np.where(instances == id)`` + ``np.random.choice``, ``:285-289``) runs on the device too
(``sample_objects``): its index lists are np.where's, its draws come from a documented counter-based generator, not numpy's."""
from __future__ import annotations

from typing import NamedTuple, Sequence

import torch

from . import lib as L


def sample_objects(instances: torch.Tensor, instance_ids: torch.Tensor, n_sample: int, seed: int, map_size: int = 65536):
    """instances i32[Npts] (instance id per scene point), instance_ids i32[N] (distinct) -> choice i32[N, n_sample] (indices into the
    scene's points, drawn with replacement from each instance's own points), counts i32[N] (points per instance).  Device tensors
    in and out; nothing is read back.  ``choice`` feeds ``prepare_objects``.  ``map_size`` bounds the instance ids the kernel can
    see: a requested id >= map_size gets count 0 and choice 0, and of two equal ids only one gets points -- callers that hold the
    ids on the host (``scan.prepare_scan``) check both and size the map from the largest id."""
    lib = L.load()
    dev = instances.device
    instances = instances.to(torch.int32).contiguous().view(-1)
    ids = instance_ids.to(device=dev, dtype=torch.int32).contiguous().view(-1)
    n_pts, n = instances.numel(), ids.numel()
    map_size = int(map_size)              # instance ids are small integers (3RScan: < 1000)
    if map_size <= 0:
        raise L.VlsatError("sample_objects: map_size must be positive")
    id_map = torch.empty(map_size, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib.vlsat_sample_objects_scratch(n_pts, n)), dtype=torch.int32, device=dev)
    choice = torch.empty(n, int(n_sample), dtype=torch.int32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    L.check(lib.vlsat_sample_objects(instances.data_ptr(), n_pts, ids.data_ptr(), n, int(n_sample), int(seed) & (2 ** 64 - 1), id_map.data_ptr(),
                                     map_size, scratch.data_ptr(), choice.data_ptr(), counts.data_ptr(), L.stream_ptr()))
    return choice, counts


def prepare_objects(scene_points: torch.Tensor, choice: torch.Tensor):
    """scene_points f32[Npts,3], choice i32[N,P] (device) -> obj_points f32[N,3,P], descriptor f32[N,11]."""
    lib = L.load()
    scene_points = scene_points.contiguous()
    choice = choice.to(torch.int32).contiguous()
    if scene_points.dim() != 2 or scene_points.shape[1] != 3 or scene_points.dtype != torch.float32:
        raise L.VlsatError("scene_points must be float32 [Npts,3]")
    n, p = choice.shape
    pts = torch.empty(n, 3, p, dtype=torch.float32, device=scene_points.device)
    desc = torch.empty(n, 11, dtype=torch.float32, device=scene_points.device)
    L.check(lib.vlsat_prepare_objects(scene_points.data_ptr(), choice.data_ptr(), n, p, pts.data_ptr(), desc.data_ptr(),
                                      L.stream_ptr()))
    return pts, desc


def fc_edges(n_per_scene: Sequence[int], device) -> tuple:
    """-> edge_indices i64[2,E] (what Mmgnet.forward takes), batch_ids i64[N,1]."""
    lib = L.load()
    n = torch.tensor([0] + list(n_per_scene), dtype=torch.int64)
    node_ptr = torch.cumsum(n, 0)
    edge_ptr = torch.cumsum(n * (n - 1), 0)
    N, E, S = int(node_ptr[-1]), int(edge_ptr[-1]), len(n_per_scene)
    d_node, d_edge = node_ptr.to(torch.int32).to(device), edge_ptr.to(device)
    edges = torch.empty(2, E, dtype=torch.int64, device=device)
    bids = torch.empty(N, 1, dtype=torch.int64, device=device)
    L.check(lib.vlsat_fc_edges(d_node.data_ptr(), d_edge.data_ptr(), S, N, E, edges.data_ptr(), bids.data_ptr(),
                               L.stream_ptr()))
    return edges, bids


# ---- proximity-pruned edge lists (csrc/proximity.hip; the rule is stated in include/vlsat.h) -------------------------------------------
def proximity_lds_boxes() -> int:
    """Boxes a block of the proximity kernels stages in LDS; spans above it are read from global memory (same result)."""
    return int(L.load().vlsat_proximity_lds_boxes())


def instance_boxes(scene_points: torch.Tensor, instances: torch.Tensor, instance_ids: torch.Tensor, map_size: int = 65536) -> torch.Tensor:
    """scene_points f32[Npts,3], instances i32[Npts], instance_ids i32[N] (distinct, each < map_size) -> boxes f32[N,6] = lo.xyz,
    hi.xyz over ALL points of each instance (unpadded; the reference's ``instances_box`` is this box -/+ 0.2,
    dataset_3dssg.py:286-288).  An id without points gets lo = +inf, hi = -inf.  Device tensors in and out, nothing is read back."""
    lib = L.load()
    scene_points = scene_points.contiguous()
    if scene_points.dim() != 2 or scene_points.shape[1] != 3 or scene_points.dtype != torch.float32:
        raise L.VlsatError("scene_points must be float32 [Npts,3]")
    dev = scene_points.device
    instances = instances.to(device=dev, dtype=torch.int32).contiguous().view(-1)
    if instances.numel() != scene_points.shape[0]:
        raise L.VlsatError("instance_boxes: one instance id per scene point")
    ids = instance_ids.to(device=dev, dtype=torch.int32).contiguous().view(-1)
    map_size = int(map_size)
    if map_size <= 0:
        raise L.VlsatError("instance_boxes: map_size must be positive")
    id_map = torch.empty(map_size, dtype=torch.int32, device=dev)
    boxes = torch.empty(ids.numel(), 6, dtype=torch.float32, device=dev)
    L.check(lib.vlsat_instance_boxes(instances.data_ptr(), scene_points.data_ptr(), instances.numel(), ids.data_ptr(), ids.numel(),
                                     id_map.data_ptr(), map_size, boxes.data_ptr(), L.stream_ptr()))
    return boxes


def proximity_edges_host(boxes, n_per_scene: Sequence[int], padding: float = 0.2, max_neighbors: int = 0):
    """The rule of ``proximity_edges`` in numpy, in the same fp32 operations (every one rounded on its own, so the distances are the
    device's bit for bit) -> (edge_indices i64[2,E], batch_ids i64[N,1], edge_ptr i64[S+1]) as numpy arrays."""
    import numpy as np

    boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32)).reshape(-1, 6)
    n_per_scene = [int(n) for n in n_per_scene]
    if sum(n_per_scene) != len(boxes) or min(n_per_scene, default=0) < 0:
        raise L.VlsatError("proximity_edges: n_per_scene does not add up to the number of boxes")
    pad = np.float32(padding)
    if not pad >= 0:
        raise L.VlsatError("proximity_edges: padding must be >= 0")
    k_cap = int(max_neighbors)
    all_keys = np.uint64(0xFFFFFFFFFFFFFFFF)
    src, dst, bids, edge_ptr, off = [], [], [], [0], 0
    for s, n in enumerate(n_per_scene):
        lo, hi = boxes[off:off + n, :3], boxes[off:off + n, 3:]
        with np.errstate(over="ignore", invalid="ignore"):
            lo_p, hi_p = lo - pad, hi + pad
            cand = (lo_p[:, None, :] < hi_p[None, :, :]).all(-1)
            cand = cand & cand.T & ~np.eye(n, dtype=bool)
            emit = cand
            if k_cap > 0 and n > 0:
                g = np.maximum(np.float32(0), np.maximum(lo[:, None, :] - hi[None, :, :], lo[None, :, :] - hi[:, None, :]))
                g = np.where(cand[:, :, None], g, np.float32(0))           # (empty boxes give inf - inf off the candidate set)
                d = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
                key = (np.ascontiguousarray(d, dtype=np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
                key = np.where(cand, key, all_keys)
                thr = np.sort(key, axis=1)[:, k_cap - 1] if k_cap <= n else np.full(n, all_keys)     # all ones: fewer candidates than the cap
                keep = key <= thr[:, None]
                emit = cand & (keep | keep.T)
        i, j = np.nonzero(emit)                                             # row-major: source-major, targets ascending
        src.append(i.astype(np.int64) + off)
        dst.append(j.astype(np.int64) + off)
        bids.append(np.full((n, 1), s, dtype=np.int64))
        edge_ptr.append(edge_ptr[-1] + len(i))
        off += n
    cat = lambda xs, shape: np.concatenate(xs, 0) if xs else np.zeros(shape, dtype=np.int64)   # noqa: E731
    return np.stack([cat(src, (0,)), cat(dst, (0,))], 0), cat(bids, (0, 1)), np.asarray(edge_ptr, dtype=np.int64)


def proximity_edges(boxes, n_per_scene: Sequence[int], padding: float = 0.2, max_neighbors: int = 0):
    """boxes f32[N,6] (``instance_boxes``), nodes per scene -> (edge_indices i64[2,E], batch_ids i64[N,1], edge_ptr i64[S+1]).

    Edge (i, j) iff i != j are in one scene, their boxes padded by ``padding`` intersect strictly on all three axes, and -- with
    ``max_neighbors > 0`` -- j is among i's ``max_neighbors`` nearest candidates OR i among j's (squared box gap in fp32, ties to the
    lower index).  The list is symmetric, so a node's out-degree can exceed ``max_neighbors``; per scene E <= min(n(n-1), 2 n
    max_neighbors).  Order: the fully connected order of ``fc_edges`` with the dropped pairs removed.  A device tensor runs the HIP
    kernels (one host wait: the edge total is read to size the list); a CPU tensor or an array runs ``proximity_edges_host``."""
    if not (isinstance(boxes, torch.Tensor) and boxes.is_cuda):
        e, b, p = proximity_edges_host(boxes.numpy() if isinstance(boxes, torch.Tensor) else boxes, n_per_scene, padding, max_neighbors)
        return torch.from_numpy(e), torch.from_numpy(b), torch.from_numpy(p)
    lib = L.load()
    dev = boxes.device
    boxes = boxes.contiguous()
    if boxes.dim() != 2 or boxes.shape[1] != 6 or boxes.dtype != torch.float32:
        raise L.VlsatError("boxes must be float32 [N,6]")
    n = torch.tensor([0] + [int(v) for v in n_per_scene], dtype=torch.int64)
    node_ptr = torch.cumsum(n, 0)
    N, S = int(node_ptr[-1]), len(n_per_scene)
    if N != boxes.shape[0] or S == 0 or int(n.min()) < 0:
        raise L.VlsatError("proximity_edges: n_per_scene does not add up to the number of boxes")
    if not float(padding) >= 0:
        raise L.VlsatError("proximity_edges: padding must be >= 0")
    d_node = node_ptr.to(torch.int32).to(dev)
    scratch = torch.empty(int(lib.vlsat_proximity_scratch_bytes(N)), dtype=torch.uint8, device=dev)
    edge_ptr = torch.empty(S + 1, dtype=torch.int64, device=dev)
    bids = torch.empty(N, 1, dtype=torch.int64, device=dev)
    L.check(lib.vlsat_proximity_count(boxes.data_ptr(), d_node.data_ptr(), S, N, float(padding), int(max_neighbors), scratch.data_ptr(),
                                      edge_ptr.data_ptr(), bids.data_ptr(), L.stream_ptr()))
    E = int(edge_ptr[S])                     # the one host wait: the list is sized from the device's count
    edges = torch.empty(2, E, dtype=torch.int64, device=dev)
    L.check(lib.vlsat_proximity_fill(boxes.data_ptr(), d_node.data_ptr(), S, N, float(padding), int(max_neighbors), scratch.data_ptr(),
                                     E, E, edges.data_ptr(), L.stream_ptr()))
    return edges, bids, edge_ptr


# ---- annotation transfer onto a predicted segmentation (csrc/label_transfer.hip; the rule is stated in include/vlsat.h) ----------------
def nearest_points_host(query, ref, max_sq_dist: float, chunk: int = 256):
    """The rule of ``nearest_points`` in numpy, in the same fp32 operations (so every index and distance bit is the device's) ->
    (nn_index i32[Q], nn_sqdist f32[Q]).  A sweep along x instead of the device's grid: the queries go in x order, a chunk at a time,
    against the annotated points whose x lies within sqrt(max_sq_dist) of the chunk's (only those can have d2 <= max_sq_dist); the
    answer is the minimum of the key (bits(d2) << 32) | index, which does not depend on how the candidates were found."""
    import numpy as np

    q = np.ascontiguousarray(np.asarray(query, dtype=np.float32)).reshape(-1, 3)
    r = np.ascontiguousarray(np.asarray(ref, dtype=np.float32)).reshape(-1, 3)
    m = np.float32(max_sq_dist)
    if not m >= 0:
        raise L.VlsatError("nearest_points: max_sq_dist must be >= 0 (it is a squared distance)")
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    best = np.full(len(q), none, dtype=np.uint64)
    r_idx = np.nonzero(np.isfinite(r).all(1))[0]
    q_idx = np.nonzero(np.isfinite(q).all(1))[0]
    if len(r_idx) and len(q_idx):
        r_idx = r_idx[np.argsort(r[r_idx, 0], kind="stable")]
        rs, rx = r[r_idx], r[r_idx, 0].astype(np.float64)
        q_idx = q_idx[np.argsort(q[q_idx, 0], kind="stable")]
        # |q.x - r.x| of a pair with d2 <= m: the rounded dx dx is at most d2, the difference and the product are off by 2^-24 each,
        # and a product that underflows to zero belongs to a |dx| below 2^-74
        w = float(np.sqrt(np.float64(m))) * (1.0 + 2.0 ** -20) + 1e-20 if np.isfinite(m) else np.inf
        with np.errstate(over="ignore", invalid="ignore"):
            for c0 in range(0, len(q_idx), chunk):
                qi = q_idx[c0:c0 + chunk]
                qc = q[qi]
                a = np.searchsorted(rx, float(qc[0, 0]) - w, "left")
                b = np.searchsorted(rx, float(qc[-1, 0]) + w, "right")
                acc = np.full(len(qi), none, dtype=np.uint64)
                for p0 in range(a, b, 16384):
                    rp, ri = rs[p0:min(p0 + 16384, b)], r_idx[p0:min(p0 + 16384, b)]
                    dx, dy, dz = (qc[:, None, k] - rp[None, :, k] for k in range(3))
                    d2 = (dx * dx + dy * dy) + dz * dz
                    key = (np.ascontiguousarray(d2).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ri.astype(np.uint64)[None, :]
                    acc = np.minimum(acc, np.where(d2 <= m, key, none).min(1))
                best[qi] = acc
    found = best != none
    nn_index = np.where(found, best & np.uint64(0xFFFFFFFF), 0).astype(np.int64).astype(np.int32)
    nn_index[~found] = -1
    nn_sqdist = np.where(found, (best >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf)).astype(np.float32)
    return nn_index, nn_sqdist


def nearest_points(query, ref, max_sq_dist: float):
    """query f32[Q,3] (the predicted cloud), ref f32[G,3] (the annotated cloud) -> (nn_index i32[Q], nn_sqdist f32[Q]): per query the
    annotated point with the smallest ``d2 = (dx*dx + dy*dy) + dz*dz`` (fp32, every operation rounded on its own; ties to the lower
    index) among those with ``d2 <= max_sq_dist``, else -1 and +inf.

    ``max_sq_dist`` is a SQUARED distance: the reference compares Open3D's squared distance with its ``--max_dist`` (default 0.1;
    data_processing/gen_data.py:268-269), so 0.1 means 0.316 in the units of the cloud.  Non-finite queries have no correspondence and
    non-finite annotated points are never returned.  Exact and deterministic.  Device tensors run the HIP kernels (nothing is read
    back); CPU tensors or arrays run ``nearest_points_host``."""
    if not (isinstance(query, torch.Tensor) and query.is_cuda):
        as_np = lambda x: x.numpy() if isinstance(x, torch.Tensor) else x   # noqa: E731
        i, d = nearest_points_host(as_np(query), as_np(ref), max_sq_dist)
        return torch.from_numpy(i), torch.from_numpy(d)
    lib = L.load()
    dev = query.device
    query = query.contiguous()
    ref = ref.to(dev).contiguous()
    for name, t in (("query", query), ("ref", ref)):
        if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
            raise L.VlsatError(f"nearest_points: {name} must be float32 [n,3]")
    if not float(max_sq_dist) >= 0:
        raise L.VlsatError("nearest_points: max_sq_dist must be >= 0 (it is a squared distance)")
    Q, G = query.shape[0], ref.shape[0]
    scratch = torch.empty(int(lib.vlsat_nearest_points_scratch_bytes(Q, G)), dtype=torch.uint8, device=dev)
    nn_index = torch.empty(Q, dtype=torch.int32, device=dev)
    nn_sqdist = torch.empty(Q, dtype=torch.float32, device=dev)
    L.check(lib.vlsat_nearest_points(query.data_ptr(), Q, ref.data_ptr(), G, float(max_sq_dist), scratch.data_ptr(), nn_index.data_ptr(),
                                     nn_sqdist.data_ptr(), L.stream_ptr()))
    return nn_index, nn_sqdist


def _overlap_ids(segment_ids, gt_ids):
    import numpy as np

    seg_ids = np.asarray(segment_ids, dtype=np.int64).reshape(-1)
    g_ids = np.asarray(gt_ids, dtype=np.int64).reshape(-1)
    for name, ids in (("segment_ids", seg_ids), ("gt_ids", g_ids)):
        if len(ids) and (len(np.unique(ids)) != len(ids) or ids.min() < 0 or ids.max() >= (1 << 24)):
            raise L.VlsatError(f"segment_overlap: {name} must be distinct integers in [0, 2^24)")
    return seg_ids, g_ids


def segment_overlap_host(pd_segments, nn_index, gt_instances, segment_ids, gt_ids, min_seg_size: int = 512, corr_thres: float = 0.5,
                         occ_thres: float = 0.75, occ_min_candidates: int = 3) -> dict:
    """The rule of ``segment_overlap`` in numpy and Python floats (fp64, the reference's own divisions) -> the same dict of numpy
    arrays."""
    import numpy as np

    seg_ids, g_ids = _overlap_ids(segment_ids, gt_ids)
    seg = np.asarray(pd_segments, dtype=np.int64).reshape(-1)
    nn = np.asarray(nn_index, dtype=np.int64).reshape(-1)
    inst = np.asarray(gt_instances, dtype=np.int64).reshape(-1)
    if len(seg) != len(nn):
        raise L.VlsatError("segment_overlap: one nearest index per predicted point")
    if corr_thres != corr_thres or occ_thres != occ_thres:
        raise L.VlsatError("segment_overlap: a threshold is NaN")
    S, n_gt = len(seg_ids), len(g_ids)

    def slots(values, ids):                          # slot of every value in ids, -1 when absent
        if not len(ids):
            return np.full(len(values), -1, dtype=np.int64)
        order = np.argsort(ids)
        pos = np.minimum(np.searchsorted(ids[order], values), len(ids) - 1)
        return np.where(ids[order][pos] == values, order[pos], -1)

    s_slot = slots(seg, seg_ids)
    size = np.bincount(s_slot[s_slot >= 0], minlength=S).astype(np.int32)
    has = (s_slot >= 0) & (nn >= 0) & (nn < len(inst))
    g_slot = slots(inst[nn[has]], g_ids)
    flat = s_slot[has][g_slot >= 0] * n_gt + g_slot[g_slot >= 0]
    counts = np.bincount(flat, minlength=S * n_gt).astype(np.int32).reshape(S, n_gt)
    match, best, second, n_cand = (np.full(S, v, dtype=np.int32) for v in (-1, 0, 0, 0))
    for s in range(S):
        c = counts[s]
        n_cand[s] = int((c > 0).sum())
        if not n_cand[s]:
            continue
        j = int(np.lexsort((g_ids, -c.astype(np.int64)))[0])       # the largest count, ties to the lower instance id
        best[s], second[s] = c[j], np.delete(c, j).max(initial=0)
        if size[s] > min_seg_size:
            r1, r2 = float(best[s]) / float(size[s]), float(second[s]) / float(size[s])
            occ = r2 / r1 if n_cand[s] >= occ_min_candidates else 0.0
            if r1 > corr_thres and occ < occ_thres:
                match[s] = j
    return {"size": size, "counts": counts, "match": match, "best": best, "second": second, "n_candidates": n_cand}


def segment_overlap(pd_segments, nn_index, gt_instances, segment_ids, gt_ids, min_seg_size: int = 512, corr_thres: float = 0.5,
                    occ_thres: float = 0.75, occ_min_candidates: int = 3) -> dict:
    """pd_segments i32[Q] (segment id per predicted point), nn_index i32[Q] (``nearest_points``), gt_instances i32[G] (instance id per
    annotated point), segment_ids (the segments to consider: host sequence, distinct) and gt_ids (the label-eligible instances: those
    with a label other than 'none'; host sequence, distinct) -> dict of ``size`` i32[S] (ALL points of a segment), ``counts``
    i32[S, n_gt] (its points whose nearest annotated point belongs to the instance), ``match`` i32[S] (slot in ``gt_ids`` of the
    accepted instance, or -1), ``best`` / ``second`` i32[S] (the largest count and the largest among the other instances) and
    ``n_candidates`` i32[S] (instances with a non-zero count).

    Accepted iff ``size > min_seg_size`` and ``best / size > corr_thres`` and ``occ < occ_thres``, all strict and in fp64, where
    ``occ = second / best`` (as the ratio of the two ratios) when at least ``occ_min_candidates`` instances have a non-zero count and 0
    otherwise.  The default 3 reproduces the reference's ``len(list) > 2`` (gen_data.py:331), under which a segment shared 51 : 49 by
    exactly two instances is accepted; 2 is probably what was meant.  Device tensors run the HIP kernels (nothing is read back); CPU
    tensors or arrays run ``segment_overlap_host``."""
    if not (isinstance(pd_segments, torch.Tensor) and pd_segments.is_cuda):
        as_np = lambda x: x.numpy() if isinstance(x, torch.Tensor) else x   # noqa: E731
        out = segment_overlap_host(as_np(pd_segments), as_np(nn_index), as_np(gt_instances), segment_ids, gt_ids, min_seg_size, corr_thres,
                                   occ_thres, occ_min_candidates)
        return {k: torch.from_numpy(v) for k, v in out.items()}
    lib = L.load()
    dev = pd_segments.device
    seg_ids, g_ids = _overlap_ids(segment_ids, gt_ids)
    seg = pd_segments.to(torch.int32).contiguous().view(-1)
    nn = nn_index.to(device=dev, dtype=torch.int32).contiguous().view(-1)
    inst = gt_instances.to(device=dev, dtype=torch.int32).contiguous().view(-1)
    if seg.numel() != nn.numel():
        raise L.VlsatError("segment_overlap: one nearest index per predicted point")
    S, n_gt = len(seg_ids), len(g_ids)
    if S * n_gt >= 1 << 31:
        raise L.VlsatError("segment_overlap: the table of counts has more than 2^31 - 1 entries")
    seg_map_size = max(65536, int(seg_ids.max(initial=0)) + 1)
    gt_map_size = max(65536, int(g_ids.max(initial=0)) + 1)
    d_seg_ids = torch.from_numpy(seg_ids.astype("int32")).to(dev)
    d_gt_ids = torch.from_numpy(g_ids.astype("int32")).to(dev)
    id_maps = torch.empty(int(lib.vlsat_segment_overlap_scratch_bytes(seg_map_size, gt_map_size)), dtype=torch.uint8, device=dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)   # noqa: E731
    out = {"size": i32(S), "counts": i32(S, n_gt), "match": i32(S), "best": i32(S), "second": i32(S), "n_candidates": i32(S)}
    L.check(lib.vlsat_segment_overlap(seg.data_ptr(), nn.data_ptr(), seg.numel(), inst.data_ptr(), inst.numel(), d_seg_ids.data_ptr(), S,
                                      d_gt_ids.data_ptr(), n_gt, id_maps.data_ptr(), seg_map_size, gt_map_size, int(min_seg_size),
                                      float(corr_thres), float(occ_thres), int(occ_min_candidates), out["size"].data_ptr(),
                                      out["counts"].data_ptr(), out["match"].data_ptr(), out["best"].data_ptr(), out["second"].data_ptr(),
                                      out["n_candidates"].data_ptr(), L.stream_ptr()))
    return out


# ---- a scan split into sub-scenes (csrc/scene_split.hip; the rules are stated in include/vlsat_split.h) --------------------------------
_M64 = (1 << 64) - 1


def split_draw(seed: int, k: int, n: int) -> int:
    """draw(k, n) of the split seeds: ``sample_objects``' counter-based generator -- splitmix64 of (seed, k), the top 32 bits scaled to n."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(k) + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return ((z >> 32) * int(n)) >> 32


def split_seed_cap(points, distance: float) -> int:
    """A bound on the number of seeds, from the xy bounding box of the finite vertices: two seeds are more than ``distance`` apart, so a
    cell of side distance / sqrt(2) holds at most one (one row and column of cells to spare for the rounding of the division).  ``points``:
    a host array [V,3]."""
    import math

    import numpy as np
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    xy = pts[np.isfinite(pts).all(1)][:, :2]
    if not distance > 0:
        raise L.VlsatError("split_seeds: distance must be positive")
    if not len(xy):
        return 1
    side = float(distance) / math.sqrt(2.0)
    ext = xy.max(0) - xy.min(0)
    cells = (int(ext[0] / side) + 2) * (int(ext[1] / side) + 2)
    return int(max(1, min(cells, len(pts))))


_SEED_ERRORS = {1: "split_seeds: a rank is negative or not below the number of selectable vertices",
                2: "split_seeds: the ranks ran out while vertices were still selectable",
                3: "split_seeds: max_seeds reached while vertices were still selectable"}


def _seed_args(points, distance, ranks):
    import numpy as np
    if tuple(points.shape[1:]) != (3,) or len(points.shape) != 2 or points.shape[0] < 1:
        raise L.VlsatError("split_seeds: points must be float32 [V,3] with V >= 1")
    distance = float(distance)
    if not 0.0 < distance < 1e150:
        raise L.VlsatError("split_seeds: distance must be positive and finite")
    if ranks is not None:
        ranks = np.asarray(ranks.cpu() if torch.is_tensor(ranks) else ranks, dtype=np.int64).reshape(-1)
    return distance, ranks


def split_seeds_host(points, distance: float = 1.0, seed: int = 0, ranks=None):
    """The seed rule of include/vlsat_split.h (vlsat_split_seeds; reference gen_data.py:69-85) in numpy, in the device's fp64 operations
    -> seed indices int32 [K] in creation order (numpy).  ``ranks``: the draws of a recorded run (rank of each seed among the
    selectable vertices); a rank out of range, or ranks running out early, raises."""
    import numpy as np
    pts = np.ascontiguousarray(points.cpu().numpy() if torch.is_tensor(points) else points, dtype=np.float32)
    distance, ranks = _seed_args(pts, distance, ranks)
    v = pts.shape[0]
    d2_max = distance * distance

    def draw(k, n):
        if ranks is None:
            return split_draw(seed, k, n)
        if k >= len(ranks):
            raise L.VlsatError(_SEED_ERRORS[2])
        if not 0 <= int(ranks[k]) < n:
            raise L.VlsatError(_SEED_ERRORS[1])
        return int(ranks[k])

    xy = pts[:, :2].astype(np.float64)
    finite = np.isfinite(pts).all(1)
    seeds = [draw(0, v)]
    dmin2 = None
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            dx, dy = xy[:, 0] - xy[seeds[-1], 0], xy[:, 1] - xy[seeds[-1], 1]
            d = dx * dx + dy * dy                                                  # (numpy rounds the products and the sum on their own)
            dmin2 = np.where(finite, d, np.nan) if dmin2 is None else np.where(d < dmin2, d, dmin2)
            selectable = np.nonzero(dmin2 > d2_max)[0]
            if not len(selectable):
                break
            seeds.append(int(selectable[draw(len(seeds), len(selectable))]))
    return np.asarray(seeds, dtype=np.int32)


def split_seeds(points: torch.Tensor, distance: float = 1.0, seed: int = 0, ranks=None, max_seeds: int | None = None) -> torch.Tensor:
    """points f32 [V,3] (device) -> the seed vertices of the scan's sub-scenes, int32 [K] in creation order (include/vlsat_split.h,
    vlsat_split_seeds): seed 0 is drawn among all vertices, every later one among the vertices more than ``distance`` away (in xy)
    from all seeds so far, until none is left.  The draws come from ``sample_objects``' counter-based generator (``split_draw``), or
    from ``ranks``.  ``max_seeds`` bounds K (``split_seed_cap`` of the host copy of the points; None: computed here, which reads the
    points back).  One short launch chain per seed is enqueued up to that bound and the chain ends itself on the device; the ONE
    host wait is reading K back.  CPU tensors: ``split_seeds_host``."""
    if not points.is_cuda:
        return torch.from_numpy(split_seeds_host(points, distance, seed, ranks))
    lib = L.load()
    if points.dtype != torch.float32:
        raise L.VlsatError("split_seeds: points must be float32 [V,3]")
    points = points.contiguous()
    distance, ranks = _seed_args(points, distance, ranks)
    dev = points.device
    v = points.shape[0]
    cap = split_seed_cap(points.cpu().numpy(), distance) if max_seeds is None else int(max_seeds)
    if not 1 <= cap <= 65536:
        raise L.VlsatError("split_seeds: more than 65536 possible seeds: distance is too small for this extent")
    d_ranks = None if ranks is None else torch.from_numpy(ranks).to(dev)
    scratch = torch.empty(int(lib.vlsat_split_seeds_scratch_bytes(v)), dtype=torch.uint8, device=dev)
    seeds = torch.empty(cap, dtype=torch.int32, device=dev)
    state = torch.empty(4, dtype=torch.int32, device=dev)
    L.check(lib.vlsat_split_seeds(points.data_ptr(), v, distance, int(seed) & _M64, L.ptr(d_ranks), 0 if ranks is None else len(ranks), cap,
                                  scratch.data_ptr(), seeds.data_ptr(), state.data_ptr(), L.stream_ptr()))
    k, status, done, _ = state.tolist()                                            # the one host wait
    if status or not done:
        raise L.VlsatError(_SEED_ERRORS[status or 3])
    return seeds[:k]


def _group_args(points, segments, segment_ids, seeds):
    import numpy as np
    ids = np.asarray(segment_ids.cpu() if torch.is_tensor(segment_ids) else segment_ids, dtype=np.int64).reshape(-1)
    if len(ids) and (ids.min() < 0 or ids.max() >= (1 << 24) or len(np.unique(ids)) != len(ids)):
        raise L.VlsatError("split_groups: segment_ids must be distinct integers in [0, 2^24)")
    if len(points.shape) != 2 or points.shape[1] != 3 or segments.shape[0] != points.shape[0]:
        raise L.VlsatError("split_groups: points must be float32 [V,3] with one segment id per vertex")
    return ids


def _unpack_groups(ids, mask, counts, keep):
    import numpy as np
    s = len(ids)
    if not s:
        return [[] for _ in range(len(mask))], np.asarray(counts, dtype=np.int32), np.asarray(keep, dtype=bool)
    bits = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8).reshape(len(mask), -1), axis=1, bitorder="little")[:, :s].astype(bool)
    order = np.argsort(ids, kind="stable")
    groups = [[int(i) for i in ids[order][bits[k][order]]] for k in range(len(mask))]
    return groups, np.asarray(counts, dtype=np.int32), np.asarray(keep, dtype=bool)


def split_groups_host(points, segments, segment_ids, seeds, bbox_distance: float = 0.75, min_seg_per_group: int = 5):
    """The group rule of include/vlsat_split.h (vlsat_split_groups; reference gen_data.py:109-122) in numpy fp64 -> (groups, counts,
    keep, mask): per seed the ascending ids of the segments with a vertex strictly inside the seed's box, their number,
    ``counts >= min_seg_per_group``, and the bit table uint32 [K, ceil(S/32)] over the slots of ``segment_ids``."""
    import numpy as np
    pts = np.ascontiguousarray(points.cpu().numpy() if torch.is_tensor(points) else points, dtype=np.float32)
    seg = np.asarray(segments.cpu() if torch.is_tensor(segments) else segments).astype(np.int64).reshape(-1)
    seeds = np.asarray(seeds.cpu() if torch.is_tensor(seeds) else seeds, dtype=np.int64).reshape(-1)
    ids = _group_args(pts, seg, segment_ids, seeds)
    if len(seeds) and (seeds.min() < 0 or seeds.max() >= len(pts)):
        raise L.VlsatError("split_groups: a seed is not a vertex index")
    s, k = len(ids), len(seeds)
    words = (s + 31) // 32
    slot_of = {int(i): n for n, i in enumerate(ids)}
    slot = np.asarray([slot_of.get(int(i), -1) for i in seg], dtype=np.int64)
    p64 = pts.astype(np.float64)
    hit = np.zeros((k, words * 32), dtype=bool)
    with np.errstate(invalid="ignore"):
        for n, sv in enumerate(seeds):
            lo, hi = p64[sv] - float(bbox_distance), p64[sv] + float(bbox_distance)
            inside = ((p64 > lo) & (p64 < hi)).all(1) & (slot >= 0)
            hit[n, slot[inside]] = True
    mask = np.packbits(hit, axis=1, bitorder="little").view(np.uint32).reshape(k, words) if words else np.zeros((k, 0), np.uint32)
    counts = hit.sum(1).astype(np.int32)
    return (*_unpack_groups(ids, mask, counts, counts >= int(min_seg_per_group)), mask)


def split_groups(points: torch.Tensor, segments: torch.Tensor, segment_ids, seeds: torch.Tensor, bbox_distance: float = 0.75,
                 min_seg_per_group: int = 5, map_size: int = 65536):
    """points f32 [V,3], segments int32 [V] (device), ``segment_ids`` (distinct, on the host or the device), seeds int32 [K] -> (groups,
    counts, keep, mask) as ``split_groups_host``: group k = the ascending ids of the segments with a vertex strictly inside the box
    ``seed point -/+ bbox_distance`` (include/vlsat_split.h, vlsat_split_groups); ``keep`` marks the groups the reference keeps.  Id 0
    counts when it is listed, as the reference's np.unique counts it.  The bit table is read back ONCE.  CPU tensors: the host rule."""
    import numpy as np
    if not points.is_cuda:
        return split_groups_host(points, segments, segment_ids, seeds, bbox_distance, min_seg_per_group)
    lib = L.load()
    if points.dtype != torch.float32:
        raise L.VlsatError("split_groups: points must be float32 [V,3]")
    points = points.contiguous()
    dev = points.device
    segments = segments.to(device=dev, dtype=torch.int32).contiguous().view(-1)
    ids = _group_args(points, segments, segment_ids, seeds)
    seeds = seeds.to(device=dev, dtype=torch.int32).contiguous().view(-1) if torch.is_tensor(seeds) else torch.tensor(
        np.asarray(seeds, dtype=np.int32).reshape(-1), dtype=torch.int32, device=dev)
    s, k = len(ids), seeds.numel()
    words = (s + 31) // 32
    map_size = max(int(map_size), int(ids.max()) + 1 if s else 1)
    d_ids = torch.from_numpy(ids.astype(np.int32)).to(dev)
    id_map = torch.empty(map_size, dtype=torch.int32, device=dev)
    out = torch.empty(k * words + 2 * k, dtype=torch.int32, device=dev)           # mask | counts | keep: one read-back
    mask, counts, keep = out[:k * words], out[k * words:k * words + k], out[k * words + k:]
    L.check(lib.vlsat_split_groups(points.data_ptr(), segments.data_ptr(), points.shape[0], d_ids.data_ptr(), s, id_map.data_ptr(), map_size,
                                   seeds.data_ptr(), k, float(bbox_distance), int(min_seg_per_group), mask.data_ptr(), counts.data_ptr(),
                                   keep.data_ptr(), L.stream_ptr()))
    host = out.cpu().numpy()                                                      # the one host wait
    mask = host[:k * words].view(np.uint32).reshape(k, words)
    return (*_unpack_groups(ids, mask, host[k * words:k * words + k], host[k * words + k:]), mask)


# ---- an unlabelled mesh over-segmented into segments (csrc/mesh_segment.hip; the rule is stated in include/vlsat_segment.h) -------------
SEG_MAX_VERTS = 1 << 24


class MeshSegments:
    """What ``segment_mesh`` found: ``labels`` int32 [V] (0 = dropped, else 1..S in the order of a segment's lowest vertex),
    ``n_segments`` (an int when trimmed, else an int32 tensor [1] on the labels' device) and ``seg_size`` int32 ([S] when trimmed, else
    [V] with zeros past S).  ``trimmed`` as in ``metrics.MergedGraph``."""
    __slots__ = ("labels", "n_segments", "seg_size", "trimmed")

    def __init__(self, labels, n_segments, seg_size, trimmed=False):
        self.labels, self.n_segments, self.seg_size, self.trimmed = labels, n_segments, seg_size, bool(trimmed)

    def trim(self) -> "MeshSegments":
        """``seg_size`` cut to S entries.  Reads ``n_segments`` back: ONE host synchronisation."""
        if self.trimmed:
            return self
        s = int(self.n_segments.reshape(-1)[0])
        return MeshSegments(self.labels, s, self.seg_size[:s], True)

    def __iter__(self):                      # labels, n_segments, seg_size = segment_mesh(...)
        return iter((self.labels, self.n_segments, self.seg_size))

    def __repr__(self):
        return f"MeshSegments({int(self.labels.shape[0])} vertices, {self.n_segments if self.trimmed else '?'} segments)"


def mesh_edges(faces):
    """faces int [F,3] -> the three sides of every triangle, int32 [3 F, 2], in the faces' order: (v0, v1), (v1, v2), (v2, v0).  A
    tensor in, a tensor on its device out; anything else goes through numpy.  Shared sides appear twice: the rule ignores duplicates."""
    import numpy as np
    if torch.is_tensor(faces):
        if faces.dim() != 2 or faces.shape[1] != 3:
            raise L.VlsatError("mesh_edges: faces must be [F,3]")
        return faces.to(torch.int32)[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2).contiguous()
    faces = np.asarray(faces)
    if faces.ndim != 2 or faces.shape[1] != 3:
        raise L.VlsatError("mesh_edges: faces must be [F,3]")
    return np.ascontiguousarray(faces.astype(np.int32)[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2))


def segment_rounds(min_verts: int) -> int:
    """ceil(log2(min_verts)), 0 for min_verts <= 1: the absorb rounds of include/vlsat_segment.h (csrc/segment_core.h: seg_rounds)."""
    r = 0
    while (1 << r) < int(min_verts):
        r += 1
    return r


def _segment_args(normals, edges, max_weight, min_verts):
    import math
    if len(normals.shape) != 2 or normals.shape[1] != 3 or not 1 <= normals.shape[0] <= SEG_MAX_VERTS:
        raise L.VlsatError("segment_mesh: normals must be float32 [V,3] with 1 <= V <= 2^24")
    if len(edges.shape) != 2 or edges.shape[1] != 2 or edges.shape[0] >= 1 << 31:
        raise L.VlsatError("segment_mesh: edges must be int32 [M,2] with M < 2^31")
    if math.isnan(float(max_weight)):
        raise L.VlsatError("segment_mesh: max_weight is NaN")
    if not -(1 << 31) <= int(min_verts) < 1 << 31:
        raise L.VlsatError("segment_mesh: min_verts must fit an int32")


def _seg_unite(parent, a, b):
    """Union-find on numpy arrays: the pairs (a[i], b[i]) united, every tree left flat with its LOWEST member as root.  Each pass
    hooks every root that still has a pair to another tree under the lowest root it sees (np.minimum.at: a set operation) and jumps
    pointers until flat; the number of trees with such a pair at least halves per pass."""
    import numpy as np
    while len(a):
        ra, rb = parent[a], parent[b]
        live = ra != rb
        if not live.any():
            break
        a, b, ra, rb = a[live], b[live], ra[live], rb[live]
        low = np.minimum(ra, rb)
        np.minimum.at(parent, ra, low)
        np.minimum.at(parent, rb, low)
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent[:] = up
    return parent


def segment_weights_host(normals, a, b, unsigned: bool = False):
    """w of include/vlsat_segment.h for the vertex pairs (a[i], b[i]) in numpy float32: every product and sum rounded on its own.
    ``unsigned``: the weight of include/vlsat_cloud.h for normals without a meaningful sign, 1 - |d|."""
    import numpy as np
    n = np.ascontiguousarray(normals, dtype=np.float32)
    na, nb = n[a], n[b]
    with np.errstate(invalid="ignore", over="ignore"):
        d = (na[:, 0] * nb[:, 0] + na[:, 1] * nb[:, 1]) + na[:, 2] * nb[:, 2]
        w = np.float32(1.0) - (np.abs(d) if unsigned else d)
        w = np.where(w < 0, np.float32(0.0), np.where(w > 2, np.float32(2.0), w)).astype(np.float32)
    return np.where(np.isnan(d), np.float32(2.0), w).astype(np.float32)


def segment_mesh_host(normals, edges, max_weight: float, min_verts: int = 20, trim: bool = True, unsigned: bool = False) -> MeshSegments:
    """``segment_mesh`` stated in numpy with the kernels' operations: the rule of include/vlsat_segment.h, step by step -- equal labels,
    count and sizes.  ``unsigned`` selects the weight 1 - |d| of include/vlsat_cloud.h.  Returns CPU tensors."""
    import numpy as np
    n = np.ascontiguousarray(normals.cpu().numpy() if torch.is_tensor(normals) else normals, dtype=np.float32)
    e = np.asarray(edges.cpu().numpy() if torch.is_tensor(edges) else edges).astype(np.int64)
    e = e.reshape(0, 2) if e.size == 0 else e
    _segment_args(n, e, max_weight, min_verts)
    v, min_verts, max_weight = n.shape[0], int(min_verts), np.float32(max_weight)
    ok = (e >= 0).all(1) & (e < v).all(1) & (e[:, 0] != e[:, 1])
    a, b = e[ok, 0], e[ok, 1]
    w = segment_weights_host(n, a, b, unsigned)
    parent = np.arange(v, dtype=np.int64)
    link = w <= max_weight
    _seg_unite(parent, a[link], b[link])                                           # step 2; parent is flat: parent[x] = root(x)
    a2, b2 = np.concatenate([a, b]), np.concatenate([b, a])                        # both directions of every edge
    bits = np.concatenate([w, w]).view(np.uint32).astype(np.uint64) << np.uint64(32)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    for _ in range(segment_rounds(min_verts) if len(a) else 0):                    # step 3
        size = np.bincount(parent, minlength=v)
        ra, rb = parent[a2], parent[b2]
        sel = (ra != rb) & (size[ra] < min_verts)
        best = np.full(v, none, dtype=np.uint64)
        np.minimum.at(best, ra[sel], bits[sel] | rb[sel].astype(np.uint64))
        src = np.nonzero(best != none)[0]
        _seg_unite(parent, src, (best[src] & np.uint64(0xFFFFFFFF)).astype(np.int64))
    size = np.bincount(parent, minlength=v)
    kept = (parent == np.arange(v)) & (size >= min_verts)                          # steps 4 and 5
    num = np.where(kept, np.cumsum(kept), 0)
    labels = num[parent].astype(np.int32)
    s = int(kept.sum())
    seg_size = np.zeros(v, dtype=np.int32)
    seg_size[:s] = size[kept]
    out = MeshSegments(torch.from_numpy(labels), torch.tensor([s], dtype=torch.int32), torch.from_numpy(seg_size))
    return out.trim() if trim else out


def segment_mesh(normals: torch.Tensor, edges: torch.Tensor, max_weight: float, min_verts: int = 20, trim: bool = True) -> MeshSegments:
    """normals f32 [V,3], edges int32 [M,2] (``mesh_edges(faces)``, or any undirected edge list: kNN edges for a cloud without faces)
    -> ``MeshSegments``: an over-segmentation by smoothness-constrained region growing (include/vlsat_segment.h, vlsat_segment_mesh).
    Edges whose normals agree (w = 1 - dot <= ``max_weight``) link their ends into components; in ceil(log2(min_verts)) rounds
    every component of fewer than ``min_verts`` vertices joins its neighbour across the lowest-weight edge (ties: the lower root); what
    is still smaller has no neighbour and gets label 0; the rest is numbered 1..S by lowest vertex.  Device tensors: the HIP kernels,
    asynchronous, 8 + 4 rounds launches and nothing read back to decide anything; ``trim=True`` then reads S back -- the ONE host
    synchronisation -- and cuts ``seg_size``, ``trim=False`` reads nothing.  CPU tensors: ``segment_mesh_host``."""
    if not normals.is_cuda:
        return segment_mesh_host(normals, edges, max_weight, min_verts, trim)
    lib = L.load()
    if normals.dtype != torch.float32:
        raise L.VlsatError("segment_mesh: normals must be float32 [V,3]")
    _segment_args(normals, edges, max_weight, min_verts)
    dev = normals.device
    normals = normals.contiguous()
    edges = edges.to(device=dev, dtype=torch.int32).contiguous()
    v, m = normals.shape[0], edges.shape[0]
    scratch = torch.empty(int(lib.vlsat_segment_mesh_scratch_bytes(v, m)), dtype=torch.uint8, device=dev)
    labels = torch.empty(v, dtype=torch.int32, device=dev)
    seg_size = torch.empty(v, dtype=torch.int32, device=dev)
    n_segments = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(lib.vlsat_segment_mesh(normals.data_ptr(), edges.data_ptr(), v, m, float(max_weight), int(min_verts), scratch.data_ptr(),
                                   labels.data_ptr(), n_segments.data_ptr(), seg_size.data_ptr(), L.stream_ptr()))
    out = MeshSegments(labels, n_segments, seg_size)
    return out.trim() if trim else out


# ---- a cloud without faces: kNN table, normals and flatness, segments (csrc/cloud.hip; the rules are stated in include/vlsat_cloud.h) ----
CLOUD_MAX_K = 32
CLOUD_SWEEPS = 6


class KnnTable(NamedTuple):
    """``knn_points``: ``index`` int32 [V,K] (-1 pads), ``sqdist`` f32 [V,K] (+inf pads), ``count`` int32 [V]."""
    index: object
    sqdist: object
    count: object


def _knn_args(shape, k, max_sq_dist):
    if len(shape) != 2 or shape[1] != 3 or not 1 <= shape[0] <= SEG_MAX_VERTS:
        raise L.VlsatError("knn_points: points must be float32 [V,3] with 1 <= V <= 2^24")
    if not 1 <= int(k) <= CLOUD_MAX_K:
        raise L.VlsatError("knn_points: 1 <= k <= 32")
    if not float(max_sq_dist) >= 0:
        raise L.VlsatError("knn_points: max_sq_dist must be >= 0 (it is a squared distance)")


def knn_points_host(points, k: int, max_sq_dist: float, chunk: int = 256) -> KnnTable:
    """The neighbour rule of include/vlsat_cloud.h in numpy, in the same fp32 operations (every index, distance bit and count is the
    device's) -> ``KnnTable`` of numpy arrays.  A sweep along x like ``nearest_points_host``: per chunk of points in x order, the keys
    (bits(d2) << 32) | j of the points within sqrt(max_sq_dist) in x, the point itself and everything beyond max_sq_dist struck out,
    and the k smallest of them -- which do not depend on how the candidates were found."""
    import numpy as np

    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, 3)
    _knn_args(p.shape, k, max_sq_dist)
    k, m = int(k), np.float32(max_sq_dist)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    best = np.full((len(p), k), none, dtype=np.uint64)
    idx = np.nonzero(np.isfinite(p).all(1))[0]
    if len(idx):
        idx = idx[np.argsort(p[idx, 0], kind="stable")]
        ps, px = p[idx], p[idx, 0].astype(np.float64)
        w = float(np.sqrt(np.float64(m))) * (1.0 + 2.0 ** -20) + 1e-20 if np.isfinite(m) else np.inf   # as in nearest_points_host
        with np.errstate(over="ignore", invalid="ignore"):
            for c0 in range(0, len(idx), chunk):
                qi = idx[c0:c0 + chunk]
                qc = p[qi]
                a = np.searchsorted(px, float(qc[0, 0]) - w, "left")
                b = np.searchsorted(px, float(qc[-1, 0]) + w, "right")
                acc = np.full((len(qi), k), none, dtype=np.uint64)
                for p0 in range(a, b, 8192):
                    rp, ri = ps[p0:min(p0 + 8192, b)], idx[p0:min(p0 + 8192, b)]
                    dx, dy, dz = (qc[:, None, c] - rp[None, :, c] for c in range(3))
                    d2 = (dx * dx + dy * dy) + dz * dz
                    key = (np.ascontiguousarray(d2).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ri.astype(np.uint64)[None, :]
                    key = np.where((d2 <= m) & (ri[None, :] != qi[:, None]), key, none)
                    if key.shape[1] > 4 * k:
                        key = np.partition(key, k - 1, axis=1)[:, :k]
                    acc = np.sort(np.concatenate([acc, key], 1), axis=1)[:, :k]
                best[qi] = acc
    found = best != none
    index = np.where(found, best & np.uint64(0xFFFFFFFF), 0).astype(np.int64).astype(np.int32)
    index[~found] = -1
    sqdist = np.where(found, (best >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf)).astype(np.float32)
    return KnnTable(index, sqdist, found.sum(1).astype(np.int32))


def knn_points(points, k: int, max_sq_dist: float) -> KnnTable:
    """points f32 [V,3] -> ``KnnTable``: per point its ``k`` (1 .. 32) nearest other points among those with
    ``d2 = (dx*dx + dy*dy) + dz*dz <= max_sq_dist`` (fp32, every operation rounded on its own: the d2 of ``nearest_points``), nearest
    first, ties to the lower index; fewer than k: the row is padded with -1 / +inf and ``count`` says how many there are
    (include/vlsat_cloud.h, vlsat_cloud_knn).  ``max_sq_dist`` is a SQUARED distance.  A point with a non-finite coordinate has no
    neighbours and is nobody's.  Exact and deterministic.  Device tensors run the HIP kernels (nothing is read back); CPU tensors or
    arrays run ``knn_points_host`` and get CPU tensors."""
    if not (isinstance(points, torch.Tensor) and points.is_cuda):
        t = knn_points_host(points.numpy() if isinstance(points, torch.Tensor) else points, k, max_sq_dist)
        return KnnTable(*(torch.from_numpy(x) for x in t))
    lib = L.load()
    if points.dtype != torch.float32:
        raise L.VlsatError("knn_points: points must be float32 [V,3]")
    _knn_args(points.shape, k, max_sq_dist)
    dev, points, v, k = points.device, points.contiguous(), points.shape[0], int(k)
    scratch = torch.empty(int(lib.vlsat_cloud_knn_scratch_bytes(v, k)), dtype=torch.uint8, device=dev)
    index = torch.empty((v, k), dtype=torch.int32, device=dev)
    sqdist = torch.empty((v, k), dtype=torch.float32, device=dev)
    count = torch.empty(v, dtype=torch.int32, device=dev)
    L.check(lib.vlsat_cloud_knn(points.data_ptr(), v, k, float(max_sq_dist), scratch.data_ptr(), index.data_ptr(), sqdist.data_ptr(),
                                count.data_ptr(), L.stream_ptr()))
    return KnnTable(index, sqdist, count)


def _normals_args(points_shape, index_shape, count_shape, min_points, viewpoint):
    import math
    if len(points_shape) != 2 or points_shape[1] != 3 or not 1 <= points_shape[0] <= SEG_MAX_VERTS:
        raise L.VlsatError("cloud_normals: points must be float32 [V,3] with 1 <= V <= 2^24")
    if len(index_shape) != 2 or index_shape[0] != points_shape[0] or not 1 <= index_shape[1] <= CLOUD_MAX_K:
        raise L.VlsatError("cloud_normals: knn_index must be int32 [V,K] with 1 <= K <= 32")
    if tuple(count_shape) != (points_shape[0],):
        raise L.VlsatError("cloud_normals: knn_count must be int32 [V]")
    if int(min_points) < 3:
        raise L.VlsatError("cloud_normals: min_points must be at least 3")
    if viewpoint is not None and (len(viewpoint) != 3 or any(math.isnan(float(x)) for x in viewpoint)):
        raise L.VlsatError("cloud_normals: the viewpoint is three numbers, none NaN")


def _jacobi_rotate(np, app, aqq, apq, arp, arq, vp, vq):
    """cloud_rotate of csrc/cloud_core.h on arrays: the same operations in the same order, the skipped pairs left as they are."""
    live = apq != 0.0
    theta = (aqq - app) / (2.0 * apq)
    den = np.abs(theta) + np.sqrt(theta * theta + 1.0)
    t = np.where(theta < 0.0, -1.0, 1.0) / den
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    tap = t * apq
    keep = lambda new, old: np.where(live, new, old)   # noqa: E731
    out = [keep(app - tap, app), keep(aqq + tap, aqq), keep(0.0, apq), keep(c * arp - s * arq, arp), keep(s * arp + c * arq, arq)]
    nvp = [keep(c * a - s * b, a) for a, b in zip(vp, vq)]
    nvq = [keep(s * a + c * b, b) for a, b in zip(vp, vq)]
    return (*out, nvp, nvq)


def cloud_normals_host(points, knn_index, knn_count, min_points: int = 5, viewpoint=None, rounded: bool = True):
    """The normal and flatness rule of include/vlsat_cloud.h in numpy float64, the same operations in the same order as
    csrc/cloud_core.h -> (normals f32 [V,3], curvature f32 [V]) as numpy arrays, every bit the device's.  ``rounded=False`` returns the
    float64 values before the last step, the rounding to fp32 (to compare the eigenvectors with another solver's)."""
    import numpy as np

    p32 = np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, 3)
    nbr = np.asarray(knn_index).astype(np.int64)
    cnt = np.asarray(knn_count).astype(np.int64).reshape(-1)
    _normals_args(p32.shape, nbr.shape, cnt.shape, min_points, viewpoint)
    v, k = nbr.shape
    p = p32.astype(np.float64)
    listed = np.clip(cnt, 0, k)
    member = (np.arange(k)[None, :] < listed[:, None]) & (nbr >= 0) & (nbr < v)
    safe = np.where(member, nbr, 0)
    with np.errstate(all="ignore"):
        s = p.copy()
        for j in range(k):
            s = np.where(member[:, j, None], s + p[safe[:, j]], s)
        n = 1 + member.sum(1)
        c = s / n[:, None].astype(np.float64)
        a = {key: np.zeros(v) for key in ("00", "01", "02", "11", "12", "22")}

        def add(a, q, on):
            d = q - c
            for key, (x, y) in (("00", (0, 0)), ("01", (0, 1)), ("02", (0, 2)), ("11", (1, 1)), ("12", (1, 2)), ("22", (2, 2))):
                a[key] = np.where(on, a[key] + d[:, x] * d[:, y], a[key])

        add(a, p, np.ones(v, bool))
        for j in range(k):
            add(a, p[safe[:, j]], member[:, j])
        trace = (a["00"] + a["11"]) + a["22"]
        have = (n >= int(min_points)) & (trace > 0.0)
        one, zero = np.ones(v), np.zeros(v)
        v0, v1, v2 = [one, zero, zero], [zero, one, zero], [zero, zero, one]      # columns of V: v0[r] = V[r][0]
        a00, a11, a22, a01, a02, a12 = a["00"], a["11"], a["22"], a["01"], a["02"], a["12"]
        for _ in range(CLOUD_SWEEPS):
            a00, a11, a01, a02, a12, v0, v1 = _jacobi_rotate(np, a00, a11, a01, a02, a12, v0, v1)
            a00, a22, a02, a01, a12, v0, v2 = _jacobi_rotate(np, a00, a22, a02, a01, a12, v0, v2)
            a11, a22, a12, a01, a02, v1, v2 = _jacobi_rotate(np, a11, a22, a12, a01, a02, v1, v2)
        lmin, nrm = a00, list(v0)
        for lam, col in ((a11, v1), (a22, v2)):
            lower = lam < lmin
            lmin = np.where(lower, lam, lmin)
            nrm = [np.where(lower, x, y) for x, y in zip(col, nrm)]
        curv = np.where(lmin > 0.0, lmin, 0.0) / ((a00 + a11) + a22)
        d = np.zeros(v)
        if viewpoint is not None:
            t = np.asarray([float(x) for x in viewpoint], dtype=np.float64)[None, :] - p
            d = (nrm[0] * t[:, 0] + nrm[1] * t[:, 1]) + nrm[2] * t[:, 2]
        big = nrm[0]
        big = np.where(np.abs(nrm[1]) > np.abs(big), nrm[1], big)
        big = np.where(np.abs(nrm[2]) > np.abs(big), nrm[2], big)
        flip = np.where(d < 0.0, True, np.where(d > 0.0, False, big < 0.0))
        nrm = np.stack([np.where(flip, -x, x) for x in nrm], 1)
        normals = np.where(have[:, None], nrm, 0.0)
        curvature = np.where(have, curv, 1.0)
    return (normals.astype(np.float32), curvature.astype(np.float32)) if rounded else (normals, curvature)


def cloud_normals(points, knn_index, knn_count, min_points: int = 5, viewpoint=None):
    """points f32 [V,3] and the table of ``knn_points`` -> (normals f32 [V,3], curvature f32 [V]): per point the eigenvector of the
    smallest eigenvalue of the covariance of the point and its neighbours, and the surface variation lambda_min / (l0 + l1 + l2) in
    [0, 1/3] -- 0 on a plane, large at a crease (include/vlsat_cloud.h, vlsat_cloud_normals: fp64, six cyclic Jacobi sweeps).  Fewer than
    ``min_points`` members (the point counts) or coincident members: normal (0, 0, 0), curvature 1.  ``viewpoint`` (x, y, z) turns every
    normal towards it; without one the sign is a convention (largest component positive) and means nothing: segment with
    ``unsigned=True``.  Device tensors run the HIP kernel; CPU tensors or arrays run ``cloud_normals_host`` and get CPU tensors."""
    if not (isinstance(points, torch.Tensor) and points.is_cuda):
        as_np = lambda x: x.numpy() if isinstance(x, torch.Tensor) else x   # noqa: E731
        n, c = cloud_normals_host(as_np(points), as_np(knn_index), as_np(knn_count), min_points, viewpoint)
        return torch.from_numpy(n), torch.from_numpy(c)
    lib = L.load()
    if points.dtype != torch.float32:
        raise L.VlsatError("cloud_normals: points must be float32 [V,3]")
    _normals_args(points.shape, knn_index.shape, knn_count.shape, min_points, viewpoint)
    dev, points = points.device, points.contiguous()
    index = knn_index.to(device=dev, dtype=torch.int32).contiguous()
    count = knn_count.to(device=dev, dtype=torch.int32).contiguous()
    v, k = index.shape
    normals = torch.empty((v, 3), dtype=torch.float32, device=dev)
    curvature = torch.empty(v, dtype=torch.float32, device=dev)
    vp = [float(x) for x in viewpoint] if viewpoint is not None else [0.0, 0.0, 0.0]
    L.check(lib.vlsat_cloud_normals(points.data_ptr(), index.data_ptr(), count.data_ptr(), v, k, int(min_points), int(viewpoint is not None),
                                    vp[0], vp[1], vp[2], normals.data_ptr(), curvature.data_ptr(), L.stream_ptr()))
    return normals, curvature


def knn_edges(knn_index):
    """The neighbour table as an explicit edge list int32 [V K, 2]: edge e joins e // K and index[e]; the -1 pads stay and are ignored
    by the rule.  ``segment_mesh`` on this list equals ``segment_cloud`` on the table."""
    import numpy as np
    if torch.is_tensor(knn_index):
        v, k = knn_index.shape
        a = torch.arange(v, dtype=torch.int32, device=knn_index.device).repeat_interleave(k)
        return torch.stack([a, knn_index.to(torch.int32).reshape(-1)], 1).contiguous()
    idx = np.asarray(knn_index).astype(np.int32)
    v, k = idx.shape
    return np.ascontiguousarray(np.stack([np.repeat(np.arange(v, dtype=np.int32), k), idx.reshape(-1)], 1))


def segment_cloud(normals: torch.Tensor, knn_index: torch.Tensor, max_weight: float, min_verts: int = 20, unsigned: bool = True,
                  trim: bool = True) -> MeshSegments:
    """normals f32 [V,3] and the neighbour table int32 [V,K] of ``knn_points`` -> ``MeshSegments``: the rule of ``segment_mesh`` over
    the pairs (i, index[i, j]) instead of mesh edges (include/vlsat_cloud.h, vlsat_segment_cloud).  ``unsigned=True`` weighs an edge
    1 - |dot|, for normals whose sign is a convention (``cloud_normals`` without a viewpoint); ``unsigned=False`` is the mesh's
    1 - dot.  A zero normal weighs 1 against everyone: it links to nobody and is absorbed by a neighbour.  Device tensors: the HIP
    kernels, asynchronous, ``trim`` as in ``segment_mesh``.  CPU tensors: ``segment_mesh_host`` on ``knn_edges(knn_index)``."""
    if not normals.is_cuda:
        return segment_mesh_host(normals, knn_edges(knn_index), max_weight, min_verts, trim, unsigned=unsigned)
    lib = L.load()
    if normals.dtype != torch.float32:
        raise L.VlsatError("segment_cloud: normals must be float32 [V,3]")
    if len(knn_index.shape) != 2 or knn_index.shape[0] != normals.shape[0] or not 1 <= knn_index.shape[1] <= CLOUD_MAX_K:
        raise L.VlsatError("segment_cloud: knn_index must be int32 [V,K] with 1 <= K <= 32")
    _segment_args(normals, torch.empty((0, 2)), max_weight, min_verts)
    dev, normals = normals.device, normals.contiguous()
    index = knn_index.to(device=dev, dtype=torch.int32).contiguous()
    v, k = index.shape
    scratch = torch.empty(int(lib.vlsat_segment_mesh_scratch_bytes(v, v * k)), dtype=torch.uint8, device=dev)
    labels = torch.empty(v, dtype=torch.int32, device=dev)
    seg_size = torch.empty(v, dtype=torch.int32, device=dev)
    n_segments = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(lib.vlsat_segment_cloud(normals.data_ptr(), index.data_ptr(), v, k, float(max_weight), int(min_verts), int(bool(unsigned)),
                                    scratch.data_ptr(), labels.data_ptr(), n_segments.data_ptr(), seg_size.data_ptr(), L.stream_ptr()))
    out = MeshSegments(labels, n_segments, seg_size)
    return out.trim() if trim else out


# ---- a cloud resampled on a voxel grid (csrc/voxel.hip; the rule is stated in include/vlsat_voxel.h) --------------------------------------
VOXEL_CELL_LIMIT = 1 << 20
VOXEL_COORD_LIMIT = 32768.0


class VoxelCloud(NamedTuple):
    """``voxel_downsample``: ``points`` f32 [M,3], ``normals`` f32 [M,3] | None, ``colors`` u8 [M,3] | None, ``voxel_of_point`` int32 [V]
    (-1: out of range or in a dropped voxel), ``first_point`` int32 [M] (the lowest input index of each voxel), ``count`` int32 [M]."""
    points: object
    normals: object
    colors: object
    voxel_of_point: object
    first_point: object
    count: object


def _voxel_args(shape, voxel, origin, min_count, normals_shape, colors_shape):
    """-> (inv as np.float32, origin as np.float32 [3]); raises on anything the rule refuses"""
    import numpy as np
    if len(shape) != 2 or shape[1] != 3 or not 1 <= shape[0] <= SEG_MAX_VERTS:
        raise L.VlsatError("voxel_downsample: points must be float32 [V,3] with 1 <= V <= 2^24")
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        size = np.float32(voxel)
        inv = np.float32(1.0) / size
    if not (size > 0 and inv > 0 and np.isfinite(inv)):
        raise L.VlsatError("voxel_downsample: voxel must be > 0 and finite, and so must 1 / voxel in fp32")
    if len(origin) != 3:
        raise L.VlsatError("voxel_downsample: the origin is three numbers")
    with np.errstate(over="ignore"):
        o = np.asarray([float(x) for x in origin], dtype=np.float32)
    if not np.isfinite(o).all():
        raise L.VlsatError("voxel_downsample: the origin must be finite")
    if int(min_count) < 1:
        raise L.VlsatError("voxel_downsample: min_count must be at least 1")
    for what, s in (("normals", normals_shape), ("colors", colors_shape)):
        if s is not None and tuple(s) != tuple(shape):
            raise L.VlsatError(f"voxel_downsample: {what} must be [V,3], one row per point")
    return inv, o


def voxel_keys_host(points, voxel: float, origin=(0.0, 0.0, 0.0)):
    """Rule 1 of include/vlsat_voxel.h in numpy: -> (key uint64 [V], in_range bool [V]); the key of a point out of range is all ones."""
    import numpy as np
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, 3)
    inv, o = _voxel_args(p.shape, voxel, origin, 1, None, None)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.floor((p - o[None, :]) * inv)                          # fp32: the difference and the product each rounded on their own
        ok = (np.abs(p) < np.float32(VOXEL_COORD_LIMIT)).all(1) & (np.abs(t) < np.float32(VOXEL_CELL_LIMIT)).all(1)
    c = (np.where(ok[:, None], t, np.float32(0)).astype(np.int64) + VOXEL_CELL_LIMIT).astype(np.uint64)
    key = (c[:, 2] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 0]
    return np.where(ok, key, np.uint64(0xFFFFFFFFFFFFFFFF)), ok


def _group_sums(np, values, order, starts):
    """int64 [V,C] summed over the runs of ``order`` that begin at ``starts``: exact, integer, in any order the same"""
    return np.add.reduceat(values[order], starts, axis=0) if len(starts) else np.zeros((0, values.shape[1]), np.int64)


def voxel_downsample_host(points, voxel: float, origin=(0.0, 0.0, 0.0), min_count: int = 1, normals=None, colors=None) -> VoxelCloud:
    """The rule of include/vlsat_voxel.h in numpy -> ``VoxelCloud`` of numpy arrays, every bit the device's: cells and keys in fp32,
    voxels by ``np.unique`` over the keys, numbered by their first point, positions and normals as int64 sums of quantised values
    (``np.rint`` rounds half to even, as llrint does), colours as integer means rounded half up."""
    import numpy as np
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, 3)
    nrm = None if normals is None else np.ascontiguousarray(np.asarray(normals, dtype=np.float32)).reshape(-1, 3)
    col = None if colors is None else np.ascontiguousarray(np.asarray(colors, dtype=np.uint8)).reshape(-1, 3)
    _voxel_args(p.shape, voxel, origin, min_count, None if nrm is None else nrm.shape, None if col is None else col.shape)
    key, ok = voxel_keys_host(p, voxel, origin)
    idx = np.nonzero(ok)[0]
    _, first, inverse, count = np.unique(key[idx], return_index=True, return_inverse=True, return_counts=True)
    first = idx[first]                                               # np.unique names the first occurrence: the lowest point index
    kept = np.nonzero(count >= int(min_count))[0]
    kept = kept[np.argsort(first[kept], kind="stable")]              # numbered by ascending first point
    number = np.full(len(count), -1, dtype=np.int64)
    number[kept] = np.arange(len(kept))
    voxel_of_point = np.full(len(p), -1, dtype=np.int32)
    voxel_of_point[idx] = number[inverse.reshape(-1)]
    members = np.nonzero(voxel_of_point >= 0)[0]
    order = members[np.argsort(voxel_of_point[members], kind="stable")]
    n = count[kept].astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64) if len(kept) else np.zeros(0, np.int64)
    q = np.rint(p.astype(np.float64) * 2.0 ** 24)
    q = np.where(ok[:, None], q, 0.0).astype(np.int64)
    out_points = (_group_sums(np, q, order, starts).astype(np.float64) / n[:, None].astype(np.float64) * 2.0 ** -24).astype(np.float32)
    out_normals = out_colors = None
    if nrm is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            counted = np.abs(nrm) < np.float32(VOXEL_COORD_LIMIT)
            qn = np.rint(np.where(counted, nrm, np.float32(0)).astype(np.float64) * 2.0 ** 20).astype(np.int64)
        s = _group_sums(np, qn, order, starts).astype(np.float64)
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        with np.errstate(invalid="ignore", divide="ignore"):
            out_normals = np.where(length[:, None] == 0, 0.0, s / length[:, None]).astype(np.float32)
    if col is not None:
        s = _group_sums(np, col.astype(np.int64), order, starts)
        out_colors = ((2 * s + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    return VoxelCloud(out_points, out_normals, out_colors, voxel_of_point, first[kept].astype(np.int32), count[kept].astype(np.int32))


def voxel_downsample(points, voxel: float, origin=(0.0, 0.0, 0.0), min_count: int = 1, normals=None, colors=None) -> VoxelCloud:
    """points f32 [V,3] resampled on a grid of cells of edge ``voxel`` anchored at ``origin`` -> ``VoxelCloud``: one representative per
    occupied cell that holds at least ``min_count`` points -- the mean position, the normalised mean normal and the mean colour, all
    from integer sums, so exact and the same in every run -- numbered by the cell's first point in the input, and ``voxel_of_point``
    to carry a result on the resampled cloud back to every input point (include/vlsat_voxel.h states the rule and its limits: |x| <
    32768 and cell coordinates below 2^20 in magnitude, else a point belongs to no voxel).  The origin anchors the grid to the frame,
    not to the cloud: two clouds in one frame share cells.  Device tensors run the HIP kernels (one host wait: the number of voxels is
    read to size the outputs); CPU tensors or arrays run ``voxel_downsample_host`` and get CPU tensors, with equal bits."""
    if not (isinstance(points, torch.Tensor) and points.is_cuda):
        as_np = lambda x: x.numpy() if isinstance(x, torch.Tensor) else x       # noqa: E731
        out = voxel_downsample_host(as_np(points), voxel, origin, min_count, None if normals is None else as_np(normals),
                                    None if colors is None else as_np(colors))
        return VoxelCloud(*(None if x is None else torch.from_numpy(x) for x in out))
    lib = L.load()
    if points.dtype != torch.float32:
        raise L.VlsatError("voxel_downsample: points must be float32 [V,3]")
    for what, x, dtype in (("normals", normals, torch.float32), ("colors", colors, torch.uint8)):
        if x is not None and not (isinstance(x, torch.Tensor) and x.device == points.device and x.dtype == dtype):
            raise L.VlsatError(f"voxel_downsample: {what} must be a {dtype} tensor on the device of the points")
    _, o = _voxel_args(points.shape, voxel, origin, min_count, None if normals is None else normals.shape,
                       None if colors is None else colors.shape)
    dev, points, v = points.device, points.contiguous(), points.shape[0]
    normals = None if normals is None else normals.contiguous()
    colors = None if colors is None else colors.contiguous()
    scratch = torch.empty(int(lib.vlsat_voxel_scratch_bytes(v)), dtype=torch.uint8, device=dev)
    voxel_of_point = torch.empty(v, dtype=torch.int32, device=dev)
    first_point = torch.empty(v, dtype=torch.int32, device=dev)
    count = torch.empty(v, dtype=torch.int32, device=dev)
    n_voxels = torch.empty(2, dtype=torch.int32, device=dev)
    L.check(lib.vlsat_voxel_assign(points.data_ptr(), v, float(voxel), float(o[0]), float(o[1]), float(o[2]), int(min_count),
                                   scratch.data_ptr(), voxel_of_point.data_ptr(), first_point.data_ptr(), count.data_ptr(),
                                   n_voxels.data_ptr(), L.stream_ptr()))
    m, overflow = (int(x) for x in n_voxels.tolist())                # the one host wait: the outputs are sized from the device's count
    if overflow:
        raise L.VlsatError("voxel_downsample: the hash table overflowed (the device raised its error flag)")
    first_point, count = first_point[:m].clone(), count[:m].clone()
    out_points = torch.empty((m, 3), dtype=torch.float32, device=dev)
    out_normals = None if normals is None else torch.empty((m, 3), dtype=torch.float32, device=dev)
    out_colors = None if colors is None else torch.empty((m, 3), dtype=torch.uint8, device=dev)
    if m:                                                            # no voxel: nothing to launch
        L.check(lib.vlsat_voxel_reduce(points.data_ptr(), 0 if normals is None else normals.data_ptr(),
                                       0 if colors is None else colors.data_ptr(), voxel_of_point.data_ptr(), count.data_ptr(), v, m,
                                       scratch.data_ptr(), out_points.data_ptr(), 0 if out_normals is None else out_normals.data_ptr(),
                                       0 if out_colors is None else out_colors.data_ptr(), L.stream_ptr()))
    return VoxelCloud(out_points, out_normals, out_colors, voxel_of_point, first_point, count)


# ---- a cloud segmented into objects: structural planes, then clusters (csrc/objects.hip; the rules are stated in include/vlsat_objects.h) ----
PLANE_MAX_HYP = 4096
PLANE_MAX_PLANES = 32
PLANE_MAX_PPM = 500000


class CloudPlanes(NamedTuple):
    """``cloud_planes``: ``plane_id`` int32 [V] (0 = no plane, else 1..n), ``planes`` f32 [P,4] = (nx, ny, nz, d) and ``counts`` int32
    [P,3] = (inliers, above, below) per found plane (unused rows zero), ``n_planes`` int32 [1]."""
    plane_id: object
    planes: object
    counts: object
    n_planes: object


class CloudClusters(NamedTuple):
    """``cloud_clusters``: ``labels`` int32 [V] (0 = none, else 1..S by lowest point), ``n_clusters`` int32 [1], ``cluster_size`` int32
    [V] (entry s - 1 is the size of cluster s, zeros past S)."""
    labels: object
    n_clusters: object
    cluster_size: object


def _planes_args(shape, n_hyp, max_planes, dist, min_inliers, outside_ppm):
    """-> dist as np.float32; raises on anything the rule refuses"""
    import numpy as np
    if len(shape) != 2 or shape[1] != 3 or not 3 <= shape[0] <= SEG_MAX_VERTS:
        raise L.VlsatError("cloud_planes: points must be float32 [V,3] with 3 <= V <= 2^24")
    if not 1 <= int(n_hyp) <= PLANE_MAX_HYP:
        raise L.VlsatError("cloud_planes: 1 <= n_hyp <= 4096")
    if not 1 <= int(max_planes) <= PLANE_MAX_PLANES:
        raise L.VlsatError("cloud_planes: 1 <= max_planes <= 32")
    with np.errstate(over="ignore"):
        d = np.float32(dist)
    if not (d > 0 and np.isfinite(d)):
        raise L.VlsatError("cloud_planes: dist must be > 0 and finite in fp32")
    if not 3 <= int(min_inliers) < 1 << 31:
        raise L.VlsatError("cloud_planes: min_inliers must be at least 3")
    if not 0 <= int(outside_ppm) <= PLANE_MAX_PPM:
        raise L.VlsatError("cloud_planes: outside_ppm must be in 0 .. 500000")
    return d


def plane_draws(seed: int, k, n: int):
    """``split_draw(seed, k, n)`` for an array of counters k (uint64 arithmetic that wraps, as the device's does) -> int64 ranks"""
    import numpy as np
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & _M64) + np.uint64(0x9E3779B97F4A7C15) * (np.asarray(k, dtype=np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return (((z >> np.uint64(32)) * np.uint64(int(n))) >> np.uint64(32)).astype(np.int64)


def plane_from_points_host(a, b, c):
    """Rule 3 of include/vlsat_objects.h on arrays of points f32 [H,3] (plane_from_points of csrc/plane_core.h: fp64, the same operations
    in the same order) -> (planes f32 [H,4], ok bool [H]); a void hypothesis has a zero row."""
    import numpy as np
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        u, v = b - a, c - a
        mx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        my = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        mz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        l2 = (mx * mx + my * my) + mz * mz
        ok = (l2 > 0.0) & (l2 < np.inf)
        length = np.sqrt(np.where(ok, l2, 1.0))
        nx, ny, nz = mx / length, my / length, mz / length
        big = nx
        big = np.where(np.abs(ny) > np.abs(big), ny, big)
        big = np.where(np.abs(nz) > np.abs(big), nz, big)
        flip = big < 0.0
        nx, ny, nz = (np.where(flip, -x, x) for x in (nx, ny, nz))
        d = -((nx * a[:, 0] + ny * a[:, 1]) + nz * a[:, 2])
        planes = np.stack([nx, ny, nz, d], 1).astype(np.float32)
    return np.where(ok[:, None], planes, np.float32(0.0)).astype(np.float32), ok


def plane_scores_host(planes, points):
    """Rule 4: s = fl(fl(fl(fl(nx x) + fl(ny y)) + fl(nz z)) + d) in fp32 for planes f32 [H,4] x points f32 [n,3] -> f32 [H,n]"""
    import numpy as np
    pl, p = np.asarray(planes, dtype=np.float32), np.asarray(points, dtype=np.float32)
    with np.errstate(all="ignore"):
        return ((pl[:, 0, None] * p[None, :, 0] + pl[:, 1, None] * p[None, :, 1]) + pl[:, 2, None] * p[None, :, 2]) + pl[:, 3, None]


def cloud_planes_host(points, n_hyp: int, max_planes: int, dist: float, min_inliers: int, outside_ppm: int, seed: int = 0) -> CloudPlanes:
    """The plane rule of include/vlsat_objects.h in numpy, the same operations in the same order -> ``CloudPlanes`` of numpy arrays,
    every bit the device's: per round the alive list, the draws of ``split_draw``, the planes in fp64 rounded to fp32, the scores in
    fp32, integer counts, the eligibility test and the key."""
    import numpy as np
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, 3)
    dist = _planes_args(p.shape, n_hyp, max_planes, dist, min_inliers, outside_ppm)
    n_hyp, max_planes, min_inliers, outside_ppm = int(n_hyp), int(max_planes), int(min_inliers), int(outside_ppm)
    alive = np.isfinite(p).all(1)
    plane_id = np.zeros(len(p), dtype=np.int32)
    planes = np.zeros((max_planes, 4), dtype=np.float32)
    counts = np.zeros((max_planes, 3), dtype=np.int32)
    found = 0
    for r in range(max_planes):
        idx = np.nonzero(alive)[0]
        n = len(idx)
        if n < 3:
            break
        k = (np.arange(n_hyp, dtype=np.uint64) + np.uint64(r * n_hyp)) * np.uint64(3)
        a, b, c = (p[idx[plane_draws(seed, k + np.uint64(j), n)]] for j in range(3))
        hyp, ok = plane_from_points_host(a, b, c)
        q = p[idx]
        inliers, above = np.zeros(n_hyp, dtype=np.int64), np.zeros(n_hyp, dtype=np.int64)
        step = max(1, (1 << 22) // n)
        with np.errstate(invalid="ignore"):
            for h0 in range(0, n_hyp, step):
                s = plane_scores_host(hyp[h0:h0 + step], q)
                inliers[h0:h0 + step] = (np.abs(s) <= dist).sum(1)
                above[h0:h0 + step] = (s > dist).sum(1)
        below = n - inliers - above
        eligible = ok & (inliers >= min_inliers) & (np.minimum(above, below) <= (n * outside_ppm) // 1000000)
        if not eligible.any():
            break
        key = (inliers.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(n_hyp, dtype=np.uint64))
        h = int(np.argmax(np.where(eligible, key, np.uint64(0))))
        with np.errstate(invalid="ignore"):
            hit = np.abs(plane_scores_host(hyp[h:h + 1], q)[0]) <= dist
        plane_id[idx[hit]] = r + 1
        alive[idx[hit]] = False
        planes[r] = hyp[h]
        counts[r] = (inliers[h], above[h], below[h])
        found = r + 1
    return CloudPlanes(plane_id, planes, counts, np.asarray([found], dtype=np.int32))


def cloud_planes(points, n_hyp: int, max_planes: int, dist: float, min_inliers: int, outside_ppm: int, seed: int = 0) -> CloudPlanes:
    """points f32 [V,3] -> ``CloudPlanes``: the structural planes of a room (include/vlsat_objects.h, vlsat_cloud_planes).  In each of up
    to ``max_planes`` rounds ``n_hyp`` planes through three drawn points (``split_draw`` under ``seed``) are scored against every
    point that is still alive; a plane is eligible when it has at least ``min_inliers`` points within ``dist`` AND at most
    ``outside_ppm`` millionths of the alive points on one of its sides -- a floor or a wall, not a table top; the eligible plane with
    most inliers wins and its inliers leave.  There is no refit: ``planes`` are the planes that were scored.  Device tensors run the HIP
    kernels: all rounds are enqueued, the rounds after a stop return at once, and nothing is read back (``n_planes`` stays on the
    device).  CPU tensors or arrays run ``cloud_planes_host`` and get CPU tensors, with equal bits."""
    if not (isinstance(points, torch.Tensor) and points.is_cuda):
        out = cloud_planes_host(points.numpy() if isinstance(points, torch.Tensor) else points, n_hyp, max_planes, dist, min_inliers,
                                outside_ppm, seed)
        return CloudPlanes(*(torch.from_numpy(x) for x in out))
    lib = L.load()
    if points.dtype != torch.float32:
        raise L.VlsatError("cloud_planes: points must be float32 [V,3]")
    dist = _planes_args(points.shape, n_hyp, max_planes, dist, min_inliers, outside_ppm)
    dev, points, v = points.device, points.contiguous(), points.shape[0]
    scratch = torch.empty(int(lib.vlsat_cloud_planes_scratch_bytes(v, int(n_hyp))), dtype=torch.uint8, device=dev)
    plane_id = torch.empty(v, dtype=torch.int32, device=dev)
    planes = torch.empty((int(max_planes), 4), dtype=torch.float32, device=dev)
    counts = torch.empty((int(max_planes), 3), dtype=torch.int32, device=dev)
    n_planes = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(lib.vlsat_cloud_planes(points.data_ptr(), v, int(n_hyp), int(max_planes), float(dist), int(min_inliers), int(outside_ppm),
                                   int(seed) & _M64, scratch.data_ptr(), plane_id.data_ptr(), planes.data_ptr(), counts.data_ptr(),
                                   n_planes.data_ptr(), L.stream_ptr()))
    return CloudPlanes(plane_id, planes, counts, n_planes)


def _clusters_args(index_shape, sqdist_shape, mask_shape, max_sq_dist, min_points):
    import math
    if len(index_shape) != 2 or not 1 <= index_shape[0] <= SEG_MAX_VERTS or not 1 <= index_shape[1] <= CLOUD_MAX_K:
        raise L.VlsatError("cloud_clusters: knn_index must be int32 [V,K] with 1 <= V <= 2^24 and 1 <= K <= 32")
    if tuple(sqdist_shape) != tuple(index_shape):
        raise L.VlsatError("cloud_clusters: knn_sqdist must be float32 [V,K], the shape of knn_index")
    if tuple(mask_shape) != (index_shape[0],):
        raise L.VlsatError("cloud_clusters: mask must be int32 [V]")
    if math.isnan(float(max_sq_dist)):
        raise L.VlsatError("cloud_clusters: max_sq_dist is NaN")
    if not 1 <= int(min_points) < 1 << 31:
        raise L.VlsatError("cloud_clusters: min_points must be at least 1")


def cloud_clusters_host(knn_index, knn_sqdist, mask, max_sq_dist: float, min_points: int = 1) -> CloudClusters:
    """The cluster rule of include/vlsat_objects.h in numpy -> ``CloudClusters`` of numpy arrays, equal to the device's: the table
    entries that join two eligible points within ``max_sq_dist`` are united (``_seg_unite``: the lowest member is the root), components
    below ``min_points`` get 0 and the rest are numbered by lowest point."""
    import numpy as np
    nbr = np.asarray(knn_index).astype(np.int64)
    d2 = np.asarray(knn_sqdist, dtype=np.float32)
    m = np.asarray(mask).reshape(-1) != 0
    _clusters_args(nbr.shape, d2.shape, m.shape, max_sq_dist, min_points)
    v, k = nbr.shape
    i = np.repeat(np.arange(v, dtype=np.int64), k)
    j = nbr.reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = (j >= 0) & (j < v) & (j != i) & (d2.reshape(-1) <= np.float32(max_sq_dist))
    ok &= m[i] & m[np.where(ok, j, 0)]
    parent = _seg_unite(np.arange(v, dtype=np.int64), i[ok], j[ok])
    size = np.bincount(parent[m], minlength=v)
    kept = m & (parent == np.arange(v)) & (size >= int(min_points))
    num = np.where(kept, np.cumsum(kept), 0)
    labels = np.where(m, num[parent], 0).astype(np.int32)
    s = int(kept.sum())
    cluster_size = np.zeros(v, dtype=np.int32)
    cluster_size[:s] = size[kept]
    return CloudClusters(labels, np.asarray([s], dtype=np.int32), cluster_size)


def cloud_clusters(knn_index, knn_sqdist, mask, max_sq_dist: float, min_points: int = 1) -> CloudClusters:
    """The table of ``knn_points`` and a mask int32 [V] (non-zero: the point takes part) -> ``CloudClusters``: Euclidean clusters, the
    connected components of the table entries that join two eligible points at a squared distance of at most ``max_sq_dist``
    (include/vlsat_objects.h, vlsat_cloud_clusters).  A component of fewer than ``min_points`` points gets 0; the rest are numbered 1..S
    by lowest point.  Points that touch through the table are one cluster: two objects closer than the radius merge.  Device tensors run
    the HIP kernels (7 launches, nothing read back); CPU tensors or arrays run ``cloud_clusters_host`` and get CPU tensors."""
    if not (isinstance(knn_index, torch.Tensor) and knn_index.is_cuda):
        as_np = lambda x: x.numpy() if isinstance(x, torch.Tensor) else x   # noqa: E731
        out = cloud_clusters_host(as_np(knn_index), as_np(knn_sqdist), as_np(mask), max_sq_dist, min_points)
        return CloudClusters(*(torch.from_numpy(x) for x in out))
    lib = L.load()
    _clusters_args(knn_index.shape, knn_sqdist.shape, mask.shape, max_sq_dist, min_points)
    dev = knn_index.device
    index = knn_index.to(dtype=torch.int32).contiguous()
    sqdist = knn_sqdist.to(device=dev, dtype=torch.float32).contiguous()
    mask = (mask.to(device=dev) != 0).to(torch.int32).contiguous()
    v, k = index.shape
    scratch = torch.empty(int(lib.vlsat_cloud_clusters_scratch_bytes(v)), dtype=torch.uint8, device=dev)
    labels = torch.empty(v, dtype=torch.int32, device=dev)
    n_clusters = torch.empty(1, dtype=torch.int32, device=dev)
    cluster_size = torch.empty(v, dtype=torch.int32, device=dev)
    L.check(lib.vlsat_cloud_clusters(index.data_ptr(), sqdist.data_ptr(), mask.data_ptr(), v, k, float(max_sq_dist), int(min_points),
                                     scratch.data_ptr(), labels.data_ptr(), n_clusters.data_ptr(), cluster_size.data_ptr(), L.stream_ptr()))
    return CloudClusters(labels, n_clusters, cluster_size)


# ---- convexity-aware clusters: bodies that touch are cut at their concave junctions (csrc/convex.hip; include/vlsat_convex.h states the rule) ----
CONVEX_MAX_ROUNDS = 64


class ConvexClusters(NamedTuple):
    """``convex_clusters``: ``labels`` int32 [V] (0 = none, else 1..S by lowest core point), ``n_clusters`` int32 [1], ``cluster_size``
    int32 [V] (entry s - 1 counts ALL final members of cluster s, zeros past S), ``state`` int32 [V]: 0 not eligible, 1 core of a kept
    component, 2 boundary (concave evidence), 3 eligible without a usable normal, 4 core of a dissolved component."""
    labels: object
    n_clusters: object
    cluster_size: object
    state: object


def _convex_args(points_shape, normals_shape, index_shape, sqdist_shape, mask_shape, link_sq_dist, concavity, min_points, absorb_rounds):
    """-> concavity as np.float32; raises on anything the rule refuses"""
    import math

    import numpy as np
    if len(index_shape) != 2 or not 1 <= index_shape[0] <= SEG_MAX_VERTS or not 1 <= index_shape[1] <= CLOUD_MAX_K:
        raise L.VlsatError("convex_clusters: knn_index must be int32 [V,K] with 1 <= V <= 2^24 and 1 <= K <= 32")
    if tuple(points_shape) != (index_shape[0], 3) or tuple(normals_shape) != (index_shape[0], 3):
        raise L.VlsatError("convex_clusters: points and normals must be float32 [V,3]")
    if tuple(sqdist_shape) != tuple(index_shape):
        raise L.VlsatError("convex_clusters: knn_sqdist must be float32 [V,K], the shape of knn_index")
    if tuple(mask_shape) != (index_shape[0],):
        raise L.VlsatError("convex_clusters: mask must be int32 [V]")
    if math.isnan(float(link_sq_dist)):
        raise L.VlsatError("convex_clusters: link_sq_dist is NaN")
    tau = np.float32(concavity)
    if not (tau >= 0 and tau <= 1):
        raise L.VlsatError("convex_clusters: concavity must be in [0, 1] (the sine of the tolerated concave angle)")
    if not 1 <= int(min_points) < 1 << 31:
        raise L.VlsatError("convex_clusters: min_points must be at least 1")
    if not 0 <= int(absorb_rounds) <= CONVEX_MAX_ROUNDS:
        raise L.VlsatError("convex_clusters: absorb_rounds must be in 0 .. 64")
    return tau


def convex_evidence_host(xi, ni, xj, nj, sqdist, concavity):
    """Rule 2 of include/vlsat_convex.h on arrays of float32 rows [n,3] (convex_c and convex_concave of csrc/convex_core.h, the same
    operations in the same order, each rounded to fp32) -> (c f32 [n], concave bool [n]).  Whether an entry COUNTS is the caller's."""
    import numpy as np
    xi, ni, xj, nj = (np.asarray(x, dtype=np.float32) for x in (xi, ni, xj, nj))
    q, tau = np.asarray(sqdist, dtype=np.float32), np.float32(concavity)
    with np.errstate(all="ignore"):
        d = xj - xi
        a = (ni[:, 0] * d[:, 0] + ni[:, 1] * d[:, 1]) + ni[:, 2] * d[:, 2]
        b = (nj[:, 0] * d[:, 0] + nj[:, 1] * d[:, 1]) + nj[:, 2] * d[:, 2]
        c = a - b
        concave = (c > 0) & (c * c > (tau * tau) * q)
    return c, concave


def convex_clusters_host(points, normals, knn_index, knn_sqdist, mask, link_sq_dist: float, concavity: float, min_points: int = 1,
                         absorb_rounds: int = 8) -> ConvexClusters:
    """The rule of include/vlsat_convex.h in numpy, the same operations in the same order (float32 throughout the predicate) ->
    ``ConvexClusters`` of numpy arrays, equal to the device's bit for bit: the concave table entries mark both their ends as boundary,
    the remaining oriented points are united along the entries within ``link_sq_dist`` (``_seg_unite``), components below
    ``min_points`` are dissolved, and in ``absorb_rounds`` synchronous rounds every unlabelled eligible point takes the label of the
    first labelled entry of its row."""
    import numpy as np
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
    n = np.ascontiguousarray(np.asarray(normals, dtype=np.float32))
    nbr = np.asarray(knn_index).astype(np.int64)
    q = np.asarray(knn_sqdist, dtype=np.float32)
    m = np.asarray(mask) != 0
    tau = _convex_args(p.shape, n.shape, nbr.shape, q.shape, m.shape, link_sq_dist, concavity, min_points, absorb_rounds)
    v, k = nbr.shape
    rows = np.arange(v, dtype=np.int64)
    eligible = m & np.isfinite(p).all(1)
    oriented = eligible & np.isfinite(n).all(1) & (n != 0).any(1)
    i, j = np.repeat(rows, k), nbr.reshape(-1)
    valid = (j >= 0) & (j < v) & (j != i)                                              # an entry that names another point
    js = np.where(valid, j, 0)
    qf = q.reshape(-1)
    with np.errstate(invalid="ignore"):
        counts = valid & oriented[i] & oriented[js] & np.isfinite(qf) & (qf >= 0)
    _, concave = convex_evidence_host(p[i], n[i], p[js], n[js], qf, tau)
    concave &= counts
    boundary = np.zeros(v, dtype=bool)
    boundary[i[concave]] = True
    boundary[js[concave]] = True
    core = oriented & ~boundary
    with np.errstate(invalid="ignore"):
        link = valid & core[i] & core[js] & (qf <= np.float32(link_sq_dist))
    parent = _seg_unite(rows.copy(), i[link], js[link])
    size = np.bincount(parent[core], minlength=v)
    kept = core & (parent == rows) & (size >= int(min_points))
    label = np.where(core & (size[parent] >= int(min_points)), parent, -1)             # the root, until the numbering
    state = np.select([~eligible, boundary, ~oriented, label < 0], [0, 2, 3, 4], 1).astype(np.int32)
    valid2, js2 = valid.reshape(v, k), js.reshape(v, k)
    for _ in range(int(absorb_rounds)):
        wait = np.nonzero(eligible & (label < 0))[0]
        if not len(wait):
            break
        seen = np.where(valid2[wait], label[js2[wait]], -1)                           # the labels at the end of the round before
        has = seen >= 0
        first = np.argmax(has, axis=1)
        take = has.any(1)
        if not take.any():
            break                                                                      # nothing can change in a later round either
        new = label.copy()
        new[wait[take]] = seen[take, first[take]]
        label = new
    num = np.where(kept, np.cumsum(kept), 0)
    labels = np.where(label >= 0, num[np.maximum(label, 0)], 0).astype(np.int32)
    s = int(kept.sum())
    cluster_size = np.zeros(v, dtype=np.int32)
    cluster_size[:s] = np.bincount(labels[labels > 0] - 1, minlength=s)[:s]
    return ConvexClusters(labels, np.asarray([s], dtype=np.int32), cluster_size, state)


def convex_clusters(points, normals, knn_index, knn_sqdist, mask, link_sq_dist: float, concavity: float, min_points: int = 1,
                    absorb_rounds: int = 8) -> ConvexClusters:
    """points and ORIENTED normals f32 [V,3], the table of ``knn_points`` and a mask int32 [V] -> ``ConvexClusters``: clusters that are
    cut where two bodies meet in a CONCAVE junction (include/vlsat_convex.h, vlsat_convex_clusters; the local-convexity criterion of
    Stein et al., CVPR 2014).  A table entry is concave when c = n_i . d - n_j . d > 0 for d = x_j - x_i and c^2 > ``concavity``^2 x
    its squared distance -- ``concavity`` is the sine of the tolerated concave angle.  Both ends of a concave entry are eroded; the
    remaining oriented points are clustered along the entries within ``link_sq_dist`` (a SQUARED distance), components of fewer than
    ``min_points`` are dissolved, and in ``absorb_rounds`` (0 .. 64) rounds every unlabelled point takes the label of the first labelled
    entry of its row, all points at once.  Device tensors run the HIP kernels (8 + ``absorb_rounds`` launches, nothing read back); CPU
    tensors or arrays run ``convex_clusters_host`` and get CPU tensors, with equal bits."""
    if not (isinstance(knn_index, torch.Tensor) and knn_index.is_cuda):
        as_np = lambda x: x.numpy() if isinstance(x, torch.Tensor) else x   # noqa: E731
        out = convex_clusters_host(as_np(points), as_np(normals), as_np(knn_index), as_np(knn_sqdist), as_np(mask), link_sq_dist, concavity,
                                   min_points, absorb_rounds)
        return ConvexClusters(*(torch.from_numpy(x) for x in out))
    lib = L.load()
    tau = _convex_args(points.shape, normals.shape, knn_index.shape, knn_sqdist.shape, mask.shape, link_sq_dist, concavity, min_points,
                       absorb_rounds)
    dev = knn_index.device
    points = points.to(device=dev, dtype=torch.float32).contiguous()
    normals = normals.to(device=dev, dtype=torch.float32).contiguous()
    index = knn_index.to(dtype=torch.int32).contiguous()
    sqdist = knn_sqdist.to(device=dev, dtype=torch.float32).contiguous()
    mask = (mask.to(device=dev) != 0).to(torch.int32).contiguous()
    v, k = index.shape
    scratch = torch.empty(int(lib.vlsat_convex_clusters_scratch_bytes(v)), dtype=torch.uint8, device=dev)
    labels = torch.empty(v, dtype=torch.int32, device=dev)
    n_clusters = torch.empty(1, dtype=torch.int32, device=dev)
    cluster_size = torch.empty(v, dtype=torch.int32, device=dev)
    state = torch.empty(v, dtype=torch.int32, device=dev)
    L.check(lib.vlsat_convex_clusters(points.data_ptr(), normals.data_ptr(), index.data_ptr(), sqdist.data_ptr(), mask.data_ptr(), v, k,
                                      float(link_sq_dist), float(tau), int(min_points), int(absorb_rounds), scratch.data_ptr(),
                                      labels.data_ptr(), n_clusters.data_ptr(), cluster_size.data_ptr(), state.data_ptr(), L.stream_ptr()))
    return ConvexClusters(labels, n_clusters, cluster_size, state)
