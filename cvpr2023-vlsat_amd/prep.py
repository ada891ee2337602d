"""Input preparation on the GPU: host-side mirror of the per-object part of
``SSGDatasetGraph.data_preparation`` (reference ``src/dataset/dataset_3dssg.py:279-294``), of the
fully-connected edge list (``:264-266``) and of ``collate_fn_mmg`` (``src/dataset/DataLoader.py:153-176``).
The selection of an object's points (``np.where(instances == id)`` + ``np.random.choice``, ``:285-289``) runs on the device too
(``sample_objects``): its index lists are np.where's, its draws come from a documented counter-based generator, not numpy's."""
from __future__ import annotations

from typing import Sequence

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
