"""ctypes binding of libvlsat_hip.so (C ABI in include/vlsat.h and the include/vlsat_*.h beside it: the registry HEADERS).

The library is loaded from this directory (built in-tree by ``build.py``).  There is no
fallback: if it is missing, ``load()`` raises -- the product path never computes on the CPU.
torch must be imported first so that the HIP runtime already mapped by torch
(``libamdhip64.so.7``) is the one this library binds to (one runtime, one set of streams).
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import re

import torch  # noqa: F401  (maps libamdhip64 before our library is loaded)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvlsat_hip.so")
_IN_TREE_LIB_PATH = LIB_PATH
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")


class VlsatDims(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("n_heads", C.c_int32), ("dim_atten", C.c_int32),
                ("gcn_aggr", C.c_int32), ("dim_point", C.c_int32), ("n_obj_class", C.c_int32),
                ("n_rel_class", C.c_int32), ("obj_logit_scale", C.c_float), ("use_gcn_edge", C.c_int32),
                ("multi_rel_outputs", C.c_int32), ("feature_transform", C.c_int32)]


class VlsatError(RuntimeError):
    pass


_lib = None
_vp, _i32, _i64, _f32, _sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t

# The public C ABI, stated once: one row per header of include/ -- its file name and {function: (restype, argtypes)}.  Paths, declared
# names, the source digest, what load() binds and what build() checks all follow from it; a new header is a new row.
Header = collections.namedtuple("Header", "file signatures")
HEADERS = {}

# include/vlsat.h: the forward, its plans and weights, the kernels' test entries, evaluation, graphs and preparation (csrc/engine_api.hip and others)
HEADERS["vlsat"] = Header("vlsat.h", {
    "vlsat_last_error": (C.c_char_p, []),
    "vlsat_version": (C.c_char_p, []),
    "vlsat_create": (C.c_int, [C.POINTER(VlsatDims), C.POINTER(_vp)]),
    "vlsat_destroy": (None, [_vp]),
    "vlsat_load_weight": (C.c_int, [_vp, C.c_char_p, _vp, _sz]),
    "vlsat_finalize_weights": (C.c_int, [_vp]),
    "vlsat_plan_create": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i32, C.POINTER(_vp)]),
    "vlsat_plan_destroy": (None, [_vp]),
    "vlsat_plan_info": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_sz), C.POINTER(_i32)]),
    "vlsat_plan_check_graph": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "vlsat_forward": (C.c_int, [_vp] * 9 + [_vp]),
    "vlsat_forward_train": (C.c_int, [_vp] * 12 + [_vp]),
    "vlsat_set_gemm_precision": (C.c_int, [_vp, _i32]),
    "vlsat_set_edge_attention_scope": (C.c_int, [_vp, _i32]),
    "vlsat_profile_enable": (C.c_int, [_vp, _i32]),
    "vlsat_profile_num_classes": (C.c_int, []),
    "vlsat_profile_class_name": (C.c_char_p, [_i32]),
    "vlsat_profile_read": (C.c_int, [_vp, _i32, C.POINTER(C.c_double), C.POINTER(_i64), C.POINTER(C.c_double)]),
    "vlsat_k_gemm": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _f32,
                               _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp]),
    "vlsat_k_split_bf16": (C.c_int, [_vp, _sz, _vp, _vp, _vp]),
    "vlsat_k_gemm_planes": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _f32,
                                      _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp]),
    "vlsat_k_gemm_bf16": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _f32,
                                    _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "vlsat_k_pointnet": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "vlsat_k_flash_attn": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _f32, _vp]),
    "vlsat_k_flash_attn_bf16": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _f32, _i32, _i32, _vp]),
    "vlsat_k_layernorm": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "vlsat_k_edge_gate": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32,
                                    _i32, _i32, _vp]),
    "vlsat_k_aggregate": (C.c_int, [_vp, _i32, _vp, _i64, _i32, _i32, _vp, _i32, _i32, _vp]),
    "vlsat_k_node_attn": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _f32, _i32, _vp]),
    "vlsat_k_dist_bias": (C.c_int, [_vp, _i32, _vp, _i32, _i32] + [_vp] * 10 + [_vp, _vp]),
    "vlsat_k_pointnet_ex": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "vlsat_k_layernorm_to": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    "vlsat_k_edge_embed": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "vlsat_k_desc_tail": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _vp]),
    "vlsat_k_row_invnorm": (C.c_int, [_vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp]),
    "vlsat_k_copy_rows": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i64, _vp]),
    "vlsat_k_pts_conv1_rows": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "vlsat_k_rowmax": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "vlsat_k_apply_stn": (C.c_int, [_vp, _i32, _vp, _i64, _i32, _vp, _i32, _vp]),
    "vlsat_prepare_objects": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "vlsat_fc_edges": (C.c_int, [_vp, _vp, _i32, _i64, _i64, _vp, _vp, _vp]),
    "vlsat_sample_objects_scratch": (_sz, [_i64, _i32]),
    "vlsat_sample_objects": (C.c_int, [_vp, _i64, _vp, _i32, _i32, C.c_uint64, _vp, _i32, _vp, _vp, _vp, _vp]),
    "vlsat_instance_boxes": (C.c_int, [_vp, _vp, _i64, _vp, _i32, _vp, _i32, _vp, _vp]),
    "vlsat_proximity_lds_boxes": (_i32, []),
    "vlsat_proximity_scratch_bytes": (_sz, [_i64]),
    "vlsat_proximity_count": (C.c_int, [_vp, _vp, _i32, _i64, _f32, _i32, _vp, _vp, _vp, _vp]),
    "vlsat_proximity_fill": (C.c_int, [_vp, _vp, _i32, _i64, _f32, _i32, _vp, _i64, _i64, _vp, _vp]),
    "vlsat_nearest_points_scratch_bytes": (_sz, [_i64, _i64]),
    "vlsat_nearest_points": (C.c_int, [_vp, _i64, _vp, _i64, _f32, _vp, _vp, _vp, _vp]),
    "vlsat_segment_overlap_scratch_bytes": (_sz, [_i32, _i32]),
    "vlsat_segment_overlap": (C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, C.c_double, C.c_double, _i32]
                              + [_vp] * 6 + [_vp]),
    "vlsat_merge_segments_scratch_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32]),
    "vlsat_merge_segments": (C.c_int, [_vp] * 5 + [_i32] * 6 + [_f32, _i32] + [_vp] * 14 + [_vp]),
    "vlsat_k_softmax_rows": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "vlsat_eval_ranks": (C.c_int, [_vp] * 6 + [_i32] * 7 + [_f32] + [_vp] * 5 + [_vp]),
    "vlsat_eval_ranks_scratch_floats": (C.c_int64, [_i32] * 3),
    "vlsat_eval_counts": (C.c_int, [_vp] * 10 + [_i32] * 4 + [_vp, _vp]),
    "vlsat_eval_recallk": (C.c_int, [_vp] * 6 + [_i32] * 6 + [_vp, _vp, _vp]),
    "vlsat_eval_recallk_scratch_bytes": (C.c_int64, [_i64, _i64, _i32, _i32, _i32]),
    "vlsat_process_val_counts": (C.c_int, [_vp] * 8 + [_i32, _vp, _vp]),
    "vlsat_eval_triplet_split": (C.c_int, [_vp] * 7 + [_i32] * 3 + [_vp, _vp]),
    "vlsat_process_val_counts_split": (C.c_int, [_vp] * 8 + [_i32, _vp, _vp, _vp, _vp]),
    "vlsat_scene_graph_topk": (C.c_int, [_vp] * 4 + [_i32] * 8 + [_vp] * 4 + [_vp]),
    "vlsat_scene_graph_scratch_bytes": (C.c_int64, [_i64, _i64, _i32, _i32, _i32, _i32, _i32]),
    "vlsat_k_exp": (C.c_int, [_vp, _i64, _vp, _vp]),
    "vlsat_forward_scene_graph": (C.c_int, [_vp] * 6 + [_i32] * 4 + [_vp] * 6 + [_vp]),
    "vlsat_graph_decode": (C.c_int, [_vp] * 5 + [_i32] * 9 + [_vp] * 7 + [_vp]),
    "vlsat_graph_decode_scratch_bytes": (C.c_int64, [_i64, _i32, _i32, _i32, _i32, _i32]),
    "vlsat_graph_decode_counts": (C.c_int, [_vp] * 5 + [_i32] * 5 + [_vp, _vp]),
    "vlsat_forward_graph": (C.c_int, [_vp] * 6 + [_i32] * 5 + [_vp] * 13 + [_vp]),
    "vlsat_scene_checksums": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "vlsat_comm_unique_id": (C.c_int, [_vp]),
    "vlsat_comm_init": (C.c_int, [_vp, _i32, _i32, C.POINTER(_vp)]),
    "vlsat_metrics_allreduce": (C.c_int, [_vp, _vp, _i32, _vp]),
    "vlsat_comm_destroy": (None, [_vp]),
    "vlsat_debug_gemm_clock_probe": (C.c_int, [_vp]),
    "vlsat_debug_option": (C.c_int, [_vp, C.c_char_p, _i32]),
    "vlsat_debug_stop_after": (C.c_int, [_vp, _i32]),
    "vlsat_debug_read": (C.c_int, [_vp, C.c_char_p, _vp, _i64]),
    "vlsat_debug_buffer": (C.c_int, [_vp, C.c_char_p, C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_i32),
                                     C.POINTER(_i32)]),
})

# include/vlsat_split.h: splitting a scan into sub-scenes and fusing the per-split graphs (csrc/scene_split.hip)
HEADERS["split"] = Header("vlsat_split.h", {
    "vlsat_split_seeds_scratch_bytes": (_sz, [_i64]),
    "vlsat_split_seeds": (C.c_int, [_vp, _i64, C.c_double, C.c_uint64, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "vlsat_split_groups": (C.c_int, [_vp, _vp, _i64, _vp, _i32, _vp, _i32, _vp, _i32, C.c_double, _i32, _vp, _vp, _vp, _vp]),
    "vlsat_fuse_splits_scratch_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32]),
    "vlsat_fuse_splits": (C.c_int, [_vp] * 5 + [_i32] * 5 + [_vp] * 15 + [_vp]),
})

# include/vlsat_calib.h: score histograms against ground truth, for thresholds and calibration (csrc/calibration.hip)
HEADERS["calib"] = Header("vlsat_calib.h", {
    "vlsat_score_hist": (C.c_int, [_vp] * 4 + [_i32] * 6 + [_vp] * 3 + [_vp]),
    "vlsat_score_hist_geometry": (None, [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
})

# include/vlsat_segment.h: an unlabelled mesh over-segmented into segments (csrc/mesh_segment.hip)
HEADERS["segment"] = Header("vlsat_segment.h", {
    "vlsat_segment_mesh_scratch_bytes": (_sz, [_i64, _i64]),
    "vlsat_segment_mesh": (C.c_int, [_vp, _vp, _i64, _i64, _f32, _i32, _vp, _vp, _vp, _vp, _vp]),
})

# include/vlsat_cloud.h: a cloud without faces -- kNN table, normals and flatness (csrc/cloud.hip), segments over the table (csrc/mesh_segment.hip)
HEADERS["cloud"] = Header("vlsat_cloud.h", {
    "vlsat_cloud_knn_scratch_bytes": (_sz, [_i64, _i32]),
    "vlsat_cloud_knn": (C.c_int, [_vp, _i64, _i32, _f32, _vp, _vp, _vp, _vp, _vp]),
    "vlsat_cloud_normals": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp]),
    "vlsat_segment_cloud": (C.c_int, [_vp, _vp, _i64, _i32, _f32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
})

# include/vlsat_voxel.h: a cloud resampled on a voxel grid -- cells and numbering, then means of positions, normals and colours (csrc/voxel.hip)
HEADERS["voxel"] = Header("vlsat_voxel.h", {
    "vlsat_voxel_scratch_bytes": (_sz, [_i64]),
    "vlsat_voxel_assign": (C.c_int, [_vp, _i64, _f32, _f32, _f32, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vlsat_voxel_reduce": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
})

# include/vlsat_objects.h: a cloud segmented into objects -- structural planes found and removed, the rest clustered (csrc/objects.hip)
HEADERS["objects"] = Header("vlsat_objects.h", {
    "vlsat_cloud_planes_scratch_bytes": (_sz, [_i64, _i32]),
    "vlsat_cloud_planes": (C.c_int, [_vp, _i64, _i32, _i32, _f32, _i32, _i32, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vlsat_cloud_clusters_scratch_bytes": (_sz, [_i64]),
    "vlsat_cloud_clusters": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _f32, _i32, _vp, _vp, _vp, _vp, _vp]),
})

# include/vlsat_flash.h: the split-fp16 edge attention of the fp32 precision mode on its own (csrc/flash_attn_bf16.hip)
HEADERS["flash"] = Header("vlsat_flash.h", {
    "vlsat_k_flash_attn_f16x3": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _f32, _i32, _i32, _vp]),
})

# include/vlsat_convex.h: clusters cut at concave junctions, for bodies that touch (csrc/convex.hip)
HEADERS["convex"] = Header("vlsat_convex.h", {
    "vlsat_convex_clusters_scratch_bytes": (_sz, [_i64]),
    "vlsat_convex_clusters": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _f32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
})

# include/vlsat_gemm.h: the split-fp16 8-phase GEMM of the fp32 precision mode on its own, and its weight planes (csrc/gemm_bf16_p8.hip)
HEADERS["gemm"] = Header("vlsat_gemm.h", {
    "vlsat_k_split_f16s": (C.c_int, [_vp, _sz, _vp, _vp, C.POINTER(_i32), _vp]),
    "vlsat_k_gemm_f16s": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _f32,
                                    _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
})


def header_path(name: str = "vlsat") -> str:
    return os.path.join(_INCLUDE, HEADERS[name].file)


def signatures(name=None) -> dict:
    """{function: (restype, argtypes)} of one header, or of all of them merged (no function is bound twice)."""
    if name is not None:
        return HEADERS[name].signatures
    merged = {}
    for h in HEADERS.values():
        assert not merged.keys() & h.signatures.keys(), (h.file, sorted(merged.keys() & h.signatures.keys()))
        merged.update(h.signatures)
    return merged


def declared_symbols(name: str = "vlsat") -> list:
    """Every function the header declares (parsed from its text)."""
    txt = open(header_path(name)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(vlsat_[a-z0-9_]+)\s*\(", txt)))


def source_files() -> list:
    """What the library is built from, in the order the source digest takes it: csrc/*.hip and *.h sorted, the headers in registry order,
    build.py (its flags and source list)."""
    csrc = os.path.join(_HERE, "csrc")
    return ([os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))]
            + [header_path(name) for name in HEADERS] + [os.path.join(_HERE, "build.py")])


def identity(lib_path: str = "") -> dict:
    """What a measurement was taken on: SHA-256 of the shared library that is (or would be) loaded and of the sources it is
    built from (source_files()) -- the GPU box has no .git, so the source digest is what a
    profile summary and a later bench run can compare; the commit is added when the summary is published (tools/)."""
    import hashlib
    path = lib_path or LIB_PATH
    out = {"lib_sha256": None, "lib_bytes": None, "source_sha256": None}
    if os.path.exists(path):
        out["lib_sha256"] = hashlib.sha256(open(path, "rb").read()).hexdigest()
        out["lib_bytes"] = os.path.getsize(path)
    h = hashlib.sha256()
    for fp in source_files():
        h.update(os.path.basename(fp).encode() + b"\0" + open(fp, "rb").read())
    out["source_sha256"] = h.hexdigest()
    return out


def load():
    """Load the shared library; raises VlsatError when it has not been built.  The in-tree library must export every bound name.  A
    library from another path (LIB_PATH reassigned: bench.py --lib, tools/pointnet_probe.py) is another build, loaded for a same-box A/B,
    and may predate any entry point: that one stays unbound, and calling it is an AttributeError."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VlsatError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(hipcc, gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in signatures().items():
        if LIB_PATH != _IN_TREE_LIB_PATH and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code: int) -> None:
    if code != 0:
        msg = load().vlsat_last_error().decode(errors="replace")
        err = VlsatError(f"libvlsat_hip error {code}: {msg}")
        err.code = code
        raise err


def ptr(t) -> int:
    """Raw device/host address of a torch tensor (None -> NULL)."""
    return 0 if t is None else t.data_ptr()


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream
