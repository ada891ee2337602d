"""The C ABI and its ctypes binding, every header of lib.HEADERS at once and without a GPU: the names a header declares are the names its
table binds and the library exports, no function is in two tables or declared twice, the name sets and argument counts are the pinned
ones, every table entry agrees with the C declaration it binds in count and kind of the parameters and in the return type, the headers
are in the source digest, and load() is strict for the in-tree library and lenient for another build."""
import ctypes as C
import hashlib
import os
import re
import shutil

import pytest

import vlsat_amd  # noqa: F401


@pytest.fixture(scope="module")
def L():
    from vlsat_amd import build as B, lib
    B.build()                      # hipcc cross-compiles gfx950 without a GPU
    return lib


# A new header is a row here, a new function a name in its row.
PINNED_NAMES = {key: set(names.split()) for key, names in {
    "vlsat": """vlsat_last_error vlsat_version vlsat_create vlsat_destroy vlsat_load_weight vlsat_finalize_weights vlsat_plan_create
        vlsat_plan_destroy vlsat_plan_info vlsat_plan_check_graph vlsat_forward vlsat_forward_train vlsat_set_gemm_precision
        vlsat_set_edge_attention_scope vlsat_profile_enable vlsat_profile_num_classes vlsat_profile_class_name vlsat_profile_read
        vlsat_k_gemm vlsat_k_split_bf16 vlsat_k_gemm_planes vlsat_k_gemm_bf16 vlsat_k_pointnet vlsat_k_flash_attn vlsat_k_flash_attn_bf16
        vlsat_k_layernorm vlsat_k_edge_gate vlsat_k_aggregate vlsat_k_node_attn vlsat_k_dist_bias vlsat_k_pointnet_ex vlsat_k_layernorm_to
        vlsat_k_edge_embed vlsat_k_desc_tail vlsat_k_row_invnorm vlsat_k_copy_rows vlsat_k_pts_conv1_rows vlsat_k_rowmax vlsat_k_apply_stn
        vlsat_prepare_objects vlsat_fc_edges vlsat_sample_objects_scratch vlsat_sample_objects vlsat_instance_boxes
        vlsat_proximity_lds_boxes vlsat_proximity_scratch_bytes vlsat_proximity_count vlsat_proximity_fill
        vlsat_nearest_points_scratch_bytes vlsat_nearest_points vlsat_segment_overlap_scratch_bytes vlsat_segment_overlap
        vlsat_merge_segments_scratch_bytes vlsat_merge_segments vlsat_k_softmax_rows vlsat_eval_ranks vlsat_eval_ranks_scratch_floats
        vlsat_eval_counts vlsat_eval_recallk vlsat_eval_recallk_scratch_bytes vlsat_process_val_counts vlsat_eval_triplet_split
        vlsat_process_val_counts_split vlsat_scene_graph_topk vlsat_scene_graph_scratch_bytes vlsat_k_exp vlsat_forward_scene_graph
        vlsat_graph_decode vlsat_graph_decode_scratch_bytes vlsat_graph_decode_counts vlsat_forward_graph vlsat_scene_checksums
        vlsat_comm_unique_id vlsat_comm_init vlsat_metrics_allreduce vlsat_comm_destroy vlsat_debug_gemm_clock_probe vlsat_debug_option
        vlsat_debug_stop_after vlsat_debug_read vlsat_debug_buffer""",
    "split": "vlsat_split_seeds vlsat_split_seeds_scratch_bytes vlsat_split_groups vlsat_fuse_splits vlsat_fuse_splits_scratch_bytes",
    "calib": "vlsat_score_hist vlsat_score_hist_geometry",
    "segment": "vlsat_segment_mesh vlsat_segment_mesh_scratch_bytes",
    "cloud": "vlsat_cloud_knn_scratch_bytes vlsat_cloud_knn vlsat_cloud_normals vlsat_segment_cloud",
    "voxel": "vlsat_voxel_scratch_bytes vlsat_voxel_assign vlsat_voxel_reduce",
    "objects": "vlsat_cloud_planes_scratch_bytes vlsat_cloud_planes vlsat_cloud_clusters_scratch_bytes vlsat_cloud_clusters",
    "flash": "vlsat_k_flash_attn_f16x3",
    "convex": "vlsat_convex_clusters_scratch_bytes vlsat_convex_clusters",
    "gemm": "vlsat_k_split_f16s vlsat_k_gemm_f16s",
}.items()}

PINNED_ARGUMENT_COUNTS = {
    "vlsat_merge_segments": 28, "vlsat_score_hist": 14, "vlsat_scene_graph_topk": 17, "vlsat_forward_scene_graph": 17,
    "vlsat_graph_decode": 22, "vlsat_forward_graph": 25, "vlsat_graph_decode_counts": 12, "vlsat_segment_mesh": 11,
    "vlsat_fuse_splits": 26, "vlsat_split_seeds": 11, "vlsat_convex_clusters_scratch_bytes": 1, "vlsat_convex_clusters": 17,
    "vlsat_cloud_knn_scratch_bytes": 2, "vlsat_cloud_knn": 9, "vlsat_cloud_normals": 13, "vlsat_segment_cloud": 12,
    "vlsat_voxel_scratch_bytes": 1, "vlsat_voxel_assign": 13, "vlsat_voxel_reduce": 12,
    "vlsat_cloud_planes_scratch_bytes": 2, "vlsat_cloud_planes": 14, "vlsat_cloud_clusters_scratch_bytes": 1, "vlsat_cloud_clusters": 12,
}


def _code(path):
    """the header's text without comments and preprocessor lines"""
    txt = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    return re.sub(r"^[ \t]*#[^\n]*", " ", txt, flags=re.M)


def _declarations(path):
    """[(name, return type, [parameter, ...])] of every `type name(params);` of the header"""
    found = re.findall(r"((?:const\s+)?[A-Za-z_]\w*[\s*]*?)\s*\b(vlsat_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _code(path))
    return [(name, " ".join(ret.split()), [] if params.strip() in ("", "void") else [" ".join(p.split()) for p in params.split(",")])
            for ret, name, params in found]


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "uint64_t": C.c_uint64}


def _agrees(c_type, ctype):
    """does the ctypes type stand for the C type (a return type, or a parameter with or without its name)?"""
    words = [w for w in re.findall(r"\w+|\*|\[", c_type) if w != "const"]
    if "*" in words or "[" in words or words[0] in ("vlsat_handle", "vlsat_plan"):
        return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
    if words[0] == "void":
        return ctype is None
    return ctype is not None and ctype is _SCALARS.get(words[0])         # a C type this table does not know agrees with nothing


def test_names_of_every_header_are_declared_bound_and_exported(L):
    lib = L.load()
    assert list(L.HEADERS) == ["vlsat", "split", "calib", "segment", "cloud", "voxel", "objects", "flash", "convex", "gemm"]
    for key in L.HEADERS:
        names = L.declared_symbols(key)
        assert set(names) == set(L.signatures(key)), f"lib.py's table and include/{L.HEADERS[key].file} disagree"
        for n in names:
            assert hasattr(lib, n), f"libvlsat_hip.so does not export {n}"
            assert getattr(lib, n).argtypes is not None, f"load() did not apply the table to {n}"
    assert b"gfx950" in lib.vlsat_version()


def test_tables_are_pairwise_disjoint(L):
    keys = list(L.HEADERS)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not set(L.signatures(a)) & set(L.signatures(b)), (a, b)
            assert not set(L.declared_symbols(a)) & set(L.declared_symbols(b)), (a, b)
    merged = L.signatures()
    assert len(merged) == sum(len(L.signatures(k)) for k in keys) and list(merged) == [n for k in keys for n in L.signatures(k)]


def test_every_function_is_declared_exactly_once(L):
    code = "\n".join(_code(L.header_path(k)) for k in L.HEADERS)
    for n in L.signatures():
        assert len(re.findall(r"\b" + n + r"\s*\(", code)) == 1, n
    declared = [d[0] for k in L.HEADERS for d in _declarations(L.header_path(k))]
    assert sorted(declared) == sorted(L.signatures())
    # a small header's functions are not so much as mentioned in vlsat.h's text, and are named in their own
    main = open(L.header_path("vlsat")).read()
    for n in PINNED_NAMES["split"]:
        assert n in open(L.header_path("split")).read() and n not in main, n
    # the whole text, comments included, opens the call's parenthesis once: the rules above it speak of the function without one
    for key, n in (("voxel", "vlsat_voxel_assign"), ("objects", "vlsat_cloud_planes"), ("convex", "vlsat_convex_clusters")):
        assert open(L.header_path(key)).read().count(n + "(") == 1, n


def test_pinned_names(L):
    assert {k: set(L.signatures(k)) for k in L.HEADERS} == PINNED_NAMES
    assert len(PINNED_NAMES["vlsat"]) == len(L.declared_symbols()) == 81
    assert sum(len(v) for v in PINNED_NAMES.values()) == len(L.signatures()) == 106


def test_pinned_argument_counts(L):
    sig = L.signatures()
    assert {n: len(sig[n][1]) for n in PINNED_ARGUMENT_COUNTS} == PINNED_ARGUMENT_COUNTS
    # the arguments of vlsat_k_gemm plus p8_part_min
    assert sig["vlsat_k_gemm_f16s"][1] == sig["vlsat_k_gemm"][1][:-1] + [C.c_int32, C.c_void_p]


def test_signatures_match_the_declarations(L):
    """Every table entry against the C declaration it binds: as many argtypes as parameters; position by position a pointer type
    (c_void_p, c_char_p, POINTER(...)) for a `*` parameter or a handle, and the ctypes type of the same name for int / int32_t, int64_t,
    float, double, size_t / uint64_t; the same for the return type, void being None.  Kinds only: what a pointer points to is not compared.  A wrong
    count or kind on a call that takes device pointers is memory corruption, and no other test holds the table to the header."""
    sig, seen = L.signatures(), 0
    for key in L.HEADERS:
        for name, ret, params in _declarations(L.header_path(key)):
            res, args = sig[name]
            assert len(params) == len(args), (name, len(params), len(args))
            for i, (p, a) in enumerate(zip(params, args)):
                assert _agrees(p, a), (name, i, p, a)
            assert _agrees(ret, res), (name, ret, res)
            seen += 1
    assert seen == len(sig)
    # the parser itself: what it makes of the forms the headers use
    assert _agrees("const float* points", C.c_void_p) and _agrees("const VlsatDims* dims", C.POINTER(L.VlsatDims))
    assert _agrees("const char* name", C.c_char_p) and _agrees("vlsat_plan p", C.c_void_p) and _agrees("void** comm", C.POINTER(C.c_void_p))
    assert not _agrees("int64_t n", C.c_int32) and not _agrees("float x", C.c_double) and not _agrees("int32_t k", C.c_void_p)
    assert not _agrees("void* stream", C.c_int64) and not _agrees("void", C.c_int) and not _agrees("int", None) and not _agrees("unsigned n", C.c_uint)


def test_headers_are_in_the_source_digest(L):
    files = L.source_files()
    for key in L.HEADERS:
        path = L.header_path(key)
        assert path.endswith("include/vlsat.h" if key == "vlsat" else f"include/vlsat_{key}.h") and files.count(path) == 1, path
    tail = len(L.HEADERS) + 1                      # after csrc/: the headers in registry order, then build.py
    assert files[-tail:] == [L.header_path(key) for key in L.HEADERS] + [os.path.join(os.path.dirname(L.__file__), "build.py")]
    csrc = files[:-tail]
    assert csrc == sorted(csrc) and {os.path.dirname(f) for f in csrc} == {os.path.join(os.path.dirname(L.__file__), "csrc")}
    assert sorted(os.path.basename(f) for f in csrc) == sorted(f for f in os.listdir(os.path.dirname(csrc[0])) if f.endswith((".hip", ".h")))
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0" + open(f, "rb").read())
    ident = L.identity()
    assert ident["source_sha256"] == h.hexdigest() and len(ident["source_sha256"]) == 64 and set(ident) == {"lib_sha256", "lib_bytes", "source_sha256"}


def test_load_is_strict_in_tree_and_lenient_for_another_build(L, tmp_path, monkeypatch):
    """A name in a table that the library does not export: the in-tree library refuses to load; a library from another path (bench.py --lib)
    loads, binds what it has and leaves that name unbound."""
    L.load()
    monkeypatch.setitem(L.HEADERS["cloud"].signatures, "vlsat_no_such_entry_point", (C.c_int, [C.c_void_p]))
    monkeypatch.setattr(L, "_lib", None)
    with pytest.raises(AttributeError):
        L.load()
    assert L._lib is None
    other = shutil.copy(L.LIB_PATH, tmp_path / "libvlsat_hip_other.so")
    monkeypatch.setattr(L, "LIB_PATH", str(other))
    lib = L.load()
    assert lib is L._lib and lib._name == str(other)
    assert lib.vlsat_cloud_knn.argtypes == L.signatures("cloud")["vlsat_cloud_knn"][1] and b"gfx950" in lib.vlsat_version()
    with pytest.raises(AttributeError):
        lib.vlsat_no_such_entry_point
