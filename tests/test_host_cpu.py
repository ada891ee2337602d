"""CPU-only tests of the host side: synthetic generators, weight inventory, the C-ABI library
(loads, argument validation that needs no GPU; its exports and signatures are test_c_abi_cpu.py's) and the
world_size-2 scene sharding over gloo."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, param_shapes, synth
from vlsat_amd import dist as vdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from vlsat_amd import build as B, lib
    B.build()                      # hipcc cross-compiles gfx950 without a GPU
    return lib


def test_param_inventory_counts():
    assert sum(int(np.prod(s)) for s in param_shapes(VLSATConfig(N_LAYERS=3)).values()) == 33_904_084
    two = param_shapes(VLSATConfig(N_LAYERS=2))
    assert two["mmg.gcn_3ds.1.edgeatten.nn_edge.0.weight"] == (1024, 1536)
    assert two["mmg.gcn_2ds.0.edgeatten.nn.3.weight"] == (32, 128, 1)
    assert "mmg.self_attn.2.attention.fc_q.weight" not in two


def test_synth_is_deterministic_and_well_formed():
    a, b = synth.make_weights(VLSATConfig()), synth.make_weights(VLSATConfig())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    s1, s2 = synth.make_scene(7, 33, 5), synth.make_scene(7, 33, 5)
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
    assert s1["obj_points"].shape == (7, 3, 33) and s1["edge_indices"].shape == (2, 42)
    assert np.abs(s1["obj_points"].mean(-1)).max() < 1e-5           # zero-meaned per object
    assert (s1["descriptor"][:, 6:] > 0).all()                       # logs are finite
    assert (s1["edge_indices"][0] != s1["edge_indices"][1]).all()
    assert (np.diff(s1["edge_indices"][0]) >= 0).all()               # source-major
    assert np.allclose(np.linalg.norm(s1["obj_2d_feats"], axis=-1), 1, atol=1e-5)
    bt = synth.collate([synth.make_scene(3, 8, 1), synth.make_scene(4, 8, 2)])
    assert bt["batch_ids"].ravel().tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert bt["edge_indices"][:, 6:].min() == 3 and bt["edge_indices"].shape[1] == 6 + 12


def _flash_release_rows():
    """the rows of the release part of the variant list of csrc/flash_pick.h, as tuples of the ten template arguments as nm prints them"""
    import re
    src = open(os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc", "flash_pick.h")).read()
    body = src[src.index("#define VLSAT_FLASH_BF16_RELEASE(X)"):src.index("// Experiments build only")]
    return [tuple(a.strip() for a in row.split(",")) for row in re.findall(r"\bX\(([^)]*)\)", body)]


def _gemm_release_rows(macro):
    """the rows of a release variant list of csrc/gemm_plan.h (the text between its #define and the next comment line), as tuples of strings"""
    import re
    src = open(os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc", "gemm_plan.h")).read()
    body = src[src.index("#define " + macro + "(X)"):]
    body = body[:body.index("\n//")]
    rows = [tuple(a.strip() for a in row.split(",")) for row in re.findall(r"\bX\(([^)]*)\)", body)]
    assert rows and len(rows) == len(set(rows)), (macro, rows)
    return rows


def test_release_library_carries_no_lab_code(L):
    """The in-tree build is the RELEASE library (csrc/common.h): no timing-ablation instantiation of the 8-phase GEMM (template
    argument ABL != 0 -- "results are garbage" by their own comment), and the lab switches of vlsat_debug_option are refused
    (they exist in `build.py --experiments` -> tools/bin/libvlsat_hip_exp.so only).  The bf16 edge attention: the instantiations in the
    library are exactly the release rows of the variant list of csrc/flash_pick.h (every row has a kernel, nothing else has), 26 of
    them, none with ABL != 0 or a ring of more than 2 tile buffers.  The GEMM: the instantiations of its four kernels are exactly the
    release rows of the four lists of csrc/gemm_plan.h -- 27 of gemm_p8_kernel, 30 of gemm_ring_kernel (none on 128 x 256 tiles: those 18
    are kernels of the experiments build), 193 of gemm_f32_kernel (34 rows on five tiles, 23 of them as a twin too), 20 of
    gemm_splitk_kernel (10 rows, single and twin)."""
    import re
    import shutil
    import subprocess
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-C", L.LIB_PATH], capture_output=True, text=True).stdout
    p8 = re.findall(r"gemm_p8_kernel<(\d+), (\d+), (?:true|false), (\d+), (\d+)>", out)
    assert p8, "nm shows no gemm_p8_kernel instantiation at all"
    assert all(abl == "0" for *_, abl in p8), sorted(set(p8))

    def built(kernel):
        return {tuple(a.split(", ")) for a in re.findall(kernel + r"<([^>]*)>", out)}
    p8_rows = {r + ("0",) for r in _gemm_release_rows("VLSAT_GEMM_P8_RELEASE")}
    ring_rows = set(_gemm_release_rows("VLSAT_GEMM_RING_RELEASE"))
    tiled = _gemm_release_rows("VLSAT_GEMM_TILED_VARIANTS")
    tiles = [("128", "128", "1"), ("128", "64", "1"), ("64", "128", "1"), ("64", "64", "1"), ("64", "64", "2")]
    tiled_rows = {(bm, bn, add, prec, ksl, "false") for add, prec, _ in tiled for bm, bn, ksl in tiles}
    tiled_rows |= {("64", "64", add, prec, "2", "true") for add, prec, twin in tiled if twin == "true"}
    sk_rows = {(prec, twin) for (prec,) in _gemm_release_rows("VLSAT_GEMM_SPLITK_VARIANTS") for twin in ("false", "true")}
    for kernel, rows, n in (("gemm_p8_kernel", p8_rows, 27), ("gemm_ring_kernel", ring_rows, 30), ("gemm_f32_kernel", tiled_rows, 193),
                            ("gemm_splitk_kernel", sk_rows, 20)):
        assert len(rows) == n, (kernel, len(rows))
        assert built(kernel) == rows, (kernel, sorted(built(kernel) - rows), sorted(rows - built(kernel)))
    assert all(r[3] == "128" for r in built("gemm_ring_kernel")), sorted(built("gemm_ring_kernel"))
    fa = {tuple(a.split(", ")) for a in re.findall(r"flash_attn_bf16_kernel<([^>]*)>", out)}
    rows = _flash_release_rows()
    assert len(rows) == len(set(rows)) == 26 and all(len(r) == 10 for r in rows), rows
    assert fa == set(rows), (sorted(fa - set(rows)), sorted(set(rows) - fa))
    assert all(r[7] == "0" and int(r[5]) <= 2 for r in fa), sorted(fa)
    src = open(os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc", "engine_api.hip")).read()
    lab = src[src.index("#ifdef VLSAT_EXPERIMENTS"):src.index("#else", src.index("#ifdef VLSAT_EXPERIMENTS"))]
    assert "flash_ablate" in lab and "gate_grid" in lab           # the lab switches sit behind the macro, not in the release path


def test_profile_stamps_and_stale_detection(L, tmp_path, monkeypatch):
    """roofline.traffic is evidence only if it was collected on the build that is running: profile summaries carry the digest of
    the sources and of the library (lib.identity()), and bench.committed_traffic() reports `stale` when the newest committed
    summary has another one (or none, like the summaries of rounds 1-4)."""
    import json
    sys.path.insert(0, ROOT)
    import bench
    ident = L.identity()
    assert ident["lib_sha256"] and len(ident["source_sha256"]) == 64 and ident == L.identity()
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    body = {"classes": {"gemm_f32": {"hbm_bytes_per_launch": 123.0}}}
    (prof / "r09_bench_pmc.json").write_text(json.dumps(body))
    assert bench.committed_traffic("cfg2", "fp32", "gemm_f32") == (123, "profiles/r09_bench_pmc.json", True)
    (prof / "r10_bench_pmc.json").write_text(json.dumps(dict(body, collected_on=ident)))
    assert bench.committed_traffic("cfg2", "fp32", "gemm_f32") == (123, "profiles/r10_bench_pmc.json", False)
    (prof / "r11_bench_pmc.json").write_text(json.dumps(dict(body, collected_on=dict(ident, source_sha256="0" * 64))))
    assert bench.committed_traffic("cfg2", "fp32", "gemm_f32")[2] is True


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the four outputs of the last timed step (float32) and the metrics vector (float64) as .npy files,
    whole when they fit the cap, otherwise the same seeded row sample on every run and within the cap."""
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    out = (torch.randn(80, 160, generator=g), torch.randn(80, 160, generator=g),
           torch.randn(3120, 26, generator=g), torch.randn(3120, 26, generator=g))
    metrics = torch.arange(9, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), out, metrics, 0, 1)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(n + ".npy" for n in bench.OUTPUT_NAMES + ("metrics",))
    for n, t in zip(bench.OUTPUT_NAMES, out):
        a = np.load(tmp_path / "a" / (n + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, t.numpy())
    m = np.load(tmp_path / "a" / "metrics.npy")
    assert m.dtype == np.float64 and np.array_equal(m, metrics.numpy())
    cap = 200_000
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", cap)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), out, metrics, 0, 1)
    total = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert total <= cap + 128 * 5                                    # (.npy headers)
    for n, t in zip(bench.OUTPUT_NAMES, out):
        b, c = np.load(tmp_path / "b" / (n + ".npy")), np.load(tmp_path / "c" / (n + ".npy"))
        assert 0 < b.shape[0] < t.shape[0] and b.shape[1:] == tuple(t.shape[1:]) and np.array_equal(b, c)
        assert all(any(np.array_equal(r, x) for x in t.numpy()) for r in b[:3])   # rows of the output, not something else


def test_c_abi_argument_validation_without_gpu(L):
    lib = L.load()
    h = C.c_void_p()
    good = L.VlsatDims(2, 8, 256, 0, 3, 160, 26, 2.6593, 1, 1, 0)
    for bad in (L.VlsatDims(0, 8, 256, 0, 3, 160, 26, 2.65), L.VlsatDims(2, 5, 256, 0, 3, 160, 26, 2.65),
                L.VlsatDims(2, 8, 250, 0, 3, 160, 26, 2.65),
                L.VlsatDims(2, 8, 256, 3, 3, 160, 26, 2.65), L.VlsatDims(2, 8, 256, 0, 5, 160, 26, 2.65)):
        assert lib.vlsat_create(C.byref(bad), C.byref(h)) == -1
        assert len(lib.vlsat_last_error()) > 0
    for ok in (L.VlsatDims(2, 4, 256, 0, 3, 160, 26, 2.65, 1, 1, 0), L.VlsatDims(2, 16, 512, 0, 3, 160, 26, 2.65, 1, 1, 0)):
        assert lib.vlsat_create(C.byref(ok), C.byref(h)) == 0        # NUM_HEADS in {4, 8, 16}, DIM_ATTEN a multiple of 4 H
        lib.vlsat_destroy(h)
    assert lib.vlsat_create(C.byref(good), C.byref(h)) == 0
    x = np.zeros(4, np.float32)
    assert lib.vlsat_load_weight(h, b"not.a.weight", x.ctypes.data, 4) == -1
    assert b"unknown weight" in lib.vlsat_last_error()
    assert lib.vlsat_load_weight(h, b"mmg.self_attn_fc.0.bias", x.ctypes.data, 4) == 0
    out = C.c_void_p()
    bid = np.zeros(3, np.int64)
    assert lib.vlsat_plan_create(h, bid.ctypes.data, None, 3, 0, 16, C.byref(out)) == -3    # weights not finalised
    with pytest.raises(L.VlsatError) as ei:
        L.check(lib.vlsat_forward(h, None, None, None, None, None, None, None, None, None))
    assert ei.value.code == -1
    lib.vlsat_destroy(h)


# Which gate kernel runs, written out by hand from the if-chain gcn_block had before gate_select existed (kernels.h).  "want16": the edge rows
# are in a 16-bit precision (terms 1 | 3) and "gate_bf16" is on.  Keys: (want16, gate_heads_mfma, gate_heads_bf16).
_GATE_SHIPPED_GEOMETRY = {           # 8 heads x DIM_ATTEN 256
    (0, 0, 0): "f32", (0, 0, 1): "f32", (0, 1, 0): "f32", (0, 1, 1): "f32", (0, 2, 0): "f32_heads", (0, 2, 1): "f32_heads",
    (1, 0, 0): "16", (1, 0, 1): "16", (1, 1, 0): "16", (1, 1, 1): "16", (1, 2, 0): "16", (1, 2, 1): "16_heads"}
_GATE_OTHER_GEOMETRIES = {
    (0, 0, 0): "valu", (0, 0, 1): "valu", (0, 1, 0): "f32_heads", (0, 1, 1): "f32_heads", (0, 2, 0): "f32_heads", (0, 2, 1): "f32_heads",
    (1, 0, 0): "valu", (1, 0, 1): "valu", (1, 1, 0): "f32_heads", (1, 1, 1): "16_heads", (1, 2, 0): "f32_heads", (1, 2, 1): "16_heads"}


def test_gate_select_chooses_what_the_forward_chose_before_it(L):
    """gate_select over every head geometry x precision x debug switch: the kernel of the hand-written tables above (with the one
    exception they do not show: no split-bf16 template at d_k = 128, so 4 heads with terms = 3 stay on the fp32 template), and only
    the two kernels of the shipped geometry offer the fused aggregation, a twin launch and row_map = 0.  Host code only: no device."""
    import gate_host
    rows = gate_host.run("select")
    assert len(rows) == 3 * 3 * 3 * 2 * 3 * 2
    seen = set()
    for left, right in rows:
        H, A, terms, bf16, hm, hb = (int(x) for x in left.split())
        kernel, fuse, twin, map0 = right.split()
        table = _GATE_SHIPPED_GEOMETRY if (H, A) == (8, 256) else _GATE_OTHER_GEOMETRIES
        want = table[int(terms != 0 and bf16 == 1), hm, hb]
        if want == "16_heads" and H == 4 and terms == 3:
            want = "f32_heads"
        assert kernel == want, (left, kernel, want)
        assert fuse == twin == map0 == ("1" if kernel in ("f32", "16") else "0"), (left, right)
        seen.add(kernel)
    assert seen == {"valu", "f32", "f32_heads", "16", "16_heads"}


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_select_core_integer_helpers_on_the_host(sanitize):
    """csrc/select_core.h compiled by g++: the float key round-trips bit for bit, is strictly monotone and positive over
    -inf .. +inf (denormals and both zeros included) and equals the formula proximity.hip / label_transfer.hip carried; count_ge
    equals a linear count on descending lists with repeats of lengths 0, 1, 2, 31, 32, 33; the dominance table of (100, 32) holds
    exactly the 1 365 triples with a b c <= 100, c <= 32.  The second case is the same stand-alone binary under ASan + UBSan."""
    import host_check
    rows = dict(host_check.lines("select_host_check", sanitize=sanitize))
    assert set(rows) == {"keys", "count_ge", "triples", "clampi"}, rows
    assert all(v.split()[0] == "ok" for v in rows.values()), rows
    assert rows["triples"] == "ok 1365"


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_evaluation_scratch_layout_on_the_host(sanitize):
    """csrc/engine.h's EvalScratch compiled by g++ (tests/eval_scratch_check.cpp): for (N, E, C, R) in (1, 0, 160, 26), (2, 2, 160, 26),
    (64, 4032, 160, 26), (3, 6, 20, 8) the carved regions are disjoint, in the order the entry points have always used, every element
    of every region is writable inside buffers of exactly the size functions' lengths, and those lengths equal 4 N C + 2 E' R + N C
    floats and 2 N + 4 E' R + 2 E' ints, E' = max(E, 1).  The second case is the same stand-alone binary under ASan + UBSan."""
    import host_check
    rows = dict(host_check.lines("eval_scratch_check", sanitize=sanitize))
    assert set(rows) == {"1 0 160 26", "2 2 160 26", "64 4032 160 26", "3 6 20 8"}, rows
    assert all(v == "ok" for v in rows.values()), rows


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_plan_graph_analyses_and_lays_out_what_plan_creation_did_before_it(sanitize):
    """csrc/plan_graph.h compiled by g++ (tests/plan_graph_check.cpp, which keeps the body vlsat_plan_create had before the header word for
    word, from the scene loop to the offset loop and the packing of the staging buffer): on every graph and configuration old and new code
    give the same packed index tables byte for byte, S, max_n, max_e, is_fc, fa_parts, tile counts, flash_flops (bit-equal), bias_total,
    the same buffers at the same offsets with the same sizes, R1 / R2, total, index_bytes, two-stream decision, kvx_slots and stn_ws_floats,
    and refuse the same graphs with the same code and text; no difference is permitted.  NUM_HEADS {4, 8, 16} x edge_scope x flash_split x
    dual_stream {0, 1, 2} x feature transform x 1..3 layers (all 216 on the small graphs, 72 or 28 of them on the large ones) over fully
    connected scenes of 1 .. 200 nodes, 9 + 40, the bench batch and E = 0; unsorted, pruned and one-edge-short lists; tile counts on both
    sides of the light-tile threshold (2048), of the key split (512; 2, 4, 9 and 16 parts; 1 .. 4 key tiles) and of the 256-query table (a
    scene one edge short of the minimum, 1016 / 1024 tiles, another minimum); nine refused graphs, four of them with two faults; one 64-node scene
    just under and just over the two-stream budget (1 566 372 edges); size classes from 1 byte to 64 GiB around every boundary and the pool
    pick on seven hand-made pools.  Small cases are carved in a host buffer of exactly `total` bytes and every region is written.  The
    program's workspace bytes for the graphs of tests/plan_cases.py are the recorded ones (the GPU test holds the library to them).  The
    second case is the same stand-alone binary under ASan + UBSan."""
    import plan_cases
    import host_check
    out = host_check.lines("plan_graph_check", sanitize=sanitize)
    rows = dict(r for r in out if len(r) == 2)
    assert set(rows) == {"fully connected", "not fully connected", "light tiles", "key split", "big tiles", "refused graphs", "budget", "size classes"}, rows
    assert all(v.split()[0] == "ok" and int(v.split()[1]) > 0 for v in rows.values()), rows
    assert rows["budget"] == "ok 2 cases, two streams up to 1566372 edges of one 64-node scene"
    ws = [r[0] for r in out if len(r) == 1]
    assert ws == [f"ws | {name} | {n}" for name, _, n in plan_cases.CASES], ws


@pytest.mark.parametrize("build", ["plain", "asan_ubsan", "experiments"])
def test_flash_pick_chooses_what_the_cascade_chose_before_it(build):
    """csrc/flash_pick.h compiled by g++ (tests/flash_pick_check.cpp): over head dim {32, 48, 64, 128} x terms {1, 2, 3} x use_tr 0..4 x
    io_split 0..3 x pv_terms {2, 3} x bq {128, 256} x qg {0, 1, 2} x parts {1, 2} x rows that fit or not (11 520 calls) flash_bf16_pick
    gives the ten template arguments and the block size, or the error text, of the if-cascade the launcher had before it (kept word
    for word in the check program).  The one permitted difference: the 24 calls with use_tr 3 | 4 that reached the ring-of-3 / ring-of-4
    kernels get the ring-of-2 kernel of use_tr 1 in the release list.  Every row of the list is reached, flash_attn_bf16_supports is
    the pick with the defaults and answers the engine as the hand-written rule did, the block is 64 x BQW.  "asan_ubsan": the same
    stand-alone binary under ASan + UBSan; "experiments": the list with the lab rows (12 more: rings of 3 and 4, ten ablations), the
    ablation values enumerated too, no difference permitted."""
    import host_check
    lab = build == "experiments"
    rows = dict(host_check.lines("flash_pick_check", sanitize=build == "asan_ubsan", defines=("VLSAT_EXPERIMENTS",) if lab else ()))
    assert set(rows) == {"legacy", "reachable", "supports", "block"}, rows
    assert all(v.split()[0] == "ok" for v in rows.values()), rows
    n = 13 if lab else 1
    assert rows["legacy"] == f"ok {11520 * n} cases, {1104 * n} launches, {0 if lab else 24} ring-of-2 for ring-of-3/4"
    assert rows["reachable"] == ("ok 38" if lab else "ok 26")
    assert rows["block"] == f"ok {38 if lab else 26} rows, 26 without ABL or a ring above 2"


@pytest.mark.parametrize("build", ["plain", "asan_ubsan", "experiments"])
def test_gemm_plan_chooses_what_the_launchers_chose_before_it(build):
    """csrc/gemm_plan.h compiled by g++ (tests/gemm_plan_check.cpp, which keeps the planner and the four launcher dispatches the library
    had before the lists word for word): whole launch sequences -- plan, tail, plan again -- of old and new code, compared launch by
    launch in family, rows, tile, k-slices per step, slot multiplier, split-K parts and slices, tiles, grid, block, kernel arguments and
    the kernel's template arguments; for refused problems the error text.  1 413 120 problems: G {512, 608, 8} x 12 M x 8 N x 8 K x two
    pitches of A x 8 operand formats = 36 864 shapes and formats, each with every other switch of the enumeration varied one at a time
    from the baseline (21 variations: 774 144); the switches that name a row varied together (additive mode 0..7 x ReLU-on-A x format of
    C x fp16 columns x no_dma x no_p8 = 576) over 60 shapes x 8 formats (276 480); and the planner's thresholds from both sides (M at
    every multiple of 64 up to 10 240 and one past it, around part_min / rem_min of each precision, N around the 64 x 128 rule's window,
    K = 192: 362 496).  Pairs: 2 027 520 twins that differ in nothing, in ReLU-on-A only, in one shape field, or share a workspace.  No
    difference is permitted.  Every row of every list is reached, and every twin form.  "asan_ubsan": the same stand-alone binary under
    ASan + UBSan; "experiments": the lists with the lab rows (13 ablations of the 8-phase kernel, 18 ring rows on 128 x 256 tiles) and
    ring_wide, ring_bk32, ring_nodb, force_tile 1..7 and ablate enumerated too.  The program also prints the launch sequences of the
    bench batch's shapes (the planner section)."""
    import host_check
    lab = build == "experiments"
    out = host_check.lines("gemm_plan_check", sanitize=build == "asan_ubsan", defines=("VLSAT_EXPERIMENTS",) if lab else ())
    rows = dict(r for r in out if len(r) == 2)
    assert set(rows) == {"legacy", "pairs", "reachable", "lists", "bench"}, rows
    assert all(v.split()[0] == "ok" for v in rows.values()), rows
    if not lab:
        assert rows["legacy"].startswith("ok 1413120 cases (774144 one switch at a time, 276480 operand products, 362496 thresholds)"), rows["legacy"]
    assert rows["pairs"].startswith("ok 2027520 pairs, "), rows["pairs"]
    assert rows["reachable"] == ("ok 8-phase 40, ring 48, persistent 34 (23 with a twin form), split-K 10" if lab else
                                 "ok 8-phase 27, ring 30, persistent 34 (23 with a twin form), split-K 10")
    assert rows["lists"] == ("ok 18 ring rows with 128 x 256 tiles, 13 ablations" if lab else "ok 0 ring rows with 128 x 256 tiles, 0 ablations")
    table = [r[0] for r in out if len(r) == 1 and r[0].startswith("table |")]
    assert len(table) == 3 * 9, table
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    if not lab:
        for line in table:
            assert line[len("table "):] in design, line          # the table in DESIGN.md is this program's output


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "cvpr2023-vlsat_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert "vlsat_oracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, f


def test_model_refuses_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vlsat_amd import lib as L
    from vlsat_amd.model import VLSATModel
    with pytest.raises(L.VlsatError):
        VLSATModel(VLSATConfig(), "cuda:0")
    with pytest.raises(L.VlsatError):
        VLSATModel(VLSATConfig(), "cpu")


def test_shard_is_a_balanced_partition():
    for n, w in ((512, 8), (64, 3), (5, 8), (0, 2)):
        parts = [vdist.shard(n, r, w) for r in range(w)]
        assert sorted(i for p in parts for i in p) == list(range(n))
        assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1


_WORKER = r"""
import os, sys, torch
sys.path.insert(0, os.environ["VLSAT_ROOT"])
import vlsat_amd
from vlsat_amd import VLSATConfig, synth, dist as vdist
from oracle import vlsat_oracle as O       # tests may use the oracle as the per-rank 'forward'
rank, local, world = vdist.init("gloo")
cfg = VLSATConfig(N_LAYERS=1)
w = O.to_torch(synth.make_weights(cfg))
mine = vdist.shard(5, rank, world)
b = {k: torch.from_numpy(v) for k, v in synth.collate([synth.make_scene(4, 16, 900 + s) for s in mine]).items()}
out = O.forward(w, cfg, b["obj_points"], b["obj_2d_feats"], b["edge_indices"], b["descriptor"], b["batch_ids"])
m = vdist.allreduce_metrics(vdist.scene_metrics(out, len(mine)))
t = vdist.max_over_ranks(float(rank + 1), torch.device("cpu"))
vdist.barrier()
if rank == 0:
    print("METRICS", " ".join(repr(float(x)) for x in m.tolist()), "MAXT", t)
"""


def test_two_rank_gloo_scene_sharding_matches_single_process(tmp_path):
    """world_size 2 over gloo: the all-reduced metrics vector equals the single-process one."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, VLSAT_ROOT=ROOT, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "29631", str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("METRICS")][0].split()
    got = np.array([float(x) for x in line[1:line.index("MAXT")]])
    assert float(line[-1]) == 2.0
    from oracle import vlsat_oracle as O
    cfg = VLSATConfig(N_LAYERS=1)
    w = O.to_torch(synth.make_weights(cfg))
    b = {k: torch.from_numpy(v) for k, v in synth.collate([synth.make_scene(4, 16, 900 + s) for s in range(5)]).items()}
    out = O.forward(w, cfg, b["obj_points"], b["obj_2d_feats"], b["edge_indices"], b["descriptor"], b["batch_ids"])
    ref = vdist.scene_metrics(out, 5).numpy()
    assert got[0] == 5 and got[1] == 20 and got[2] == 60
    assert np.allclose(got, ref, rtol=1e-9, atol=1e-6), (got, ref)
