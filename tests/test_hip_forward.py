"""Full-forward parity of the HIP path (through VLSATModel -> C ABI) against the CPU oracle and the
golden vectors made from the real reference.  Tolerance from BASELINE.json north_star: 1e-3 fp32
on the four outputs (two are logits scaled by 14.29, two are probabilities).  Needs an MI355X."""
import os

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-3          # the contract
TIGHT = 1e-4        # what an fp32 implementation should actually reach; catches subtle indexing bugs
NAMES = ("obj3d", "obj2d", "rel3d", "rel2d")


def _dev(b):
    return {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}


def _cpu(b):
    return {k: torch.from_numpy(v) for k, v in b.items()}


_MODELS = {}


def model_for(cfg):
    from vlsat_amd.model import VLSATModel
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    key = (cfg.N_LAYERS, cfg.GCN_AGGR, cfg.USE_GCN_EDGE, cfg.WITH_BN, cfg.multi_rel_outputs, cfg.dim_point, cfg.num_rel_class, cfg.feature_transform)
    if key not in _MODELS:
        _MODELS[key] = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    return _MODELS[key]


def run_hip(cfg, b):
    d = _dev(b)
    m = model_for(cfg)
    out = m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def run_oracle(cfg, b, taps=None, dtype=torch.float32):
    from oracle import vlsat_oracle as O
    w = O.to_torch(synth.make_weights(cfg), dtype)
    c = _cpu(b)
    return O.forward(w, cfg, c["obj_points"].to(dtype), c["obj_2d_feats"].to(dtype), c["edge_indices"],
                     c["descriptor"].to(dtype), c["batch_ids"], taps=taps)


def _check(got, ref, tol, what):
    errs = {}
    for n, g, r in zip(NAMES, got, ref):
        r = torch.as_tensor(r)
        assert g.shape == r.shape, (what, n, g.shape, r.shape)
        assert torch.isfinite(g).all(), f"{what} {n}: non-finite output"
        errs[n] = float((g - r.float()).abs().max()) if g.numel() else 0.0
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if v > tol}
    assert not bad, f"{what}: max-abs-err over {tol}: {bad}"
    return errs


# ------------------------------------------------------------------------------------------------
def test_staged_taps_cfg1():
    """Stop the forward after each stage and compare the workspace with the oracle's taps:
    localises a failure to one kernel in a single GPU run."""
    cfg = VLSATConfig(N_LAYERS=2)
    b = synth.make_batch(1, 8, 256, seed0=1000)
    taps = {}
    run_oracle(cfg, b, taps)
    d = _dev(b)
    m = model_for(cfg)
    n, p = 8, 256

    def stage(stage_id, buf):
        m.debug_stop_after(stage_id)
        try:
            m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])
            return m.debug_buffer(d["edge_indices"], d["batch_ids"], n, p, buf).cpu()
        finally:
            m.debug_stop_after(-1)

    def close(got, ref, name, tol=TIGHT):
        err = float((got - ref).abs().max())
        print(f"stage {name}: {err:.2e}")
        assert err < tol, f"stage {name}: max-abs-err {err:.3e}"

    close(stage(1, "F"), taps["obj_encoder"], "pointnet")
    close(stage(2, "X3"), taps["node_embed"], "node_embed")
    close(stage(3, "E3"), taps["rel_encoder_3d"], "rel_encoder_3d")
    close(stage(3, "E2"), taps["rel_encoder_2d"], "rel_encoder_2d")
    close(stage(4, "X2"), taps["clip_adapter"], "adapter")
    close(stage(10, "X3"), taps["self_attn0"], "self_attn0")
    close(stage(11, "X2"), taps["cross_attn0"], "cross_attn0")
    # the engine keeps the gated / aggregated channels head-major (h*32 + m); the reference order is m*8 + h
    ref_order = lambda t: t.view(t.shape[0], 8, 32).transpose(1, 2).reshape(t.shape[0], 256)
    close(ref_order(stage(12, "G")), taps["gcn3d0.gated"], "gate3d (head layout)")
    close(ref_order(stage(12, "AGG3")), taps["gcn3d0.agg"], "aggregate3d")
    close(stage(12, "E3"), taps["gcn3d0.edge"], "gcn3d edge")
    close(stage(12, "X3"), torch.relu(taps["gcn3d0.node"]), "gcn3d node (+inter-layer relu)")
    close(stage(13, "E2"), taps["gcn2d0.edge"], "gcn2d edge")
    close(stage(13, "X2"), torch.relu(taps["gcn2d0.node"]), "gcn2d node (+inter-layer relu)")
    close(stage(14, "E2"), torch.relu(taps["cross_attn_rel0"]), "edge cross-attention (+relu)")


def test_cfg1_golden_and_oracle(golden_dir):
    cfg = VLSATConfig(N_LAYERS=2)
    b = synth.make_batch(1, 8, 256, seed0=1000)
    got = run_hip(cfg, b)
    z = np.load(os.path.join(golden_dir, "cfg1_n8_p256_l2.npz"))
    _check(got, [z[n] for n in NAMES], TIGHT, "cfg1 vs reference golden")
    _check(got, run_oracle(cfg, b, dtype=torch.float64), TIGHT, "cfg1 vs fp64 oracle")


def test_cfg2_scene_golden(golden_dir):
    cfg = VLSATConfig(N_LAYERS=3)
    b = synth.make_batch(1, 40, 256, seed0=1000)
    got = run_hip(cfg, b)
    z = np.load(os.path.join(golden_dir, "cfg2_n40_p256_l3.npz"))
    _check(got, [z[n] for n in NAMES], TOL, "cfg2 scene vs reference golden")
    _check(got, [z[n] for n in NAMES], 3e-4, "cfg2 scene vs reference golden (tight)")


def test_ragged_batch_golden(golden_dir):
    cfg = VLSATConfig(N_LAYERS=2)
    b = synth.collate([synth.make_scene(5, 64, 2000), synth.make_scene(7, 64, 2001)])
    got = run_hip(cfg, b)
    z = np.load(os.path.join(golden_dir, "ragged_n5_n7_p64_l2.npz"))
    _check(got, [z[n] for n in NAMES], TIGHT, "ragged 2-scene batch vs per-scene reference")


def test_reference_batch_mode_golden(golden_dir):
    """set_batch_mode('reference'): the multi-scene call exactly as Mmgnet.forward computes it (edge cross-attention
    over the whole batch) against the real reference's batched call; switching back restores the
    per-scene contract."""
    from vlsat_amd.model import VLSATModel
    cfg = VLSATConfig(N_LAYERS=2)
    b = synth.collate([synth.make_scene(5, 64, 2000), synth.make_scene(7, 64, 2001)])
    z = np.load(os.path.join(golden_dir, "ragged_n5_n7_p64_l2.npz"))
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    d = _dev(b)
    call = lambda: [o.cpu() for o in m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])]
    m.set_batch_mode("reference")
    _check(call(), [z["batched_" + n] for n in NAMES], TIGHT, "reference batch mode vs the reference's batched call")
    m.set_batch_mode("per_scene")
    _check(call(), [z[n] for n in NAMES], TIGHT, "back to per-scene")
    m.close()


@pytest.mark.parametrize("aggr", ["max", "add", "mean"])
def test_general_edges_golden(golden_dir, aggr):
    """Non fully-connected, unsorted edge list with an empty source segment; L=1 (ReLU applies)."""
    cfg = VLSATConfig(N_LAYERS=1, GCN_AGGR=aggr)
    z = np.load(os.path.join(golden_dir, "general_edges_n6_p32_l1.npz"))
    sc = synth.make_scene(6, 32, 3000)
    sc["edge_indices"] = z["edge_indices"]
    got = run_hip(cfg, synth.collate([sc]))
    _check(got, [z[f"{aggr}.{n}"] for n in NAMES], TIGHT, f"general edges / {aggr}")


@pytest.mark.parametrize("case", sorted(synth.SWITCH_CASES))
def test_config_switches_golden(golden_dir, case):
    """MODEL.WITH_BN / USE_GCN_EDGE=false / multi_rel_outputs=false (log_softmax, 27 classes) / USE_RGB+USE_NORMAL
    (9 point channels) and all of them together: ragged 2-scene batch against the real reference run with that
    switch (tests/golden/make_golden_switches.py), and against the oracle."""
    cfg = VLSATConfig(**synth.SWITCH_CASES[case])
    b = synth.collate(synth.switch_scenes(cfg))
    z = np.load(os.path.join(golden_dir, case + ".npz"))
    got = run_hip(cfg, b)
    _check(got, [z[n] for n in NAMES], TIGHT, f"{case} vs reference golden")
    _check(got, run_oracle(cfg, b), TIGHT, f"{case} vs oracle")


@pytest.mark.parametrize("seed", range(6))
def test_random_graphs_vs_oracle(seed):
    """Randomised batches: 1..5 scenes of 1..11 objects, random point counts, arbitrary edge lists (random subsets of
    all ordered pairs INCLUDING self loops and duplicate edges, in random order across scenes), all three aggregators."""
    g = np.random.default_rng(100 + seed)
    cfg = VLSATConfig(N_LAYERS=int(g.integers(1, 4)), GCN_AGGR=("max", "add", "mean")[seed % 3])
    n_pts = int(g.integers(2, 130))              # >= 2: the descriptor's unbiased std needs two points
    scenes = []
    for s in range(int(g.integers(1, 6))):
        n = int(g.integers(1, 12))
        sc = synth.make_scene(n, n_pts, 9000 + 10 * seed + s)
        pairs = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), 0).reshape(2, -1)      # with self loops
        k = int(g.integers(0, pairs.shape[1] + 3))
        pick = g.integers(0, pairs.shape[1], k) if k else np.zeros(0, np.int64)                          # with duplicates
        sc["edge_indices"] = np.ascontiguousarray(pairs[:, pick]).astype(np.int64).reshape(2, -1)
        scenes.append(sc)
    b = synth.collate(scenes)
    perm = g.permutation(b["edge_indices"].shape[1])
    b["edge_indices"] = np.ascontiguousarray(b["edge_indices"][:, perm])
    _check(run_hip(cfg, b), run_oracle(cfg, b), TIGHT, f"random graph batch #{seed} ({len(scenes)} scenes, E={len(perm)})")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16_mixed", "bf16x3_attn1", "fp16_mixed"])
def test_two_stream_mode_is_bit_identical(precision):
    """Two-stream plans run the forward on up to three lanes (engine_forward.hip): the dependency-exact schedule of round 5
    ("sched" = 1: 3D chain / 2D edge chain / 2D node chain, coupled by one event per data-flow edge, the 3D chain up to a layer
    ahead) and the fork / join schedule of round 4 ("sched" = 0).  Same kernels on the same data, so the outputs of both must be
    bit-identical to the single-stream schedule -- any difference is a race or a missing dependency.  30 scenes of 2-59 objects
    plus a 6-scene batch, every forward 3 times BACK TO BACK without a host wait (so that the next forward's 3D lane meets the
    previous one's tail), in every precision mode."""
    from vlsat_amd.model import VLSATModel
    cfg = VLSATConfig(N_LAYERS=3)
    w = synth.make_weights(cfg)
    single = VLSATModel(cfg, DEV).load_state(w).eval().set_gemm_precision(precision).debug_option("dual_stream", 0)
    exact = VLSATModel(cfg, DEV).load_state(w).eval().set_gemm_precision(precision).debug_option("sched", 1)
    forkjoin = VLSATModel(cfg, DEV).load_state(w).eval().set_gemm_precision(precision).debug_option("sched", 0)
    g = np.random.default_rng(7)
    batches = [_dev(synth.collate([synth.make_scene(int(g.integers(2, 60)), int(g.integers(8, 200)), 12000 + i)])) for i in range(30)]
    batches.append(_dev(synth.collate([synth.make_scene(int(n), 64, 12100 + j) for j, n in enumerate((40, 3, 17, 1, 58, 25))])))
    for i, b in enumerate(batches):
        args = (b["obj_points"], b["obj_2d_feats"], b["edge_indices"], b["descriptor"], b["batch_ids"])
        ref = [o.clone() for o in single(*args)]
        for name, m in (("exact", exact), ("fork/join", forkjoin)):
            outs = [[o.clone() for o in m(*args)] for rep in range(3)]
            torch.cuda.synchronize()
            for rep, got in enumerate(outs):
                for n, a, c in zip(NAMES, got, ref):
                    assert torch.equal(a, c), f"{name} batch {i} rep {rep} {n}: max diff {float((a - c).abs().max()):.3e}"
    for m in (single, exact, forkjoin):
        m.close()


def test_feature_transform_ragged_vs_oracle():
    """MODEL.feature_transform on a ragged batch: a single-object scene without edges, 100 points per object (not a
    multiple of anything), L=2, all four outputs against the oracle (which is pinned to the reference for this switch)."""
    cfg = VLSATConfig(N_LAYERS=2, feature_transform=True)
    b = synth.collate([synth.make_scene(1, 100, 13000), synth.make_scene(9, 100, 13001), synth.make_scene(3, 100, 13002)])
    _check(run_hip(cfg, b), run_oracle(cfg, b), TIGHT, "feature_transform ragged batch")


def test_edges_interleaved_across_scenes():
    """Edges not grouped by scene: the glue permutes them (VLSAT_EGRAPH path) and un-permutes
    the relation outputs."""
    cfg = VLSATConfig(N_LAYERS=2)
    b = synth.collate([synth.make_scene(6, 32, 4000), synth.make_scene(4, 32, 4001), synth.make_scene(9, 32, 4002)])
    perm = np.random.default_rng(0).permutation(b["edge_indices"].shape[1])
    b2 = dict(b)
    b2["edge_indices"] = np.ascontiguousarray(b["edge_indices"][:, perm])
    ref = run_oracle(cfg, b2)
    got = run_hip(cfg, b2)
    _check(got, ref, TIGHT, "interleaved edges")
    base = run_hip(cfg, b)
    assert float((got[2] - base[2][perm]).abs().max()) < 1e-5


def test_single_object_scene_and_no_edges():
    cfg = VLSATConfig(N_LAYERS=2)
    b = synth.collate([synth.make_scene(1, 32, 4100), synth.make_scene(3, 32, 4101)])
    got = run_hip(cfg, b)
    _check(got, run_oracle(cfg, b), TIGHT, "scene with one object (no edges)")


@pytest.mark.parametrize("n_obj,n_pts", [(1, 16), (2, 1), (3, 65), (9, 128)])
def test_degenerate_shapes(n_obj, n_pts):
    """Smallest graphs: a lone object (E = 0), two objects with ONE point each, odd point counts
    (128 is the shipped config's num_points, config/mmgnet.json:73)."""
    cfg = VLSATConfig(N_LAYERS=2)
    sc = synth.make_scene(n_obj, max(n_pts, 2), 4200 + n_obj)     # descriptor needs >= 2 raw points (unbiased std)
    if n_pts == 1:
        sc["obj_points"] = np.ascontiguousarray(sc["obj_points"][:, :, :1])
    b = synth.collate([sc])
    got = run_hip(cfg, b)
    assert got[2].shape == (n_obj * (n_obj - 1), 26)
    _check(got, run_oracle(cfg, b), TIGHT, f"{n_obj} objects x {n_pts} points")


def _per_scene_err(got, ref, S, N, E):
    """max-abs-err per scene over the four outputs: [S] tensor"""
    worst = torch.zeros(S)
    for g, r, rows in zip(got, ref, (N, N, E, E)):
        d = (g - r).abs().view(S, -1).max(1)[0]
        worst = torch.maximum(worst, d)
    return worst


def test_batch_independence_full_size(bench_batch_oracle):
    """cfg 2 at full batch size (64 scenes x 40 objects x 256 points, L=3): ALL 64 scenes against the fp32 oracle
    (which evaluates scene by scene, i.e. the block-diagonal contract of SURVEY F9), three of them also against
    themselves run alone, and scene 0 against the reference golden."""
    cfg, b, ref = bench_batch_oracle
    S, N, P = 64, 40, 256
    E = N * (N - 1)
    got = run_hip(cfg, b)
    for g in got:
        assert torch.isfinite(g).all()
    per = _per_scene_err(got, ref, S, N, E)
    print(f"64/64 scenes vs fp32 oracle: worst scene {int(per.argmax())} at {float(per.max()):.2e}, median {float(per.median()):.2e}")
    assert float(per.max()) < TIGHT, f"scenes over {TIGHT}: {torch.nonzero(per >= TIGHT).view(-1).tolist()}"
    for s in (0, 17, 63):
        one = run_hip(cfg, synth.make_batch(1, N, P, seed0=1000 + s))
        for name, g, o, rows in zip(NAMES, got, one, (N, N, E, E)):
            err = float((g[s * rows:(s + 1) * rows] - o).abs().max())
            assert err < 2e-5, f"scene {s} {name}: batched vs alone {err:.3e}"
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "cfg2_n40_p256_l3.npz"))
    _check([got[0][:N], got[1][:N], got[2][:E], got[3][:E]], [z[n] for n in NAMES], TOL, "batch-64 scene 0 vs golden")
    assert float(got[2].min()) >= 0 and float(got[2].max()) <= 1


def test_mid_size_scene_multi_tile():
    """70 objects x 100 points (ragged last point chunk), E = 4830: several flash-attention
    query tiles with a partial last one, several GEMM rounds; against the fp32 oracle."""
    cfg = VLSATConfig(N_LAYERS=2)
    b = synth.collate([synth.make_scene(70, 100, 7000), synth.make_scene(3, 100, 7001)])
    _check(run_hip(cfg, b), run_oracle(cfg, b), TIGHT, "70-object scene + 3-object scene")


def test_cfg5_large_scene_stress(golden_dir):
    """BASELINE configs[4]: 200 objects x 1024 points, dense graph E = 39 800, L = 3, one scene.
    Compared with the committed oracle subsample (tests/golden/make_golden_cfg5.py) plus
    size-independent properties."""
    cfg = VLSATConfig(N_LAYERS=3)
    z = np.load(os.path.join(golden_dir, "cfg5_n200_p1024_l3_sub.npz"))
    b = synth.make_batch(1, 200, 1024, seed0=5000)
    got = run_hip(cfg, b)
    idx = torch.from_numpy(z["edge_idx"])
    _check([got[0], got[1], got[2][idx], got[3][idx]], [z["obj3d"], z["obj2d"], z["rel3d"], z["rel2d"]], TOL,
           "cfg5 vs oracle subsample")
    for g in got:
        assert torch.isfinite(g).all()
    assert float(got[2].min()) >= 0 and float(got[2].max()) <= 1 and float(got[3].min()) >= 0 and float(got[3].max()) <= 1
    m = model_for(cfg)
    d = _dev(b)
    info = m.plan_info(d["edge_indices"], d["batch_ids"], 200, 1024)
    assert info["n_scenes"] == 1 and info["is_fc"] and info["workspace_bytes"] < 2 * 1024 ** 3   # O(E), not O(E^2)


def test_plan_layout_is_the_host_checked_one_and_key_split_changes_nothing():
    """The three graphs of tests/plan_cases.py: the library's plan has the workspace bytes that tests/plan_graph_check.cpp printed after
    holding csrc/plan_graph.h against the old plan creation (so the layout on the device is the verified one), the scene count and is_fc.
    An fp32 forward with "flash_split" 1 (the default: 16 key parts where there is an edge at all) is finite and equals the forward
    with "flash_split" 0 -- compared as tests/test_hip_round6.py compares its forwards around "flash_split": torch.equal.  (No scene here
    has more than three key tiles, so each uses one part of the plan's 16 and the merge multiplies by exp2(0) = 1.)"""
    import plan_cases
    cfg = VLSATConfig()
    m = model_for(cfg)
    for i, (name, sizes, ws_bytes) in enumerate(plan_cases.CASES):
        d = _dev(synth.collate([synth.make_scene(n, plan_cases.POINTS, 8800 + 10 * i + j) for j, n in enumerate(sizes)]))
        args = (d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])
        info = m.plan_info(d["edge_indices"], d["batch_ids"], sum(sizes), plan_cases.POINTS)
        assert info == {"n_scenes": len(sizes), "workspace_bytes": ws_bytes, "is_fc": True}, (name, info)
        def run():
            out = m(*args)
            torch.cuda.synchronize()
            return [o.clone() for o in out]
        split = run()
        try:
            m.debug_option("flash_split", 0)
            whole = run()
        finally:
            m.debug_option("flash_split", 1)
        for n, a, b in zip(NAMES, split, whole):
            assert torch.isfinite(a).all(), (name, n)
            print(name, n, float((a - b).abs().max()) if a.numel() else 0.0)
            assert torch.equal(a, b), (name, n, float((a - b).abs().max()))


def test_plan_cache_not_fooled_by_address_reuse():
    """Two different graphs with identical shapes: a plan must never be reused across them."""
    cfg = VLSATConfig(N_LAYERS=2)
    m = model_for(cfg)
    outs = []
    for seed in (6000, 6001):
        sc = synth.make_scene(6, 32, seed)
        g = np.random.default_rng(seed)
        keep = g.permutation(sc["edge_indices"].shape[1])[:20]
        sc["edge_indices"] = np.ascontiguousarray(sc["edge_indices"][:, keep])
        b = synth.collate([sc])
        got = run_hip(cfg, b)
        _check(got, run_oracle(cfg, b), TIGHT, f"graph seed {seed}")
        outs.append(got)
        del got
        torch.cuda.empty_cache()


def test_3d_only_path_is_bit_identical_and_faster():
    """forward_3d skips the 2D branch; its outputs must equal forward()'s 3D outputs bit for bit."""
    import time
    cfg = VLSATConfig(N_LAYERS=3)
    m = model_for(cfg)
    d = _dev(synth.make_batch(8, 40, 256, seed0=1000))
    full = m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])
    o3, r3 = m.forward_3d(d["obj_points"], d["edge_indices"], d["descriptor"], d["batch_ids"])
    torch.cuda.synchronize()
    assert torch.equal(o3, full[0]) and torch.equal(r3, full[2])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    t_full = timed(lambda: m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"]))
    t_3d = timed(lambda: m.forward_3d(d["obj_points"], d["edge_indices"], d["descriptor"], d["batch_ids"]))
    print(f"3D-only {t_3d / 5 * 1e3:.2f} ms vs full {t_full / 5 * 1e3:.2f} ms")
    assert t_3d < 0.7 * t_full


def test_errors_are_loud():
    from vlsat_amd import lib as L
    from vlsat_amd.model import VLSATModel
    cfg = VLSATConfig(N_LAYERS=2)
    m = model_for(cfg)
    d = _dev(synth.make_batch(1, 4, 32, seed0=1))
    with pytest.raises(L.VlsatError):          # istrain=True needs train_outputs=True + triplet_projector_2d weights
        m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"], istrain=True)
    with pytest.raises(L.VlsatError):
        m(d["obj_points"].cpu(), d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])
    with pytest.raises(L.VlsatError):
        m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], None, d["batch_ids"])
    bad = d["edge_indices"].clone()
    bad[1, 0] = 99
    with pytest.raises(L.VlsatError):
        m(d["obj_points"], d["obj_2d_feats"], bad, d["descriptor"], d["batch_ids"])
    fresh = VLSATModel(cfg, DEV)
    with pytest.raises(L.VlsatError):
        fresh(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])
    w = synth.make_weights(cfg)
    w.pop("mmg.gcn_2ds.1.prop.2.bias")
    with pytest.raises(L.VlsatError):
        fresh.load_state(w)


def test_cfg3_split_bf16_gemms(golden_dir):
    """BASELINE configs[2]: bf16 MFMA for the GEMMs, tolerance 1e-2.  The split-bf16 mode (3 MFMAs per
    product, fp32 accumulate) must meet it with a wide margin; the single-rounding bf16 mode is only
    required to be sane (it sits at ~2e-2 on the x14.29 object logits)."""
    from vlsat_amd.model import VLSATModel
    cfg = VLSATConfig(N_LAYERS=3)
    z = np.load(os.path.join(golden_dir, "cfg2_n40_p256_l3.npz"))
    b = synth.make_batch(1, 40, 256, seed0=1000)
    d = _dev(b)
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    try:
        m.set_gemm_precision("bf16x3")
        got = [o.cpu() for o in m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])]
        errs = _check(got, [z[n] for n in NAMES], 1e-2, "cfg3 bf16x3 vs reference golden")
        assert max(errs.values()) < 1e-3, errs                  # in practice fp32-tolerance too
        for mode, tol in (("bf16_mixed", 1e-2), ("bf16x3_attn1", 1e-2), ("fp16_mixed", 2e-3)):       # the faster modes against the same reference-made golden
            m.set_gemm_precision(mode)
            gm = [o.cpu() for o in m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])]
            _check(gm, [z[n] for n in NAMES], tol, f"cfg3 {mode} vs reference golden")
        m.set_gemm_precision("bf16")
        got1 = [o.cpu() for o in m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])]
        _check(got1, [z[n] for n in NAMES], 1e-1, "single-rounding bf16 vs reference golden (informational)")
        m.set_gemm_precision("fp32")
        got0 = [o.cpu() for o in m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])]
        _check(got0, [z[n] for n in NAMES], 3e-4, "back to fp32")
    finally:
        m.close()
    # ragged batch through the bf16x3 GEMM tails
    cfg2 = VLSATConfig(N_LAYERS=2)
    bb = synth.collate([synth.make_scene(5, 64, 2000), synth.make_scene(7, 64, 2001)])
    m2 = VLSATModel(cfg2, DEV).load_state(synth.make_weights(cfg2)).eval().set_gemm_precision("bf16x3")
    dd = _dev(bb)
    got2 = [o.cpu() for o in m2(dd["obj_points"], dd["obj_2d_feats"], dd["edge_indices"], dd["descriptor"], dd["batch_ids"])]
    zz = np.load(os.path.join(golden_dir, "ragged_n5_n7_p64_l2.npz"))
    _check(got2, [zz[n] for n in NAMES], 1e-3, "ragged batch bf16x3")
    m2.close()


@pytest.mark.parametrize("mode,tol", [("bf16x3", 1e-3), ("bf16_mixed", 1e-2), ("bf16x3_attn1", 1e-2), ("fp16_mixed", 2e-3)])
def test_cfg3_full_batch_all_scenes(bench_batch_oracle, mode, tol):
    """BASELINE configs[2] at the config's own batch (64 scenes x 40 x 256, L=3): every scene against the fp32 oracle.
    bf16x3 (three bf16 MFMAs per product) must stay inside the fp32 contract (1e-3); the mixed mode (single-rounded bf16
    on the edge-row matrix work, split-bf16 on node rows) inside the config's 1e-2."""
    from vlsat_amd.model import VLSATModel
    cfg, b, ref = bench_batch_oracle
    S, N = 64, 40
    E = N * (N - 1)
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval().set_gemm_precision(mode)
    try:
        d = _dev(b)
        got = [o.cpu() for o in m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])]
        per = _per_scene_err(got, ref, S, N, E)
        errs = {n: float((g - r).abs().max()) for n, g, r in zip(NAMES, got, ref)}
        print(f"{mode}: 64/64 scenes, worst scene {int(per.argmax())} at {float(per.max()):.2e}, per output {errs}")
        assert float(per.max()) < tol, f"{mode}: scenes over {tol}: {torch.nonzero(per >= tol).view(-1).tolist()}"
        # the same with every experiment switch of the bf16 modes turned off one at a time (fp32 tensors between the
        # kernels, fp32 attention, gather instead of the LDS transpose read): same contract
        for opt in ("split_fmt", "flash_tr", "flash_bf16", "pointnet_bf16", "gate_bf16", "ln_resid", "gemm_splitk", "gemm_p8"):
            m.debug_option(opt, 0)
            alt = [o.cpu() for o in m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])]
            pa = _per_scene_err(alt, ref, S, N, E)
            print(f"{mode} with {opt}=0: worst scene at {float(pa.max()):.2e}")
            assert float(pa.max()) < (1e-2 if mode == "fp16_mixed" else tol), (mode, opt)      # (fp16_mixed without its tensor formats / kernels is bf16_mixed: that mode's contract)
            m.debug_option(opt, 1)
    finally:
        m.close()


@pytest.mark.parametrize("seed", range(4))
def test_random_graphs_bf16x3_vs_oracle(seed):
    """The bf16 kernels (GEMM pipes, attention, object encoder, gate) on randomised batches: 1..5 scenes of 1..11
    objects, odd point counts (partial 128-point chunks, objects split over several blocks), arbitrary edge lists with
    self loops / duplicates / empty scenes, every aggregator; split-bf16 must stay inside the fp32 contract."""
    from vlsat_amd.model import VLSATModel
    g = np.random.default_rng(400 + seed)
    cfg = VLSATConfig(N_LAYERS=int(g.integers(1, 4)), GCN_AGGR=("max", "add", "mean")[seed % 3])
    n_pts = int(g.integers(2, 300))
    scenes = []
    for s in range(int(g.integers(1, 6))):
        n = int(g.integers(1, 12))
        sc = synth.make_scene(n, n_pts, 9500 + 10 * seed + s)
        pairs = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), 0).reshape(2, -1)
        k = int(g.integers(0, pairs.shape[1] + 3))
        pick = g.integers(0, pairs.shape[1], k) if k else np.zeros(0, np.int64)
        sc["edge_indices"] = np.ascontiguousarray(pairs[:, pick]).astype(np.int64).reshape(2, -1)
        scenes.append(sc)
    b = synth.collate(scenes)
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval().set_gemm_precision("bf16x3")
    try:
        d = _dev(b)
        got = [o.cpu() for o in m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])]
        _check(got, run_oracle(cfg, b), TOL, f"bf16x3 random graph batch #{seed}")
    finally:
        m.close()


@pytest.mark.parametrize("case", ["switch_no_gcn_edge", "switch_rgb_normal", "switch_with_bn", "switch_single_rel"])
def test_config_switches_bf16x3(golden_dir, case):
    """The config switches that reach the bf16 kernels (gate without the edge half, 9 point channels, folded BN, log_softmax
    head) in split-bf16 mode against the real reference's goldens."""
    from vlsat_amd.model import VLSATModel
    cfg = VLSATConfig(**synth.SWITCH_CASES[case])
    b = synth.collate(synth.switch_scenes(cfg))
    z = np.load(os.path.join(golden_dir, case + ".npz"))
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval().set_gemm_precision("bf16x3")
    try:
        d = _dev(b)
        got = [o.cpu() for o in m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])]
        _check(got, [z[n] for n in NAMES], TOL, f"{case} in bf16x3 vs reference golden")
    finally:
        m.close()
