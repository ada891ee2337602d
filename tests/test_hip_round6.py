"""Round 6 on the device: switches added this round must not change results where they are pure re-orderings of memory traffic, and
must stay inside the parity tolerance where they re-order a floating-point sum.  Needs an MI355X."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, synth
from vlsat_amd.model import VLSATModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("obj3d", "obj2d", "rel3d", "rel2d")


def _batch(n_scenes, n_obj, n_pts, seed0):
    b = synth.make_batch(n_scenes, n_obj, n_pts, seed0=seed0)
    return b, {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}


def _run(m, d):
    out = m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])
    torch.cuda.synchronize()
    return [o.clone() for o in out]


@pytest.mark.parametrize("precision,tol", [("bf16_mixed", 1e-2), ("bf16x3", 1e-3), ("fp32", 1e-3)])
def test_k_tile_rotation_of_the_8_phase_gemm_stays_inside_the_tolerance(precision, tol):
    """"gemm_k_rot" r: column tile tn of a row panel walks its K-tiles starting at tn * r (the blocks that share an A panel then ask
    L2 for the same lines a K-tile apart instead of in the same microsecond; default since round 6: 1 for the half-row bf16
    launches, 0 elsewhere).  A rotation of the fp32 summation order: not bit-identical, but every output stays inside the mode's
    tolerance against the CPU oracle, on a batch large enough for the 8-phase kernel to take the edge-row launches (E >= 65536)."""
    from oracle import vlsat_oracle as O
    cfg = VLSATConfig(N_LAYERS=1)
    w = synth.make_weights(cfg)
    b, d = _batch(44, 40, 32, seed0=4200)                          # E = 68 640
    c = {k: torch.from_numpy(v) for k, v in b.items()}
    ref = O.forward(O.to_torch(w), cfg, c["obj_points"], c["obj_2d_feats"], c["edge_indices"], c["descriptor"], c["batch_ids"])
    outs = {}
    for r in (0, 1, 3):
        m = VLSATModel(cfg, DEV).load_state(w).eval().set_gemm_precision(precision).debug_option("gemm_k_rot", r)
        outs[r] = _run(m, d)
        m.close()
        for n, g, x in zip(NAMES, outs[r], ref):
            assert float((g.cpu() - x).abs().max()) < tol, (precision, r, n)
    if precision != "fp32":
        assert any(not torch.equal(x, y) for x, y in zip(outs[0], outs[1]))        # (the switch reaches the kernel)


PAIR_CASES = {
    "default": dict(N_LAYERS=3),
    "one_layer": dict(N_LAYERS=1),
    "aggr_add": dict(N_LAYERS=2, GCN_AGGR="add"),
    "aggr_mean": dict(N_LAYERS=2, GCN_AGGR="mean"),
    "no_gcn_edge": dict(N_LAYERS=2, USE_GCN_EDGE=False),
    "single_rel": dict(N_LAYERS=2, multi_rel_outputs=False, num_rel_class=27),
    "with_bn": dict(N_LAYERS=2, WITH_BN=True),
}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16_mixed", "bf16x3_attn1", "fp16_mixed"])
@pytest.mark.parametrize("case", sorted(PAIR_CASES))
def test_paired_schedule_of_one_scene_plans_is_bit_identical(precision, case):
    """One-scene plans (E <= "pair_max_edges") run the 3D / 2D twin stages -- relation encoders, gcn_3ds | gcn_2ds, both head pairs -- as
    launches of TWO problems each (engine_forward.hip: paired schedule; gemm_splitk / gemm_f32 / gate / aggregate kernels select the
    problem by blockIdx.y), with the edge cross-attention of layer l on the second lane under the node attentions of layer l + 1.
    Every block runs the single launch's code on its own problem, so the outputs must be BIT-IDENTICAL to the unpaired schedule
    ("pair_twins" 0) and to the single-stream one ("dual_stream" 0): scenes of 2..64 objects (E = 2 .. 4032), one isolated object (no
    edge: not paired), a ragged three-scene batch, every forward twice back to back (lane t of the second forward meets the first)."""
    if precision != "fp32" and case in ("with_bn",):
        pytest.skip("covered in fp32")
    cfg = VLSATConfig(**PAIR_CASES[case])
    w = synth.make_weights(cfg)
    mods = {k: VLSATModel(cfg, DEV).load_state(w).eval().set_gemm_precision(precision) for k in ("pair", "nopair", "single")}
    mods["pair"].debug_option("pair_twins", 1)
    mods["nopair"].debug_option("pair_twins", 0)
    mods["single"].debug_option("dual_stream", 0)
    graphs = [synth.make_batch(1, n, 32, seed0=4300 + n) for n in (2, 3, 5, 9, 17, 26, 40, 41, 57, 64)]
    graphs.append(synth.make_batch(1, 1, 32, seed0=4399))
    graphs.append(synth.collate([synth.make_scene(n, 32, 4400 + n) for n in (7, 1, 19)]))
    for b in graphs:
        d = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
        outs = {}
        for k, m in mods.items():
            first = m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])
            first = [o.clone() for o in first]
            second = m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])
            torch.cuda.synchronize()
            for x, y in zip(first, second):
                assert torch.equal(x, y), (k, "not reproducible call to call")
            outs[k] = first
        n = b["obj_points"].shape[0]
        for name, a, c, e in zip(NAMES, outs["pair"], outs["nopair"], outs["single"]):
            assert torch.isfinite(a).all(), (n, name)
            assert torch.equal(a, c), (precision, case, n, name, "paired vs unpaired", float((a - c).abs().max()) if a.numel() else 0.0)
            assert torch.equal(a, e), (precision, case, n, name, "paired vs one stream", float((a - e).abs().max()) if a.numel() else 0.0)
    for m in mods.values():
        m.close()


def test_paired_schedule_through_the_evaluation_loop():
    """The paired schedule inside vlsat_process_val_counts with several replicas in flight: the summary of a one-scene-per-call loop
    equals the reference-compatible loop's, as before."""
    from vlsat_amd import evaluate as EV
    cfg = VLSATConfig(N_LAYERS=2)
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    items = []
    for i, n in enumerate((9, 14, 33, 40, 21, 5, 60, 12)):
        b = synth.make_batch(1, n, 32, seed0=4500 + i)
        e = b["edge_indices"].shape[1]
        g = np.random.default_rng([n, 7])
        it = {k: torch.from_numpy(v).to(DEV) for k, v in b.items() if k != "edge_indices"}
        it.update(edge_indices=torch.from_numpy(b["edge_indices"]).t().contiguous().to(DEV), gt_class=torch.from_numpy(g.integers(0, 160, n)).to(DEV),
                  gt_rel_cls=torch.from_numpy((g.random((e, 26)) < 0.05).astype(np.int64)).to(DEV), fc_sizes=[n])
        items.append(it)
    ref = EV.validation(m, items, device=DEV, workers=0)
    for k in (1, 3):
        got = EV.validation(m, items, device=DEV, workers=k)
        assert got == ref, [q for q in ref if got[q] != ref[q]]
    m.close()


def test_fp16_node_tables_of_nn_edge_0():
    """"gather_f16": [P_i | P_j] of the node-side projection (the x_i and x_j parts of nn_edge's first Linear, reference
    network_MMG.py:59-60,92, hoisted to node rows) stored as fp16 half rows and gathered per edge by nn_edge.0 -- default in the
    single-rounding modes, off in the split-bf16 ones, never in fp32.  Against the CPU oracle on a batch that takes the 8-phase kernel
    (E = 68 640) and on one-scene plans (the paired schedule's twin launches): bf16_mixed stays inside 1e-2 with and without, the two differ
    (the switch reaches the kernels) by less than the tolerance; bf16x3's default equals "off" bit for bit and its forced "on" stays inside
    1e-3; fp32 ignores the switch bit for bit."""
    from oracle import vlsat_oracle as O
    cfg = VLSATConfig(N_LAYERS=2)
    w = synth.make_weights(cfg)
    cases = [_batch(44, 40, 32, seed0=4500), _batch(1, 26, 32, seed0=4501), _batch(1, 1, 32, seed0=4502)]
    for b, d in cases:
        c = {k: torch.from_numpy(v) for k, v in b.items()}
        ref = O.forward(O.to_torch(w), cfg, c["obj_points"], c["obj_2d_feats"], c["edge_indices"], c["descriptor"], c["batch_ids"])
        outs = {}
        for precision, tol in (("bf16_mixed", 1e-2), ("bf16x3", 1e-3), ("fp32", 1e-3)):
            for v in (-1, 0, 1):
                m = VLSATModel(cfg, DEV).load_state(w).eval().set_gemm_precision(precision).debug_option("gather_f16", v)
                outs[precision, v] = _run(m, d)
                m.close()
                for n, g, x in zip(NAMES, outs[precision, v], ref):
                    assert g.numel() == 0 or float((g.cpu() - x).abs().max()) < tol, (precision, v, n)      # (one object: no relation rows)
        same = lambda a, b_: all(torch.equal(x, y) for x, y in zip(a, b_))
        assert same(outs["bf16_mixed", -1], outs["bf16_mixed", 1]) and same(outs["bf16x3", -1], outs["bf16x3", 0])
        assert same(outs["fp32", 1], outs["fp32", 0]) and same(outs["fp32", -1], outs["fp32", 0])
        if d["edge_indices"].shape[1]:
            assert not same(outs["bf16_mixed", 0], outs["bf16_mixed", 1]) and not same(outs["bf16x3", 0], outs["bf16x3", 1])
            diff = max(float((x - y).abs().max()) for x, y in zip(outs["bf16_mixed", 0], outs["bf16_mixed", 1]))
            assert diff < 1e-2, diff               # (two realisations of the mode's rounding noise: each inside 1e-2 of the oracle above)


def test_fp16_out_projection_of_the_single_rounded_edge_attention():
    """"outproj_f16": the out-projection of the edge cross-attention (reference transformer/attention.py:77,121-122) hands its rows to the
    LayerNorm as fp16 half rows where the attention runs single-rounded (bf16_mixed, bf16x3_attn1): both settings inside the mode's tolerance
    against the CPU oracle, different from each other (the switch reaches the kernels: 8-phase epilogue for E = 68 640, the 64 x 64 kernels
    for a one-scene plan); bf16x3 and fp32 have no such launch and ignore the switch bit for bit."""
    from oracle import vlsat_oracle as O
    cfg = VLSATConfig(N_LAYERS=2)
    w = synth.make_weights(cfg)
    same = lambda a, b_: all(torch.equal(x, y) for x, y in zip(a, b_))
    for b, d in (_batch(44, 40, 32, seed0=4600), _batch(1, 26, 32, seed0=4601)):
        c = {k: torch.from_numpy(v) for k, v in b.items()}
        ref = O.forward(O.to_torch(w), cfg, c["obj_points"], c["obj_2d_feats"], c["edge_indices"], c["descriptor"], c["batch_ids"])
        for precision, tol, touched in (("bf16_mixed", 1e-2, True), ("bf16x3_attn1", 1e-2, True), ("bf16x3", 1e-3, False), ("fp32", 1e-3, False)):
            outs = {}
            for v in (0, 1):
                m = VLSATModel(cfg, DEV).load_state(w).eval().set_gemm_precision(precision).debug_option("outproj_f16", v)
                outs[v] = _run(m, d)
                m.close()
                for n, g, x in zip(NAMES, outs[v], ref):
                    assert float((g.cpu() - x).abs().max()) < tol, (precision, v, n)
            assert same(outs[0], outs[1]) != touched, precision
            if touched:                                    # 3D outputs never read the 2D edge attention's result ... which is where the switch acts
                assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2])


def test_fp16_mixed_has_the_margin_bf16_mixed_lacks():
    """Precision mode 5 ('fp16_mixed'): 'bf16_mixed' with fp16 instead of bf16 in the half-row tensors and on the matrix cores of the edge-row
    kernels (v_mfma_f32_32x32x16_f16: the same rate, 2^-12 instead of 2^-9 per stored value and operand; GEMM, edge attention, gate,
    PointNet; node rows stay split-bf16).  Against the fp64 oracle on three scenes of a 16-scene batch: Xavier-scale weights inside 2e-3
    (bf16_mixed: 5e-3), the x1.5 stress weights -- where bf16_mixed is at 1.5e-2 -- inside 5e-3 (x2 is beyond both: 1.4e-2, tools/stress_scan.py).  The 8-phase kernel takes
    the edge-row launches of the batch (E = 24 960); a one-scene plan runs the same mode on the small kernels (paired schedule)."""
    from oracle import vlsat_oracle as O
    cfg = VLSATConfig(N_LAYERS=3)
    scenes = [synth.make_scene(40, 256, 1000 + s) for s in range(16)]
    d = {k: torch.from_numpy(v).to(DEV) for k, v in synth.collate(scenes).items()}
    one = {k: torch.from_numpy(v).to(DEV) for k, v in synth.collate([scenes[7]]).items()}
    for scale, tol16, bf_above in ((1.0, 2e-3, 2e-3), (1.5, 5e-3, 5e-3)):
        w = synth.make_weights(cfg) if scale == 1.0 else synth.make_weights_stress(cfg, scale)
        w64 = O.to_torch(w, torch.float64)
        outs = {}
        for mode in ("fp16_mixed", "bf16_mixed"):
            m = VLSATModel(cfg, DEV).load_state(w).eval().set_gemm_precision(mode)
            outs[mode] = _run(m, d)
            outs[mode, "one"] = _run(m, one)
            m.close()
        worst = {"fp16_mixed": 0.0, "bf16_mixed": 0.0}
        for s in (0, 7, 15):
            c = {k: torch.from_numpy(v) for k, v in synth.collate([scenes[s]]).items()}
            ref = O.forward(w64, cfg, c["obj_points"].double(), c["obj_2d_feats"].double(), c["edge_indices"], c["descriptor"].double(), c["batch_ids"])
            sl = [slice(s * 40, (s + 1) * 40)] * 2 + [slice(s * 1560, (s + 1) * 1560)] * 2
            for mode in worst:
                worst[mode] = max(worst[mode], *[float((g[i].cpu() - r.float()).abs().max()) for g, r, i in zip(outs[mode], ref, sl)])
                if s == 7:                      # the same scene as a one-scene plan: the same mode on the small kernels
                    e1 = max(float((g.cpu() - r.float()).abs().max()) for g, r in zip(outs[mode, "one"], ref))
                    assert e1 < (tol16 if mode == "fp16_mixed" else 3e-2), (scale, mode, e1)
        print(f"stress x{scale}: fp16_mixed {worst['fp16_mixed']:.2e}, bf16_mixed {worst['bf16_mixed']:.2e}")
        assert worst["fp16_mixed"] < tol16, (scale, worst)
        assert worst["bf16_mixed"] > bf_above, (scale, worst)          # (the margin is the point: if bf16_mixed ever gets here, tighten tol16)


def test_fp16_mixed_on_the_other_head_geometries():
    """Mode 5 off the default geometry: NUM_HEADS 4 / 16 run the edge attention at head dims 128 / 32 (flash_attn_bf16_kernel<1, true, 3, 3, 128 | 32, 2>)
    and, like DIM_ATTEN 128 / 512, the gate on the head-geometry template (edge_gate_bf16_hd_kernel<1, 3, ...>); against the CPU oracle inside 2e-3
    where bf16_mixed needs its 1e-2, and auto_precision offers the mode there too.  The same batches in the two other 16-bit forms the edge
    attention has at head dims 128 / 32 and no other test runs there: single rounding on split pairs (mode 4, 'bf16x3_attn1':
    flash_attn_bf16_kernel<1, true, 1, 3, 128 | 32>) and split-bf16 with a two-term P.V product ('bf16x3' with flash_pv_terms 2: <3, true, 1, 2, 32>;
    at head dim 128 that mode keeps the fp32 attention), inside those modes' tolerances of this file."""
    from oracle import vlsat_oracle as O
    for kw in (dict(NUM_HEADS=4), dict(NUM_HEADS=16), dict(DIM_ATTEN=512), dict(NUM_HEADS=16, DIM_ATTEN=128)):
        cfg = VLSATConfig(N_LAYERS=2, **kw)
        w = synth.make_weights(cfg)
        b, d = _batch(3, 12, 64, seed0=4800)
        c = {k: torch.from_numpy(v) for k, v in b.items()}
        ref = O.forward(O.to_torch(w), cfg, c["obj_points"], c["obj_2d_feats"], c["edge_indices"], c["descriptor"], c["batch_ids"])
        errs = {}
        for mode, tol in (("fp16_mixed", 2e-3), ("bf16_mixed", 1e-2), ("bf16x3_attn1", 1e-2), ("bf16x3", 1e-3)):
            m = VLSATModel(cfg, DEV).load_state(w).eval().set_gemm_precision(mode)
            if mode == "bf16x3":
                m.debug_option("flash_pv_terms", 2)
            out = _run(m, d)
            errs[mode] = max(float((g.cpu() - x).abs().max()) for g, x in zip(out, ref))
            assert errs[mode] < tol, (kw, mode, errs)
            if mode == "fp16_mixed":
                r = m.auto_precision(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"], tol=1e-2)
                assert "fp16_mixed" in r["errors"] or r["mode"] == "bf16_mixed", r
            m.close()
        print(kw, {k: f"{v:.2e}" for k, v in errs.items()})
        assert errs["fp16_mixed"] < 0.5 * errs["bf16_mixed"], (kw, errs)


@pytest.mark.parametrize("mode", ["bf16_mixed", "bf16x3_attn1"])
@pytest.mark.parametrize("sizes", [(66, 67, 70, 65, 72, 66, 69, 68), (40, 9, 23, 40, 31, 12, 40, 17, 40, 3, 40, 26)])
def test_64_queries_per_wave_edge_attention_is_bit_identical(mode, sizes):
    """"flash_qg" 1 | 2: the half-row edge attention (reference transformer/attention.py:60-76 as called from
    network_MMG.py:231) with TWO 32-query groups per wave -- every K / V fragment read from LDS feeds two MFMAs, Q and O of both groups
    register-resident (flash_attn_bf16.hip QG = 2; 2 = the P.V product of the first group issued in front of the second group's
    softmax).  A query sees the same keys in the same order through the same instructions, so the outputs must equal the shipped kernel
    BIT FOR BIT: on the 256-query tile table (scenes of >= 4096 edges: four waves per block) and on the 128-query one (two waves
    per block; scene sizes that leave the second group of a wave partly or wholly past the scene's last edge)."""
    cfg = VLSATConfig(N_LAYERS=2)
    w = synth.make_weights(cfg, seed=5)
    scenes = [synth.make_scene(n, 64, 900 + i) for i, n in enumerate(sizes)]
    d = {k: torch.from_numpy(v).to(DEV) for k, v in synth.collate(scenes).items()}
    m = VLSATModel(cfg, DEV).load_state(w).eval().set_gemm_precision(mode)
    m.debug_option("flash_split", 0)
    base = _run(m, d)
    for qg in (1, 2):
        m.debug_option("flash_qg", qg)
        got = _run(m, d)
        for n, a, b in zip(NAMES, base, got):
            assert torch.equal(a, b), (qg, n, float((a - b).abs().max()))
    m.close()
