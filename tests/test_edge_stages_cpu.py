"""csrc/edge_stages.h: every edge-row Linear of the forward as the GemmArgs of its launch -- what engine_forward.hip launches and what
edge_pairs_plan asks the GEMM planner about.  tests/edge_stages_check.cpp (g++, through tests/host_check.py; plain and with ASan + UBSan in
the stand-alone binary) prints every field the builders set, per stage, branch and case; TABLE below states each stage once more, typed in
from the launch sites engine_forward.hip had before the builders (gcn_block, rel_head, rel_encoder, edge_attn_q / kv / out, nn_edge0_args
and the triplet_projector_2d block), so a builder cannot drift from what was launched.  No HIP header, no library, no device."""
import pytest

import host_check

DIMS = dict(E=720, D=512, NPC=6 * 512 + 256, R=26)
# what a launch has unless its row says otherwise: M = E, lda = ldw = K, ldc = N, a bias, no additive operands, fp32 tensors, no pair words
DEFAULTS = dict(M="E", lda="K", ldw="K", ldc="N", ops="1", bias="1", resid="0", ldr="0", g="0", ldg0="0", ldg1="0", g1="0", act="'none'", relu_a="0",
                a_split="0", c_split="0", r_split="0", c_scale="1", c_f16_cols="0", g_f16="0", a_pair="0", c_pair="0")
# chain: the branch's chain tensor as pairs (E3 for br 0, the LayerNorm's / conv3's E2 for br 1); hbig, r1: of the branch; every name below
# is a parameter of the line (see edge_stages_check.cpp) or one of e3 / e2 / hbig / r1 / oe / kvp, whether that tensor pairs
NN_EDGE0 = dict(K="D", N="2 * D", bias="0", g="3", ldg0="NPC", ldg1="NPC", act="'relu'", a_split="S", c_split="S")
TABLE = {
    "conv2": dict(K="64", N="128", lda="128", act="'relu'", c_split="S"),
    "conv3": dict(K="128", N="D", act="'relu'", a_split="S", c_split="S", c_pair="chain"),
    "nn_edge.0": dict(NN_EDGE0, g1="D if g16 else 2 * D", g_f16="g16", relu_a="relu", a_pair="chain", c_pair="hbig"),
    "proj_edge": dict(K="D", N="D", relu_a="relu", a_split="S", c_split="S if gate16 else 0", a_pair="chain"),
    "nn_edge.2": dict(K="2 * D", N="D", a_split="S", c_split="S", a_pair="hbig", c_pair="e3 if br == 0 else 0"),
    "head1": dict(K="D", N="512", act="'relu'", relu_a="relu", a_split="S", c_split="S", a_pair="chain", c_pair="r1"),
    "head2": dict(K="512", N="256", act="'relu'", a_split="S", c_split="S", a_pair="r1"),
    "head3": dict(K="256", N="R", act="'sigmoid' if sig else 'none'", a_split="S"),
    "attn_q": dict(K="D", N="D", a_split="S", c_split="SA", c_scale="0.25 if SA else 1"),
    "attn_kv": dict(K="D", N="2 * D", a_split="S", c_split="SA", a_pair="e3", c_pair="2 if kvp else 0"),
    "attn_out": dict(K="D", N="D", a_split="SA", resid="0 if lnres else 1", ldr="0 if lnres else D", r_split="0 if lnres else S",
                     c_f16_cols="D if o16 else 0", a_pair="oe"),
    "triplet0": dict(NN_EDGE0, g1="2 * D", c_pair="hbig2"),
    "triplet2": dict(K="2 * D", N="D", a_split="S", a_pair="hbig2"),
}
LINES = {"conv2": 3, "head3": 6, "conv3": 24, "nn_edge.2": 24, "head2": 24, "nn_edge.0": 96, "proj_edge": 96, "head1": 48, "triplet0": 12,
         "triplet2": 12, "attn_q": 36, "attn_kv": 36, "attn_out": 144}


def _value(v):
    return v if isinstance(v, str) else int(v) if float(v) == int(v) else float(v)


def _lines(sanitize):
    for left, right in host_check.lines("edge_stages_check", sanitize=sanitize):
        stage, *params = left.split()
        case = {k: (v if k == "pairs" else int(v)) for k, v in (p.split("=") for p in params)}
        got = {k: (v if k == "act" else float(v)) for k, v in (f.split("=") for f in right.split())}
        yield stage, case, got


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_every_stage_is_the_launch_of_the_table(sanitize):
    seen = {}
    for stage, case, got in _lines(sanitize):
        seen[stage] = seen.get(stage, 0) + 1
        rest, kvp = case.get("pairs") in ("all", "nokv"), case.get("pairs") in ("all", "kv")
        env = dict(DIMS, **case, e3=rest, e2=rest, oe=rest, hbig2=rest, kvp=kvp)
        if "br" in case:
            env.update(chain=rest, hbig=rest, r1=rest)
        row = dict(DEFAULTS, **TABLE[stage])
        env["K"], env["N"] = eval(row["K"], {}, env), eval(row["N"], {}, env)
        want = {k: _value(eval(v, {}, env)) for k, v in row.items()}
        assert set(want) == set(got), (stage, sorted(set(want) ^ set(got)))
        assert {k: _value(v) for k, v in got.items()} == want, (stage, case, {k: (got[k], want[k]) for k in want if _value(got[k]) != want[k]})
        # nn_edge.2 never writes pair words on the 2D branch (its E2 is the fp32 residual of the out-projection), the query projection
        # never reads them, and K | V leave as attention pair words exactly when kv is set
        if stage == "nn_edge.2" and case["br"] == 1:
            assert got["c_pair"] == 0, case
        if stage == "attn_q":
            assert got["a_pair"] == 0 and got["c_pair"] == 0, case
        if stage == "attn_kv":
            assert got["c_pair"] == (2 if case["pairs"] in ("all", "kv") else 0), case
    assert seen == LINES
