"""fp32 mode, "edge_pairs_e2": whether the 2D chain tensor E2, as the LayerNorm of the edge attention and conv3 of rel_encoder_2d write it,
travels as GEMM pair words (csrc/edge_pairs.h EdgePairs::e2).  tests/e2_pairs_check.cpp (g++, through tests/host_check.py; plain and with
ASan + UBSan in the stand-alone binary) prints the decision of every plan next to what plan_gemm gives each launch that touches that E2;
the expected decision is derived here from those planner answers and from the plan's switches, never from a guessed kernel.  Also: the
numpy float16 packer that tests/test_hip_layernorm_pairs.py compares the LayerNorm kernel with, against the header's f16s_pair_pack.
No HIP header, no library, no device."""
import numpy as np
import pytest

import host_check
import e2_pairs_pack as P

LAUNCHES = ("conv3", "nn_edge.0", "proj_edge", "head")
# plans whose switches refuse E2 before any launch is asked, with a word of the reason
REFUSED = {
    "bench batch, 3D only": "2D branch does not run",
    "bench batch, debug stop": "debug stop",
    "bench batch, training outputs": "training outputs",
    "bench batch, feature_transform": "feature_transform",
    "bench batch, edge_pairs 0": "edge_pairs is 0",
    "bench batch, edge_pairs_e2 0": "edge_pairs_e2 is 0",
    "E = 0": "no edges",
    "one scene of 9 objects, paired schedule": "paired schedule",
}


def _rows(sanitize):
    out = {}
    for name, right in host_check.lines("e2_pairs_check", sanitize=sanitize):
        cells = [c.strip() for c in right.split(" | ")]
        assert [c.split()[0] for c in cells] == ["E2", "Hbig2", *LAUNCHES], (name, right)
        e2 = cells[0].split(None, 1)[1]
        assert e2 == "pairs" or (e2.startswith("fp32 (") and e2.endswith(")") and len(e2) > 10), (name, e2)     # a refusal states its reason
        out[name] = dict(e2=e2, hbig2=int(cells[1].split()[1]), **{c.split()[0]: c.split()[1].split(",") for c in cells[2:]})
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_when_e2_pairs(sanitize):
    """E2 pairs exactly where no switch of the plan refuses it and every part of every launch that touches it is on a kernel with the
    pair form, as the planner answers for the launch's own shape and flags"""
    rows = _rows(sanitize)
    assert len(rows) == 21
    for name, r in rows.items():
        every_part = [p for launch in LAUNCHES for p in r[launch]]
        forms = all(p.endswith("+") or p == "none" for p in every_part)
        if name in REFUSED:
            assert r["e2"].startswith("fp32 (") and REFUSED[name] in r["e2"], (name, r["e2"])
        elif forms:
            assert r["e2"] == "pairs", (name, r)
        else:
            assert r["e2"].startswith("fp32 ("), (name, r)
            bad = next(p for p in every_part if p.endswith("-"))          # the refusal names the kind of part that has no form
            word = {"exact-": "exact", "splitk-": "split-K", "p8-": "8-phase", "tiled-": "persistent"}.get(bad)
            assert word is None or word in r["e2"], (name, bad, r["e2"])
    # the plans the GPU tests and the benchmark run: what the planner said, stated once more in words
    assert rows["bench batch"]["e2"] == "pairs" and rows["bench batch"]["hbig2"] == 1
    assert all(p == "p8+" or p == "tiled+" for launch in LAUNCHES for p in rows["bench batch"][launch])
    assert "p8+" in rows["bench batch"]["nn_edge.0"] and "p8+" in rows["bench batch"]["proj_edge"] and "p8+" in rows["bench batch"]["head"]
    assert rows["E = 720"]["e2"] == "pairs" and rows["E = 720, gemm_p8_part_min 1"]["e2"] == "pairs"
    assert rows["bench batch, flash_exact 1"]["e2"] == "pairs" and rows["E = 720, flash_exact 1"]["e2"] == "pairs"
    assert rows["bench batch, no proj_edge"]["e2"] == "pairs" and rows["bench batch, no proj_edge"]["proj_edge"] == ["none"]
    for opt in ("gemm_exact", "gemm_small_exact"):
        for plan in ("bench batch", "E = 720"):
            assert "exact" in rows[f"{plan}, {opt} 1"]["e2"], (plan, opt)
    assert "split-K" in rows["scenes of 5, 1 and 7 objects (E = 62)"]["e2"]
    assert rows["scenes of 5, 1 and 7 objects (E = 62), gemm_splitk 0"]["e2"] == "pairs"


def test_numpy_pack_is_the_headers_pack():
    """pack (numpy float16, tests/e2_pairs_pack.py) == f16s_pair_pack (the header's integer code) on the values
    tests/test_hip_layernorm_pairs.py plants and on random ones at three scales"""
    rng = np.random.default_rng(11)
    x = np.concatenate([P.PLANTED, rng.standard_normal(600).astype(np.float32), (rng.standard_normal(600) * 2e-4).astype(np.float32),
                        (rng.standard_normal(600) * 5e4).astype(np.float32)])
    bits = x.view(np.uint32)
    words = []
    for i in range(0, len(bits), 500):
        rows = host_check.lines("e2_pairs_check", "pack", *(f"{b:08x}" for b in bits[i:i + 500]))
        assert [r[0] for r in rows] == [f"{b:08x}" for b in bits[i:i + 500]]
        words += [int(r[1], 16) for r in rows]
    got = P.pack(x)
    assert got.dtype == np.uint32 and (got == np.array(words, np.uint32)).all(), x[got != np.array(words, np.uint32)][:8]
    assert P.pack(np.float32(-0.0)) == 0x80000000 and P.pack(np.float32(7e4)) == P.pack(np.float32(65504.0)) == 0x7BFF0000
    assert P.pack(np.float32(-7e4)) == 0xFBFF0000
