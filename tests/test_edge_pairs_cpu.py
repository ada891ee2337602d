"""The fp32 mode's GEMM pair words (csrc/gemm_f16s_planes.h f16s_pair_pack) and the function that decides which edge tensors of a forward
carry them (csrc/edge_pairs.h edge_pairs_plan), compiled by g++ (tests/edge_pairs_check.cpp through tests/host_check.py): no HIP header,
no library, no device."""
import numpy as np
import pytest

import host_check

TENSORS = ("Hbig3", "Hbig2", "R1_3", "R1_2", "E3", "Oe", "KV")


def _plans(sanitize):
    rows = dict(host_check.lines("edge_pairs_check", sanitize=sanitize))
    out = {}
    for name, right in rows.items():
        if name in ("format", "forms"):
            out[name] = right
            continue
        cells = [c.strip() for c in right.split(" | ")]
        assert [c.split()[0] for c in cells] == list(TENSORS), (name, right)
        for c in cells:                              # every refusal states its reason
            assert c.split()[1] == "pairs" or (c.split()[1] == "fp32" and c.endswith(")") and len(c.split("(", 1)[1]) > 3), (name, c)
        out[name] = {c.split()[0] for c in cells if c.split()[1] == "pairs"}
    return out, rows


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_which_tensors_pair(sanitize):
    """the bench plan at 256 CUs, the plans of tests/test_hip_edge_pairs.py, every *_exact option, a bf16 mode, feature_transform, training
    outputs, a debug stop, the probability tap, 3D only, the exact attention kernel, head dims 32 / 128, split keys (Oe stays fp32).
    "asan_ubsan": the same stand-alone binary under ASan + UBSan."""
    got, rows = _plans(sanitize)
    assert got["format"].startswith("ok ") and got["format"].endswith(" 0 wrong"), got["format"]
    assert got["forms"] == "ok 13 rows, 0 wrong"
    # (R1 of the 2D head never pairs: measured, its first Linear pays for the packing what the second saves -- profiles/edge_pairs_ab.txt)
    everything = {"Hbig3", "Hbig2", "R1_3", "E3", "Oe", "KV"}
    no_e3, no_attn, no_r1 = everything - {"E3"}, everything - {"Oe", "KV"}, everything - {"R1_3"}
    want = {
        "bench batch, 256 CUs": everything,
        "bench batch, edge_pairs 0": set(),
        "bench batch, gemm_exact 1": set(),
        "bench batch, gemm_small_exact 1": set(),
        "bench batch, a bf16 mode": set(),
        "bench batch, feature_transform": no_e3,
        "bench batch, training outputs": no_e3,
        "bench batch, debug stop": no_e3,
        "bench batch, probability tap": no_e3,
        "bench batch, 3D only": {"Hbig3", "R1_3", "E3"},
        "bench batch, gemm_dma 0": set(),
        "bench batch, gemm_p8 0": everything,
        "bench batch, flash_exact 1": no_attn,
        "bench batch, head dim 32": no_attn,
        "bench batch, head dim 128": no_attn,
        "bench batch, head dim 128 asked of the split-fp16 kernel": no_attn,
        "bench batch, flash_tr 0": everything,
        "bench batch, four key parts": everything - {"Oe"},
        "E = 720": no_r1,                                # (the relation head's second Linear is 48 tiles: split-K)
        "E = 720, gemm_p8_part_min 1": no_r1,
        "E = 720, three key parts": no_r1 - {"Oe"},
        "E = 720, gemm_splitk 0": everything,
        "E = 720, gemm_p8_part_min 1, gemm_splitk 0": everything,
        "scenes of 5, 1 and 7 objects (E = 62)": set(),
        "E = 0": set(),
        "one scene of 9 objects, paired schedule": set(),
        "one scene of 9 objects, pair_twins 0": set(),
        "one scene of 200 objects": everything,
    }
    assert {k: v for k, v in got.items() if k not in ("format", "forms")} == want
    assert "split-K" in rows["E = 720"] and "paired schedule" in rows["one scene of 9 objects, paired schedule"]
    assert "exact" in rows["bench batch, gemm_exact 1"] and "edge_pairs is 0" in rows["bench batch, edge_pairs 0"]
    assert "measured" in rows["bench batch, 256 CUs"] and "R1_2 fp32 (the 2D branch does not run)" in rows["bench batch, 3D only"]
    assert "split keys" in rows["E = 720, three key parts"] and "head dim not built" in rows["bench batch, head dim 128 asked of the split-fp16 kernel"]


def _on_the_fly(x, relu):
    """what a reader of an fp32 tensor computes (gemm_p8_kernel.h FS, gemm_core.h f16s_split8) in numpy: clamp (the lower bound is the
    ReLU), Ah = f16(x), Al = f16((x - Ah) 2^11) -- the difference and the product are exact in fp32"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        xc = np.clip(x, np.float32(0.0 if relu else -65504.0), np.float32(65504.0))
        hi = xc.astype(np.float16)
        lo = ((xc - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo


def test_pair_word_unpacks_to_the_on_the_fly_split():
    """pack (the header's integer code, through the check program) then unpack (the two halves of the word; a pending ReLU as a signed max
    on the word) gives exactly the (Ah, Al) of the on-the-fly split in numpy float16: -0.0, values below 2^-13 (lo parts that are fp16
    subnormals even times 2^11), +-65504 and beyond, infinities, and 4000 random values at the forward's and the stress weights' scales"""
    rng = np.random.default_rng(5)
    special = np.array([0.0, -0.0, 1.0, -1.0, 65504.0, -65504.0, 65519.0, 65520.0, 7e4, -7e4, 3e38, -3e38, np.inf, -np.inf,
                        2.0 ** -13, -2.0 ** -13, 1.2e-4, 6.1e-5, -6.1e-5, 6e-8, 2.9e-8, 1e-12, -1e-12, 1e-40, 0.1, -0.3333], np.float32)
    x = np.concatenate([special, rng.standard_normal(1000).astype(np.float32), (rng.standard_normal(1000) * 3000).astype(np.float32),
                        (rng.standard_normal(1000) * 2e-4).astype(np.float32), (rng.standard_normal(1000) * 40000).astype(np.float32)])
    bits = x.view(np.uint32)
    words, relu_words, k_words, v_words = [], [], [], []
    for i in range(0, len(bits), 500):
        rows = host_check.lines("edge_pairs_check", "pack", *(f"{b:08x}" for b in bits[i:i + 500]))
        assert [r[0] for r in rows] == [f"{b:08x}" for b in bits[i:i + 500]]
        words += [int(r[1].split()[0], 16) for r in rows]
        relu_words += [int(r[1].split()[1], 16) for r in rows]
        k_words += [int(r[1].split()[2], 16) for r in rows]
        v_words += [int(r[1].split()[3], 16) for r in rows]
    for relu, w in ((False, words), (True, relu_words)):
        w = np.array(w, np.uint32)
        hi, lo = _on_the_fly(x, relu)
        got_hi, got_lo = (w >> 16).astype(np.uint16).view(np.float16), (w & 0xffff).astype(np.uint16).view(np.float16)
        # bit for bit, except the sign of a zero: relu(-0.0) and relu(x < 0) are +0 in the word, numpy's clip keeps -0.0
        for got, ref, what in ((got_hi, hi, "Ah"), (got_lo, lo, "Al")):
            same = (got.view(np.uint16) == ref.view(np.uint16)) | ((got == 0) & (ref == 0) & relu)
            assert same.all(), (relu, what, x[~same][:5], got[~same][:5], ref[~same][:5])
        assert np.isfinite(got_hi.astype(np.float32)).all() and np.isfinite(got_lo.astype(np.float32)).all()
    # the attention pair words: split4h<true> of a K element and of a V element times 2^3 (flash_attn_bf16.hip), lo unscaled
    for shift, w in ((0, k_words), (3, v_words)):
        w = np.array(w, np.uint32)
        with np.errstate(over="ignore", invalid="ignore"):
            xc = np.clip(x * np.float32(2.0 ** shift), np.float32(-65504.0), np.float32(65504.0))
            hi = xc.astype(np.float16)
            lo = (xc - hi.astype(np.float32)).astype(np.float16)
        assert ((w >> 16).astype(np.uint16) == hi.view(np.uint16)).all() and ((w & 0xffff).astype(np.uint16) == lo.view(np.uint16)).all(), shift
    # the word's sign bit is the sign of x: that is what makes the ReLU a signed integer max
    assert ((np.array(words, np.uint32) >> 31).astype(bool) == np.signbit(x)).all()
