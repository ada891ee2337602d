"""Score histograms without a GPU: the host restatement against the existing decode counts at every checked threshold,
evaluate.operating_points against a brute-force loop over thresholds and a direct numpy statement of the object figures, and
the bin function of csrc/calib_core.h under ASan + UBSan against the PyTorch restatement."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, lib as L, metrics as M

import host_check
from calibration_checks import assert_counts_match, brute_object_numbers, host_tables, make_case, special_scores

CASES = [(1, True), (26, True), (32, True), (27, False)]


@pytest.mark.parametrize("bins", [16, 1024, 4096])
@pytest.mark.parametrize("r,multi", CASES)
def test_host_tables_hold_the_decode_counts_of_every_threshold(r, multi, bins):
    case = make_case(700, r, bins, multi, seed=r * 7 + bins)
    if r >= 26:                                     # room for every special value
        have = set(case["rp"].view(torch.int32).view(-1).tolist())
        assert set(special_scores(bins, multi).view(torch.int32).tolist()) <= have
    t = host_tables(case)
    assert t.rel.shape == (r, 2, bins + 1) and t.obj.shape == (2, bins + 1) and t.confusion.shape == (160, 160)
    assert t.rel.data_ptr() == t.buffer.data_ptr() and t.buffer.numel() == t.rel.numel() + t.obj.numel() + t.confusion.numel()
    assert_counts_match(t, case)
    valid = int(((case["gt_cls"] >= 0) & (case["gt_cls"] < 160)).sum())
    assert int(t.obj.sum()) == valid == int(t.confusion.sum())
    if not multi:                                   # class 0 is never eligible, and one cell per row at most is
        assert int(t.rel[0, :, :bins].sum()) == 0 and int(t.rel[:, :, :bins].sum()) <= 700


def test_tables_accumulate_and_reject_what_they_cannot_hold():
    case = make_case(300, 26, 16, True, seed=3)
    one = host_tables(case)
    acc = M.ScoreTables(26, 160, 16)
    for _ in range(2):
        M.score_histograms(case["probs"], case["rp"], case["gt_cls"], case["gt_rel"], True, 16, obj_probs=case["probs"], rel_probs=case["rp"],
                           tables=acc)
    assert torch.equal(acc.buffer, 2 * one.buffer)
    for bad in (8, 24, 8192):
        with pytest.raises(L.VlsatError):
            M.ScoreTables(26, 160, bad)
    with pytest.raises(L.VlsatError):
        M.score_histograms(case["probs"], case["rp"], case["gt_cls"], case["gt_rel"], True, 32, tables=acc)
    with pytest.raises(ValueError):
        one.counts_at(0.51)                         # not a multiple of 1 / 16
    with pytest.raises(ValueError):
        one.counts_at(16)


def _brute_curves(case, bins):
    r = case["rp"].shape[1]
    out = np.zeros((3, r, bins))
    counts = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(bins):
            c = M.decode_counts_host(case["probs"], case["rp"], case["gt_cls"], case["gt_rel"], case["multi"], k / bins, obj_probs=case["probs"],
                                     rel_probs=case["rp"])[:3 * r].numpy().astype(np.float64)
            counts.append(c)
            tp, fp, fn = c[0::3], c[1::3], c[2::3]
            out[0, :, k], out[1, :, k], out[2, :, k] = tp / (tp + fp), tp / (tp + fn), 2 * tp / (2 * tp + fp + fn)
    return out, counts


@pytest.mark.parametrize("multi", [True, False])
def test_operating_points_equal_a_loop_over_thresholds(multi):
    bins, r = 16, 7
    case = make_case(400, r, bins, multi, seed=11, n=200)
    if multi:
        case["gt_rel"][:, 4] = 0                    # a predicate without ground truth
        case["rp"][:, 5] = 0.0                      # a predicate never scored above 0
        case["gt_rel"][:50, 5] = 1
    else:
        case["gt_rel"][case["gt_rel"] == 4] = 0
        case["rp"][:, 5] = 0.0
    ops = EV.operating_points(host_tables(case), default=0.25)
    curves, counts = _brute_curves(case, bins)
    for i, name in enumerate(("precision", "recall", "f1")):
        np.testing.assert_array_equal(ops[name], curves[i], err_msg=name)
    n_gt = counts[0][0::3] + counts[0][2::3]
    for p in range(r):
        if n_gt[p] == 0:
            want_k = 4                              # default 0.25 = 4 / 16
            assert np.isnan(ops["ap"][p])
        else:
            f1 = curves[2, p]
            best = np.nanmax(f1)
            want_k = min(k for k in range(bins) if f1[k] == best)
            ap, nxt = 0.0, 0.0
            terms = []
            for k in range(bins):
                nxt = curves[1, p, k + 1] if k + 1 < bins else 0.0
                prec = curves[0, p, k]
                terms.append((curves[1, p, k] - nxt) * (0.0 if np.isnan(prec) else prec))
            assert ops["ap"][p] == pytest.approx(sum(terms), rel=1e-12, abs=1e-15)
        assert int(ops["k"][p]) == want_k and float(ops["threshold"][p]) == want_k / bins
        assert [int(ops[f][p]) for f in ("tp", "fp", "fn")] == [int(counts[want_k][3 * p + j]) for j in range(3)]
    assert ops["threshold"].dtype == torch.float32 and int(ops["k"][4]) == 4
    if multi:
        assert int(ops["k"][5]) == 0                # asserting everything is the only way to any recall
    occurs = n_gt > 0
    assert ops["mean_ap"] == pytest.approx(float(np.mean(ops["ap"][occurs])))
    # the chosen vector through the existing counts gives the promised tp / fp / fn, and graph_quality's F1 of them
    again = M.decode_counts_host(case["probs"], case["rp"], case["gt_cls"], case["gt_rel"], multi, ops["threshold"], obj_probs=case["probs"],
                                 rel_probs=case["rp"])
    assert torch.equal(again[:3 * r], ops["counts"])
    q, qd = EV.graph_quality(again, r), EV.graph_quality(torch.cat([torch.from_numpy(counts[4]).long(), again[-2:]]), r)
    assert ops["micro_f1"] == q["micro_f1"] and ops["macro_f1"] == q["macro_f1"]
    assert ops["micro_f1_default"] == qd["micro_f1"] and ops["macro_f1_default"] == qd["macro_f1"]
    assert ops["macro_f1"] >= ops["macro_f1_default"]
    # the object head
    assert int((case["gt_cls"] == -1).sum()) > 0
    ece, per, acc = brute_object_numbers(case["probs"], case["gt_cls"], bins)
    assert ops["ece"] == pytest.approx(ece, rel=1e-12) and ops["obj_acc"] == pytest.approx(acc, rel=1e-12)
    np.testing.assert_array_equal(ops["per_class_acc"], per)
    assert ops["mean_class_acc"] == pytest.approx(float(np.nanmean(per)), rel=1e-12)
    assert int(ops["obj_bin_count"].sum()) == int(((case["gt_cls"] >= 0) & (case["gt_cls"] < 160)).sum())


def test_operating_points_of_empty_tables_are_nan_not_errors():
    ops = EV.operating_points(M.ScoreTables(3, 4, 16))
    assert np.isnan(ops["mean_ap"]) and np.isnan(ops["ece"]) and np.isnan(ops["mean_class_acc"])
    assert ops["threshold"].tolist() == [0.5, 0.5, 0.5]
    with pytest.raises(ValueError):
        EV.operating_points(M.ScoreTables(3, 4, 16), default=0.3)


def _bin_rows(sanitize):
    """rows (bins, fp32 bit pattern, eligible, column) that tests/calib_host_check.cpp printed"""
    rows = []
    for left, col in host_check.lines("calib_host_check", sanitize=sanitize):
        bins, bits, eligible = left.split(":")
        rows.append((int(bins), int(bits, 16), int(eligible), int(col)))
    return rows


def test_bin_function_under_host_sanitizers_equals_the_restatement():
    rows = _bin_rows(sanitize=True)
    assert len(rows) == sum((3 * b + 10) * 2 for b in (16, 1024, 4096))
    for bins in (16, 1024, 4096):
        sel = [x for x in rows if x[0] == bins]
        p = torch.from_numpy(np.array([x[1] for x in sel], dtype=np.uint32).view(np.float32).copy())
        elig = torch.tensor([bool(x[2]) for x in sel])
        want = M._score_columns(p, elig, bins)
        assert want.tolist() == [x[3] for x in sel], bins
        assert {x[3] for x in sel if not x[2]} == {bins}
    assert rows == _bin_rows(sanitize=False)
