"""Helpers shared by the score-histogram tests (not a test module): the score generator with every value at which the bin rule can
go wrong, and the comparison of a table with the existing decode counts."""
import numpy as np
import torch

from vlsat_amd import metrics as M


def special_scores(bins: int, nan: bool) -> torch.Tensor:
    """Every edge k / bins, its two fp32 neighbours, then 0.0, -0.0, 1.0, a denormal, a negative, 1.5, +inf (and NaN): the last
    7 (8) entries are the ones that are no edge."""
    edge = torch.arange(bins, dtype=torch.float32) / bins
    up, down = torch.nextafter(edge, torch.tensor(2.0)), torch.nextafter(edge, torch.tensor(-1.0))
    rest = [0.0, -0.0, 1.0, 1e-42, -0.3, 1.5, float("inf")] + ([float("nan")] if nan else [])
    return torch.cat([edge, up, down, torch.tensor(rest, dtype=torch.float32)])


def make_case(e: int, r: int, bins: int, multi: bool, seed: int, n: int = 50, c: int = 160) -> dict:
    """CPU tensors: ``rp`` [E, R] = rand ** 4 (most scores near 0, as a trained head's) with the special values scattered in -- all
    of them where E * R has room for them in three quarters of the cells, otherwise the non-edge ones and a random sample of the
    rest; NaN only in the multi-label cases; ``gt_rel`` 10 % hot cells (multi-label) or a random label with 0 = none; object
    probabilities with an exact tie and ``gt_cls`` in -1..C (-1 and C: nodes without a class)."""
    g = torch.Generator().manual_seed(seed)
    rp = torch.rand(e, r, generator=g) ** 4
    sp = special_scores(bins, multi)
    room = (e * r * 3) // 4
    n_rest = 8 if multi else 7
    if sp.numel() > room:
        keep = torch.randperm(sp.numel() - n_rest, generator=g)[:max(room - n_rest, 0)]
        sp = torch.cat([sp[keep], sp[-n_rest:]])[:e * r]
    rp.view(-1)[torch.randperm(e * r, generator=g)[:sp.numel()]] = sp
    gt_rel = (torch.rand(e, r, generator=g) < 0.1).long() if multi else torch.randint(0, r, (e,), generator=g)
    probs = torch.softmax(torch.randn(n, c, generator=g) * 3, -1)
    if n > 2 and c > 3:
        probs[1, 2] = probs[1, 3] = probs[1].max()                 # a tied row maximum: the lower class is top-1
    gt_cls = torch.randint(-1, c, (n,), generator=g)
    if n:
        gt_cls[0] = probs[0].argmax()                              # at least one right node
    if n > 3:
        gt_cls[2::9] = -1                                          # nodes without a class, below and above the range
        gt_cls[3] = c
    return {"rp": rp, "gt_rel": gt_rel, "probs": probs, "gt_cls": gt_cls, "multi": multi, "bins": bins}


def host_tables(case) -> "M.ScoreTables":
    return M.score_histograms_host(case["probs"], case["rp"], case["gt_cls"], case["gt_rel"], case["multi"], case["bins"],
                                   obj_probs=case["probs"], rel_probs=case["rp"])


def device_tables(case, dev, tables=None) -> "M.ScoreTables":
    d = lambda t: t.to(dev)
    return M.score_histograms(d(case["probs"]), d(case["rp"]), d(case["gt_cls"]), d(case["gt_rel"]), case["multi"], case["bins"],
                              obj_probs=d(case["probs"]), rel_probs=d(case["rp"]), tables=tables)


def ks_to_check(bins: int, r: int, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    return [0, 1, bins // 2, bins - 1, torch.randint(0, bins, (r,), generator=g)]


def assert_counts_match(tables, case):
    """tables.counts_at(k) == the tp / fp / fn of decode_counts_host at threshold k / bins, for the k of ks_to_check."""
    e, r = case["rp"].shape
    bins = case["bins"]
    assert int(tables.rel.sum()) == e * r
    for k in ks_to_check(bins, r):
        kv = tables.k_vector(k)
        thr = kv.to(torch.float32) / bins                           # exact: bins is a power of two
        want = M.decode_counts_host(case["probs"], case["rp"], case["gt_cls"], case["gt_rel"], case["multi"], thr, obj_probs=case["probs"],
                                    rel_probs=case["rp"])
        assert torch.equal(tables.counts_at(k), want[:3 * r]), (r, bins, k)
        assert torch.equal(tables.counts_at(thr), want[:3 * r])


def assert_tables_equal(got, want, what=""):
    for f in ("rel", "obj", "confusion"):
        a, b = getattr(got, f).cpu(), getattr(want, f).cpu()
        assert a.shape == b.shape and torch.equal(a, b), (what, f, int((a != b).sum()))


def brute_object_numbers(probs, gt_cls, bins):
    """ECE (bin midpoints), per-class accuracy and overall accuracy straight from top-1 and gt_cls in numpy."""
    p, gt = probs.numpy(), gt_cls.numpy()
    c = p.shape[1]
    top1 = np.array([min(k for k in range(c) if row[k] == row.max()) for row in p])
    conf = p[np.arange(len(p)), top1]
    ok = (gt >= 0) & (gt < c)
    top1, conf, gt = top1[ok], conf[ok], gt[ok]
    col = np.minimum(np.floor(conf * np.float32(bins)).astype(np.int64), bins - 1)
    ece = 0.0
    for b in range(bins):
        sel = col == b
        if sel.any():
            ece += sel.sum() / len(gt) * abs((top1[sel] == gt[sel]).mean() - (b + 0.5) / bins)
    per = np.full(c, np.nan)
    for k in range(c):
        if (gt == k).any():
            per[k] = (top1[gt == k] == k).mean()
    return ece, per, float((top1 == gt).mean())
