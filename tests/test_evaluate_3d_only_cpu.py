"""3D-only evaluation on the host side (no GPU): evaluate.accumulate / accumulate_split / recall_vector with the 2D input missing leave
the 2D entries of the additive vectors as they are and give the 3D entries of the two-branch call; summarize / recall_summarize /
split_summarize / _summaries with use_2d=False return the 3D branch's keys (and ``scenes``) with the two-branch values; the defaults
return what they returned before.  Everything is compared exactly.  A "2D key" ends in ``_2d`` or, for recall_summarize's pooled
values, in ``_2d_pooled``."""
import numpy as np
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV
from vlsat_amd.metrics import recallk_width

R, C = 26, 160


def _is_2d(name):
    return name.endswith("_2d") or name.endswith("_2d_pooled")


def _batch(seed, n=9, e=40):
    """rank lists and the cls_matrix of one batch as process_val returns them: rows per edge, one -1 row for an edge without gt"""
    g = np.random.default_rng(seed)
    rows = []
    for _ in range(e):
        s, o = g.integers(0, C, 2)
        preds = sorted(g.choice(R, g.integers(0, 3), replace=False).tolist()) or [-1]
        rows += [[s, g.integers(1, 12), o, g.integers(1, 12), p] for p in preds]
    cm = np.array(rows, dtype=np.int64)
    ranks = {}
    for sfx in ("", "_2d"):
        ranks["top_k_obj" + sfx] = g.integers(1, 13, n)
        ranks["top_k_rel" + sfx] = g.integers(1, 8, len(cm))
        ranks["top_k_triplet" + sfx] = g.integers(1, 103, len(cm))
    return ranks, cm


def _same(a, b):
    return np.array(a, np.float64).tobytes() == np.array(b, np.float64).tobytes()


def _check_vec(names, only, full, in_2d=0.0):
    bad = [(f, a, b) for f, a, b in zip(names, only.tolist(), full.tolist()) if not _same(a, in_2d if _is_2d(f) else b)]
    assert len(names) == len(only) == len(full) and not bad, bad[:8]


def _check_summary(only, full):
    assert set(only) == {k for k in full if not _is_2d(k)} and not [k for k in only if "_2d" in k]
    assert all(_same(v, full[k]) for k, v in only.items()), [(k, v, full[k]) for k, v in only.items() if not _same(v, full[k])][:8]


def _vectors():
    F, S = EV.fields(), EV.split_fields()
    table = (np.random.default_rng(3).random(C * C * R) < 0.5).astype(np.uint8)
    full, only, kept = np.zeros(len(F)), np.zeros(len(F)), np.array([7.0 if _is_2d(f) else 0.0 for f in F])
    sfull, sonly, skept = np.zeros(len(S)), np.zeros(len(S)), np.array([7.0 if _is_2d(f) else 0.0 for f in S])
    for seed in (1, 2, 3):
        ranks, cm = _batch(seed)
        only3 = {k: v for k, v in ranks.items() if not k.endswith("_2d")}
        EV.accumulate(full, ranks, cm, 1)
        EV.accumulate(only, only3, cm, 1)                                  # the 2D keys missing
        EV.accumulate(kept, dict(only3, top_k_obj_2d=None, top_k_rel_2d=None, top_k_triplet_2d=None), cm, 1)    # ... or None
        EV.accumulate_split(sfull, ranks["top_k_triplet"], ranks["top_k_triplet_2d"], cm, table)
        EV.accumulate_split(sonly, ranks["top_k_triplet"], None, cm, table)
        EV.accumulate_split(skept, ranks["top_k_triplet"], None, cm, table)
    return (F, full, only, kept), (S, sfull, sonly, skept)


def _recall_counts(seed, scenes=4):
    """per-scene counts in metrics.recallk_counts' layout: gt edges, gt per class, then per variant hit@K and class hits"""
    g = torch.Generator().manual_seed(seed)
    c = torch.zeros(scenes, recallk_width(R), dtype=torch.int64)
    gtc = torch.randint(0, 4, (scenes, R), generator=g)
    gtc[1] = 0                                                              # a scene without gt edges
    c[:, 1:1 + R] = gtc
    c[:, 0] = gtc.sum(1)
    c[:, 1 + R:] = torch.minimum(torch.randint(0, 4, (scenes, recallk_width(R) - 1 - R), generator=g), c[:, :1])
    return c


def test_accumulators_skip_a_missing_2d_input():
    (F, full, only, kept), (S, sfull, sonly, skept) = _vectors()
    assert full[F.index("tri_n_2d")] > 0 and sfull[S.index("zs_n_2d")] > 0
    _check_vec(F, only, full)
    _check_vec(F, kept, full, in_2d=7.0)
    _check_vec(S, sonly, sfull)
    _check_vec(S, skept, sfull, in_2d=7.0)
    c3, c2 = _recall_counts(11), _recall_counts(12)
    c2[:, :1 + R] = c3[:, :1 + R]                                           # (the gt counts depend on the labels only)
    RF = EV.recall_fields()
    vfull, vonly = EV.recall_vector(c3, c2, R), EV.recall_vector(c3, None, R)
    assert vonly.dtype == torch.float64 and vonly.shape == vfull.shape == (len(RF),)
    _check_vec(RF, vonly.numpy(), vfull.numpy())
    assert any(v for f, v in zip(RF, vfull.tolist()) if _is_2d(f))


def test_summaries_without_the_2d_branch_and_defaults_unchanged():
    (F, full, only, _), (S, sfull, sonly, _) = _vectors()
    c3, c2 = _recall_counts(11), _recall_counts(12)
    c2[:, :1 + R] = c3[:, :1 + R]
    vfull, vonly = EV.recall_vector(c3, c2, R).numpy(), EV.recall_vector(c3, None, R).numpy()
    # from the two-branch vectors and from the 3D-only ones: the same 3D values either way
    for vec, rvec, svec in ((full, vfull, sfull), (only, vonly, sonly)):
        _check_summary(EV.summarize(vec, use_2d=False), EV.summarize(full))
        _check_summary(EV.recall_summarize(rvec, use_2d=False), EV.recall_summarize(vfull))
        _check_summary(EV.split_summarize(svec, use_2d=False), EV.split_summarize(sfull))
        whole, whole_full = np.concatenate([vec, rvec, svec]), np.concatenate([full, vfull, sfull])
        _check_summary(EV._summaries(whole, True, True, use_2d=False), EV._summaries(whole_full, True, True))
        _check_summary(EV._summaries(np.concatenate([vec, svec]), False, True, use_2d=False),
                       EV._summaries(np.concatenate([full, sfull]), False, True))
        _check_summary(EV._summaries(vec, False, False, use_2d=False), EV.summarize(full))
    s = EV.summarize(only, use_2d=False)
    assert s["scenes"] == 3 and 0 < s["tri_acc@100_3d"] <= 100 and len(s) == 1 + 8 + 2 + 3
    assert len(EV.recall_summarize(vonly, use_2d=False)) == 4 * 3 * 4 and len(EV.split_summarize(sonly, use_2d=False)) == 6
    # the defaults: what the functions returned before they took the argument (both branches, all keys)
    for default, explicit in ((EV.summarize(full), EV.summarize(full, R, True)), (EV.recall_summarize(vfull), EV.recall_summarize(vfull, R, True)),
                              (EV.split_summarize(sfull), EV.split_summarize(sfull, True)),
                              (EV._summaries(np.concatenate([full, vfull, sfull]), True, True),
                               EV._summaries(np.concatenate([full, vfull, sfull]), True, True, True))):
        assert list(default) == list(explicit) and all(_same(default[k], explicit[k]) for k in default)
        assert any(_is_2d(k) for k in default)
    assert len(EV.summarize(full)) == 1 + 2 * 13 and len(EV.recall_summarize(vfull)) == 2 * 48 and len(EV.split_summarize(sfull)) == 12
    assert len(EV.fields()) == 361 and len(EV.split_fields()) == 12 and len(EV.recall_fields()) == 2 + R + 2 * 4 * 3 * (3 + R)
