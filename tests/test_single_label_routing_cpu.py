"""Which route ``metrics.process_val_counts`` takes for a single-label model (``MODEL.multi_rel_outputs = false``), without a GPU
and without the library: a stub model whose ``process_val_counts`` records its arguments, and whose forward -- the first step of the
separate-call route -- records the call and stops the test there (``SeparateCalls``), since everything after it needs the device.
One call: the stub's method exactly once, no forward, the target handed over as the int64 [E, R] one-hot matrix with column 0
("none") cleared, and ``single_label=True`` (VLSATModel.process_val_counts keeps its refusal of such a model for callers that do not pass it).  ``recall=`` given, or the method answering False (a plan that had to permute the edges): the separate calls."""
from types import SimpleNamespace

import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, metrics as M

R, N, E = 9, 4, 12


class SeparateCalls(Exception):
    """the stub's forward was reached: the separate-call route"""


class Stub:
    def __init__(self, multi, answer=True):
        self.config = SimpleNamespace(multi_rel_outputs=multi, num_rel_class=R, num_obj_class=20)
        self.answer, self.one_call, self.forwards = answer, [], []

    def process_val_counts(self, counts, obj_points, obj_2d_feats, gt_cls, descriptor, gt_rel_multihot, edges_e2, batch_ids=None, n_scenes=1,
                           fc_sizes=None, single_label=False, **split):
        self.one_call.append(dict(counts=counts, obj_2d_feats=obj_2d_feats, gt_cls=gt_cls, gt_rel=gt_rel_multihot, edges=edges_e2, n_scenes=n_scenes,
                                  fc_sizes=fc_sizes, single_label=single_label, split=split))
        return self.answer

    def __call__(self, *args, **kw):
        self.forwards.append("forward")
        raise SeparateCalls

    def forward_3d(self, *args, **kw):
        self.forwards.append("forward_3d")
        raise SeparateCalls


def _inputs():
    g = torch.Generator().manual_seed(1)
    labels = torch.tensor([0, 3, 0, 8, 1, 0, 0, 2, 5, 0, 7, 4], dtype=torch.int32)        # half 'none'; an int32 loader tensor
    edges = torch.tensor([[a, b] for a in range(N) for b in range(N) if a != b])
    return dict(obj_points=torch.rand(N, 3, 8, generator=g), obj_2d_feats=torch.rand(N, 512, generator=g), gt_cls=torch.randint(0, 20, (N,), generator=g),
                descriptor=torch.rand(N, 11, generator=g), gt_rel_cls=labels, edge_indices=edges)


def _run(model, x, use_2d=True, **kw):
    counts = torch.zeros(len(EV.fields(R)), dtype=torch.int64)
    got = M.process_val_counts(model, counts, x["obj_points"], x["obj_2d_feats"] if use_2d else None, x["gt_cls"], x["descriptor"], x["gt_rel_cls"],
                               x["edge_indices"], None, 1, [N], **kw)
    return counts, got


@pytest.mark.parametrize("use_2d", [True, False])
def test_single_label_model_takes_the_one_call(use_2d):
    model, x = Stub(multi=False), _inputs()
    counts, got = _run(model, x, use_2d)
    assert len(model.one_call) == 1 and model.forwards == [], (len(model.one_call), model.forwards)    # (the parent ran the forward here)
    assert got is counts
    call = model.one_call[0]
    hot = call["gt_rel"]
    assert hot.dtype == torch.int64 and tuple(hot.shape) == (E, R) and hot.is_contiguous()
    labels = x["gt_rel_cls"].long()
    want = torch.zeros(E, R, dtype=torch.int64)
    want[torch.arange(E), labels] = 1
    want[:, 0] = 0
    assert torch.equal(hot, want)
    assert int(hot[:, 0].sum()) == 0 and hot.sum(1).tolist() == (labels > 0).long().tolist()
    assert call["counts"] is counts and call["n_scenes"] == 1 and call["fc_sizes"] == [N] and call["split"] == {}
    assert call["single_label"] is True                                   # the model is named as single-label: the method refuses it otherwise
    assert (call["obj_2d_feats"] is None) == (not use_2d)
    assert call["gt_cls"].dtype == torch.int64 and call["edges"].dtype == torch.int64 and tuple(call["edges"].shape) == (E, 2)


def test_the_split_vectors_travel_with_the_one_call():
    model, x = Stub(multi=False), _inputs()
    table, split = torch.zeros(20 * 20 * R, dtype=torch.uint8), torch.zeros(12, dtype=torch.int64)
    _run(model, x, split_table=table, split_counts=split)
    assert len(model.one_call) == 1 and model.forwards == []
    assert model.one_call[0]["split"]["split_table"] is table and model.one_call[0]["split"]["split_counts"] is split


@pytest.mark.parametrize("multi", [False, True])
def test_recall_or_a_permuted_plan_take_the_separate_calls(multi):
    x = _inputs()
    if multi:
        x["gt_rel_cls"] = torch.nn.functional.one_hot(x["gt_rel_cls"].long(), R)
    model = Stub(multi)                                                   # recall= given: the one call is not tried
    with pytest.raises(SeparateCalls):
        _run(model, x, recall=torch.zeros(len(EV.recall_fields(R)), dtype=torch.float64))
    assert model.one_call == [] and model.forwards == ["forward"]
    model = Stub(multi, answer=False)                                     # the method answered False: nothing enqueued, the separate calls follow
    with pytest.raises(SeparateCalls):
        _run(model, x)
    assert len(model.one_call) == 1 and model.forwards == ["forward"] and model.one_call[0]["single_label"] is (not multi)
    model = Stub(multi, answer=False)
    with pytest.raises(SeparateCalls):
        _run(model, x, use_2d=False)
    assert len(model.one_call) == 1 and model.forwards == ["forward_3d"]


def test_the_loop_vectors_follow_the_models_relation_classes():
    """validation() lays its additive vectors out for the model's own num_rel_class (a model without a config: the reference's 26),
    the length the one call writes for that model"""
    assert EV._model_n_rel(Stub(multi=False)) == R and EV._model_n_rel(object()) == EV.N_REL == 26
    assert len(EV.fields(R)) == 1 + R + 2 * (11 + 6 * R)
