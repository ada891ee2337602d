"""Reference checkpoint directory layout (model_base.py:47-129): round trip, DataParallel key
prefix, best/last selection -- and the files written by the REAL reference's BaseModel.save(),
rebuilt from their record under tests/golden/."""
import hashlib
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, synth
from vlsat_amd import checkpoint as CK


def test_round_trip_and_selection(tmp_path):
    cfg = VLSATConfig(N_LAYERS=1)
    w = synth.make_weights(cfg, seed=3)
    d = str(tmp_path / "ckp" / "Mmgnet" / "exp")
    CK.save_reference_checkpoint(d, w, best=True, iteration=700, eva_res=41.5, data_parallel=True)
    got, meta = CK.load_reference_checkpoint(d, cfg, best=True)
    assert meta == {"iteration": 700, "eva_res": 41.5, "suffix": "_best.pth"}
    assert set(got) == set(w) and all(np.array_equal(got[k], w[k]) for k in w)
    assert sorted(f for f in os.listdir(d) if f.startswith("mmg")) == ["mmg_best.pth"]
    # a later plain checkpoint wins when best=False (model_base.py:88-96)
    w2 = {k: v + 1 for k, v in w.items()}
    CK.save_reference_checkpoint(d, w2, best=False, iteration=900)
    got2, meta2 = CK.load_reference_checkpoint(d, cfg, best=False)
    assert meta2["suffix"] == ".pth" and np.array_equal(got2["mlp_3d.0.bias"], w2["mlp_3d.0.bias"])
    assert CK.load_reference_checkpoint(d, cfg, best=True)[1]["suffix"] == "_best.pth"
    os.remove(os.path.join(d, "mmg.pth"))
    with pytest.raises(FileNotFoundError):
        CK.load_reference_checkpoint(d, cfg, best=False)
    with pytest.raises(KeyError):
        CK.load_reference_checkpoint(d, VLSATConfig(N_LAYERS=2), best=True)       # layer 1 tensors absent


def test_reads_what_the_real_reference_saves(tmp_path, golden_dir):
    """The directory the real reference's BaseModel.save() wrote for an L=1 model holding the seed-5 formula weights, rebuilt
    from its record (tests/golden/make_golden_checkpoint.py): the same files, keys, shapes and dtypes, and every tensor the
    loader reads byte-identical to what the reference saved (SHA-256 of the recorded tensor against synth)."""
    cfg = VLSATConfig(N_LAYERS=1)
    want = synth.make_weights(cfg, seed=5)
    rec = json.load(open(os.path.join(golden_dir, "reference_checkpoint_l1.json")))["files"]
    d = tmp_path / "ckp" / "Mmgnet" / "golden"
    d.mkdir(parents=True)
    matched = 0
    for fname, entry in rec.items():
        if "value" in entry:
            obj = dict(entry["value"])
        elif "model" in entry:
            mod = fname[:-len("_best.pth")]
            sd = OrderedDict()
            for key, shape, dtype, sha in entry["model"]:
                full = f"{mod}.{key}"
                if full in want:
                    t = torch.from_numpy(want[full])
                    assert list(t.shape) == shape and str(t.dtype) == "torch." + dtype, (full, shape, dtype)
                    assert hashlib.sha256(t.numpy().tobytes()).hexdigest() == sha, f"{full}: not what the reference saved"
                    matched += 1
                else:                                # dead at eval (triplet projectors, logit scale, BN counters): any value
                    t = torch.zeros(shape, dtype=getattr(torch, dtype))
                sd[key] = t
            obj = {"model": sd}
        else:
            obj = {k: {} for k in entry["keys"]}     # optimizer / lr_scheduler state: not read by the loader
        torch.save(obj, d / fname)
    assert matched == len(want)
    got, meta = CK.load_reference_checkpoint(str(d), cfg, best=True)
    assert meta["iteration"] == 33 and meta["eva_res"] == 12.0 and meta["suffix"] == "_best.pth"
    assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
