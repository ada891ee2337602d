#!/usr/bin/env python3
"""Record of the checkpoint directory the REAL reference's BaseModel.save() writes (imported read-only through the
stand-ins of make_golden.py), for tests/test_checkpoint_cpu.py::test_reads_what_the_real_reference_saves:

    python tests/golden/make_golden_checkpoint.py        ->  tests/golden/reference_checkpoint_l1.json

The directory itself is ~64 MB (one .pth per top-level sub-module, formula weights of an L=1 model, seed 5), so only
its description is stored: every file name, the top-level keys of every file, and for each tensor of a `model`
state_dict its shape, dtype and the SHA-256 of its bytes; the `config_best.pth` dict verbatim.  The test rebuilds an
equivalent directory from this record (checking the recorded digests against vlsat_amd.synth) and reads it with
vlsat_amd.checkpoint.
"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
from vlsat_amd import VLSATConfig  # noqa: E402


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    MG.install_standins()
    cfg = VLSATConfig(N_LAYERS=1)
    m = MG.build_reference(1)
    MG.load_formula_weights(m, cfg, seed=5)
    m.eva_res, m.iteration = 12.0, 33
    m.save()                                         # BaseModel.save -> one .pth per sub-module
    files = {}
    for f in sorted(os.listdir(m.saving_pth)):
        obj = torch.load(os.path.join(m.saving_pth, f), map_location="cpu", weights_only=False)
        entry = {"keys": sorted(obj)}
        if f.startswith("config"):
            entry["value"] = {k: obj[k] for k in sorted(obj)}
        elif isinstance(obj.get("model"), dict) and all(isinstance(v, torch.Tensor) for v in obj["model"].values()):
            entry["model"] = [[k, list(v.shape), str(v.dtype).replace("torch.", ""), digest(v)] for k, v in obj["model"].items()]
        files[f] = entry
    out = os.path.join(HERE, "reference_checkpoint_l1.json")
    with open(out, "w") as fh:
        json.dump({"what": "files BaseModel.save() writes for an L=1 Mmgnet holding vlsat_amd.synth.make_weights(seed=5), "
                           "eva_res=12.0, iteration=33", "files": files}, fh, indent=0)
        fh.write("\n")
    print(out, os.path.getsize(out), "bytes,", len(files), "files")


if __name__ == "__main__":
    main()
