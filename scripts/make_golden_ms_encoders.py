"""Writes tests/golden/ms_encoders.pt and tests/golden/ms_encoders_<key>.pt from the reference's OWN multi-scale encoders
(ptlflow/models/ccmr/extractor.py `BasicEncoder_resconv` / `Basic_Context_Encoder_resconv` as CCMR and CCMR+,
ptlflow/models/ms_raft_plus/extractor.py `BasicEncoder` / `Basic_Context_Encoder`), imported unmodified through oracle/ref_loader.py
(which stands in for torchvision's `TF.resize`: bilinear, align_corners=False, antialias on); build container only, CPU:

    python scripts/make_golden_ms_encoders.py

Each class gets the seeded parameter recipe of tests/msenc_model.py (`recipe_state_dict`, loaded strictly) in float64 and runs on the
seeded 32 x 48 pair `golden_input()`: the feature encoders on the pair, the context encoders on its first image.  Stored — settings,
names, shapes and recorded results only, no parameter values:

    ms_encoders.pt          input [2, 3, 32, 48] float64; per encoder key: the recipe's seed, the state_dict names and shapes, and a
                            float64 (sum, sum of magnitudes) per parameter
    ms_encoders_<key>.pt    every pyramid level's output, coarse to fine, rounded to float32 (a feature encoder's two halves
                            concatenated again along the batch) — one file per encoder, so that each stays below 1 MiB
"""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from msenc_model import ENCODERS, SEEDS, golden_input, recipe_state_dict  # noqa: E402
from oracle import ref_loader  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main() -> None:
    ref_loader.load()
    x = golden_input()
    meta = {"input": x, "encoders": {}}
    for key, (cls, _kw, (mod, name, kw)) in ENCODERS.items():
        ref = getattr(ref_loader.ref_module(mod), name)(**kw).double().eval()
        shapes = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
        sd = recipe_state_dict(shapes, SEEDS[key], torch.float64)
        ref.load_state_dict(sd, strict=True)
        with torch.no_grad():
            outs = ref([x[0:1], x[1:2]]) if cls.split_pairs else ref(x[0:1])
        levels = [(torch.cat(list(o), 0) if cls.split_pairs else o).float().contiguous() for o in outs]
        meta["encoders"][key] = {"seed": SEEDS[key], "shapes": shapes,
                                 "checksums": {k: (float(v.sum()), float(v.abs().sum())) for k, v in sd.items()},
                                 "levels": [tuple(o.shape) for o in levels]}
        path = os.path.join(GOLDEN, f"ms_encoders_{key}.pt")
        torch.save(levels, path)
        print(f"wrote {path}: {os.path.getsize(path)} bytes, levels {[tuple(o.shape) for o in levels]}")
    path = os.path.join(GOLDEN, "ms_encoders.pt")
    torch.save(meta, path)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
