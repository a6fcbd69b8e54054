#!/usr/bin/env python3
"""
Generate tests/golden/cond.npz by RUNNING THE REFERENCE's conditioning modules on the CPU (nn.py:103-121
timestep_embedding; unet.py time_embed, label_emb and every ResBlock's emb_layers, in module order):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cond.py

Build container only, like make_golden.py, whose helpers (flags, TINY, PUBLISHED, synth) it reuses.  Stored: the
reference's OUTPUTS, the timesteps, the labels and the seeds; the parameters are regenerated on both sides from
guided_diffusion/synth.py (only the parameters this path reads are set: the convolutions keep their construction-time
values, which nothing here evaluates).  Models, timesteps and row counts are tests/cond_ref.py's (MODELS, GOLDEN_T,
GOLDEN_ROWS: the published widths have 18 176 columns a row, so seven rows of them).

Per model tag:  <tag>/emb   time_embed(timestep_embedding(t, mc)) [+ label_emb(y)]         [rows, 4 mc]
                <tag>/rows  every ResBlock's emb_layers(emb), concatenated in module order  [rows, film_total]
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
from make_golden import flags, ref_su, ref_unet, synth  # noqa: E402
from guided_diffusion import nn as ref_nn  # noqa: E402  (the reference's, imported by make_golden)

sys.path.insert(0, os.path.dirname(HERE))
import cond_ref as CR  # noqa: E402


def load_cond_synth(model, seed):
    sd = model.state_dict()
    with torch.no_grad():
        for k, _ in CR.cond_keys((k, tuple(v.shape)) for k, v in sd.items()):
            sd[k].copy_(torch.from_numpy(synth.synth_param(k, tuple(sd[k].shape), seed)))
    model.eval()


if __name__ == "__main__":
    torch.manual_seed(0)
    out = {"t": CR.GOLDEN_T, "seed_y": np.array([CR.GOLDEN_SEED_Y], dtype=np.int64)}
    for tag, (fl, seed) in CR.MODELS.items():
        model, _ = ref_su.sr_create_model_and_diffusion(**flags(**fl))
        load_cond_synth(model, seed)
        R = CR.GOLDEN_ROWS[tag]
        t = torch.from_numpy(CR.GOLDEN_T[:R])
        blocks = [m for m in model.modules() if isinstance(m, ref_unet.ResBlock)]
        with torch.no_grad():
            emb = model.time_embed(ref_nn.timestep_embedding(t, model.model_channels))
            if model.num_classes is not None:
                y = CR.golden_labels(R, model.num_classes)
                out[tag + "/y"] = y
                emb = emb + model.label_emb(torch.from_numpy(y))
            rows = torch.cat([b.emb_layers(emb) for b in blocks], dim=1)
        out[tag + "/seed"] = np.array([seed], dtype=np.int64)
        out[tag + "/emb"] = emb.numpy()
        out[tag + "/rows"] = rows.numpy()
        print(tag, len(blocks), "ResBlocks", tuple(emb.shape), tuple(rows.shape), flush=True)
    path = os.path.join(HERE, "cond.npz")
    np.savez_compressed(path, **out)
    print("wrote cond.npz", os.path.getsize(path), "bytes")
