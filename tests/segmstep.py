"""Shared by the CPU and GPU tests that step the shipped segmentation configuration (`CONFIGS["surreal-segm"]` at an eighth of its widths, B = 2):
the clips, the same-seed initial states and the schedule of frame indices.  The seeds are those of the calibration the arg-max conditions of
oracle/stepcheck.py were measured on (tools/stepcheck_reference.py segm -> profiles/stepcheck_segm.txt): with them iteration 3 of the reference's own
fp32 arithmetic has ONE pixel of 131 072 whose two largest softmax values differ by 2.0e-9 in fp64 and which fp32 assigns to the other part."""
import numpy as np
import torch

from oracle import dcvgan_oracle as O
from tests import goldenio as G

T_RANDS = (5, 11, 2, 7)
SEED_RUN = 2
SEED_DATA = 78
B = 2


def config():
    from dcvgan_amd.configs import CONFIGS
    return CONFIGS["surreal-segm"].scaled(batchsize=B, width_div=8)


def calibration_clips():
    """(colour clip uniform in [-1, 1), one-hot part maps): the real batch of the calibration."""
    return G.real_clips(B, 25, SEED_DATA)


def clip_bytes():
    """What a loader hands over: uint8 part labels (B, T, H, W) as in segm.npy — the labels of `calibration_clips` — and uint8 colour frames
    (B, T, H, W, 3) in disk order."""
    gd = torch.Generator().manual_seed(SEED_DATA)
    torch.rand(B, 3, 16, 64, 64, generator=gd)
    labels = torch.randint(0, 25, (B, 16, 64, 64), generator=gd)
    color = torch.randint(0, 256, (B, 16, 64, 64, 3), generator=gd)
    return labels.numpy().astype(np.uint8), color.numpy().astype(np.uint8)


def decoded(labels, color_u8):
    """dataset.py:127-131 for the colour frames and dataset.py:176-181 (np.eye(25)[labels], transposed) for the labels, per clip."""
    xc = torch.from_numpy(np.ascontiguousarray(color_u8.transpose(0, 4, 1, 2, 3)).astype(np.float32) / 127.5 - 1.0)
    xg = torch.from_numpy(np.stack([O.segmentation_one_hot(l) for l in labels]))
    return xc, xg


def initial_states(cfg):
    """-> (models on the CPU, their state dicts as the oracle's states), built in the reference's order under cfg.seed."""
    from dcvgan_amd import trainer
    torch.manual_seed(cfg.seed)
    models = trainer.build_models(cfg, torch.device("cpu"))
    return models, {n: {k: v.detach().clone() for k, v in m.state_dict().items()} for n, m in models.items()}
