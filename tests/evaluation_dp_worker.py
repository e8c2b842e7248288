"""Child process of tests/test_evaluation_dp_gpu.py: one data-parallel rank (gloo, cuda:0).  The rank accumulates its half of the rows — integer-valued features,
so every sum is exact in any order, and logits — into a FeatureMoments and an InceptionStats, all-reduces both and writes the states it then holds.
Usage: python tests/evaluation_dp_worker.py RANK WORLD PORT OUT.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import rig  # noqa: E402

N_ROWS, DIM, CLASSES = 37, 80, 7      # rows over both ranks (an odd count: the halves differ), feature and class counts


def data():
    """-> (features (N_ROWS, DIM) fp32 integers in [-8, 8], logits (N_ROWS, CLASSES) fp32), the same on every rank."""
    g = np.random.default_rng(2024)
    return g.integers(-8, 9, size=(N_ROWS, DIM)).astype(np.float32), (g.standard_normal((N_ROWS, CLASSES)) * 3.0).astype(np.float32)


def rows_of(rank, world):
    return slice(rank * N_ROWS // world, (rank + 1) * N_ROWS // world)


def main():
    import torch
    import torch.distributed as dist
    rank, world, port, out, _ = rig.rank_args()
    rig.init_rank(port, rank, world)
    from dcvgan_amd import evaluation as E
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    feats, logits = data()
    mine = rows_of(rank, world)
    fm = E.FeatureMoments(DIM, dev).update(torch.from_numpy(feats[mine]).to(dev))
    st = E.InceptionStats(CLASSES, dev).update(torch.from_numpy(logits[mine]).to(dev))
    res = {"rank": rank, "n_before": [fm.n, st.n]}
    fm.all_reduce()
    st.all_reduce()
    torch.cuda.synchronize()
    sd = fm.state_dict()
    res.update(n=[fm.n, st.n], sum=sd["sum"].tolist(), gram=sd["gram"].tolist(), inception=st.state_host().tolist(), score=st.score())
    json.dump(res, open(out, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
