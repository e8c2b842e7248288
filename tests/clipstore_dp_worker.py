"""Child process of tests/test_clipstore_dp_gpu.py: one data-parallel rank (gloo, cuda:0).  Every rank builds the same store from a seed and a ClipSampler whose
rank and world come from torch.distributed; for each of ITERATIONS batches (they cross an epoch boundary) it compares its own batch with its slice of the batch a
single-process sampler of batch size B x world makes on the same store.  The sampler makes no collective call; the only ones here are this check's own
all_gathers, which put the ranks' batches side by side.
Usage: python tests/clipstore_dp_worker.py RANK WORLD PORT OUT.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import rig  # noqa: E402

T, H, W, B = 16, 12, 10, 3
COUNTS = [T, T + 1, 40, T + 3, 25, T, T + 1, 31, T + 2, 60, T + 1, 19, 22]      # 13 videos: two iterations of 2 x 3 clips per epoch, one video dropped
ITERATIONS = 5
SEED = 77


def main():
    import torch
    import torch.distributed as dist
    rank, world, port, out, _ = rig.rank_args()
    rig.init_rank(port, rank, world)
    from dcvgan_amd import clipstore as CS
    from dcvgan_amd import native
    native.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(4)
    videos = [(rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8), rng.integers(0, 256, size=(n, H, W, 1), dtype=np.uint8)) for n in COUNTS]
    st = CS.ClipStore.from_arrays(videos, T, "depth", dev)
    torch.manual_seed(SEED)                       # the samplers' seed follows torch's, the same on every rank
    mine = CS.ClipSampler(st, B)                  # rank and world from torch.distributed
    whole = CS.ClipSampler(st, B * world, rank=0, world=1)
    res = {"rank": rank, "sampler_rank": mine.rank, "sampler_world": mine.world, "len": [len(mine), len(whole)], "slice_equal": [], "gathered_equal": [],
           "table_equal": [], "sha": [], "state": []}
    for it in range(ITERATIONS):
        b, full = mine.next_batch(), whole.next_batch()
        torch.cuda.synchronize()
        sl = slice(rank * B, (rank + 1) * B)
        res["slice_equal"].append(bool(torch.equal(b["color"], full["color"][sl]) and torch.equal(b["depth"], full["depth"][sl])))
        res["table_equal"].append(bool(torch.equal(mine.last_table, whole.last_table[sl])))
        ok = True
        for k in ("color", "depth"):              # the check's own collective: the ranks' batches concatenated are the single-process batch, byte for byte
            parts = [torch.empty(b[k].shape, dtype=torch.float32) for _ in range(world)]
            dist.all_gather(parts, b[k].cpu())
            ok = ok and bool(torch.equal(torch.cat(parts), full[k].cpu()))
        res["gathered_equal"].append(ok)
        res["sha"].append(rig.sha_of([b["color"], b["depth"]]))
        res["state"].append([mine.epoch, mine.iteration])
    json.dump(res, open(out, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
