"""CPU: the synchronised-BatchNorm entries are declared, exported and bound alike; marking touches exactly the BatchNorm2d / BatchNorm3d modules; and the
exchange — an all-reduce(SUM) of a zeroed table in which each rank filled its own row — returns the same table on every rank (gloo, host tensors)."""
import datetime
import os
import re
import socket

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dcv_bn_sync_row_doubles", "dcv_bn_sync_sums", "dcv_bn_sync_finalize", "dcv_bn_sync_backward_sums", "dcv_bn_sync_backward_apply")


def test_header_and_binding_agree_on_the_new_entries():
    import ctypes
    from dcvgan_amd import native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dcvgan_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\b(size_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/dcvgan_hip.h"
        assert name in native.EXPORTS
        res, args = native._SIGS[name]
        assert len(args) == len(m.group(2).split(",")), name          # one ctypes type per declared parameter
        assert res is (ctypes.c_size_t if m.group(1) == "size_t" else ctypes.c_int)
    L = native.lib()                                                  # every bound name resolves in the library (AttributeError otherwise)
    assert L.dcv_version() == native.ABI_VERSION == 4                 # added symbols only
    assert L.dcv_bn_sync_row_doubles(5) == 11 and L.dcv_bn_sync_row_doubles(0) == 0
    # argument checks need no GPU: nothing is launched for a call without tensors
    n0 = L.dcv_launch_count()
    assert L.dcv_bn_sync_sums(None, None, None, 0, 0, None, None, 0, None) == native.DCV_EINVAL
    assert L.dcv_bn_sync_finalize(None, 2, 4, 1e-5, 0.1, None, None, None, None, None, None) == native.DCV_EINVAL
    assert L.dcv_launch_count() == n0


def test_marking_touches_exactly_the_batchnorm_2d_and_3d_modules():
    import torch.nn as nn
    from dcvgan_amd import optim
    net = nn.Sequential(nn.Conv2d(3, 4, 1), nn.BatchNorm2d(4), nn.LeakyReLU(0.2), nn.Sequential(nn.Conv3d(4, 4, 1), nn.BatchNorm3d(4)), nn.BatchNorm1d(4),
                        nn.GroupNorm(2, 4), nn.Dropout2d(0.5))
    other = nn.ModuleList([nn.BatchNorm2d(2)])
    assert optim.sync_bn_group_of(net) is None
    keys = sorted(net.state_dict())
    h = optim.sync_batchnorm(net, force=True)
    marked = [m for m in net.modules() if "_dcv_sync_bn" in m.__dict__]
    assert [type(m) for m in marked] == [nn.BatchNorm2d, nn.BatchNorm3d] and all(m._dcv_sync_bn is h for m in marked)
    assert h.world == 1 and h.rank == 0 and h.force and h.active and optim.sync_bn_group_of(net) is h
    assert sorted(net.state_dict()) == keys                           # a mark is no parameter and no buffer
    assert "_dcv_sync_bn" not in other[0].__dict__
    # a dict of models (trainer.build_models' result) and an existing handle
    h2 = optim.sync_batchnorm({"a": net, "b": other}, group=h)
    assert h2 is h and other[0]._dcv_sync_bn is h
    optim.unsync_batchnorm(net)
    assert not [m for m in net.modules() if "_dcv_sync_bn" in m.__dict__] and other[0]._dcv_sync_bn is h
    optim.unsync_batchnorm([other])
    assert optim.sync_bn_group_of(other) is None
    # without force a world of one is not active: layers.batch_norm stays on the local route
    assert not optim.sync_batchnorm(net).active


def test_build_models_marks_on_request_only():
    from dcvgan_amd import optim, trainer
    from dcvgan_amd.configs import CONFIGS
    import torch.nn as nn
    cfg = CONFIGS["isogd-depth"].scaled(batchsize=2, width_div=16)
    cpu = torch.device("cpu")
    assert optim.sync_bn_group_of(trainer.build_models(cfg, cpu)) is None
    models = trainer.build_models(cfg, cpu, sync_bn=True)
    bns = [m for net in models.values() for m in net.modules() if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d))]
    assert len(bns) == 23                                             # the reference's 23 BatchNorm groups
    assert all(m.__dict__.get("_dcv_sync_bn") is optim.sync_bn_group_of(models) for m in bns)


def _exchange_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    from dcvgan_amd import optim
    grp = optim.SyncBnGroup()
    ok = grp.world == world and grp.rank == rank and grp.active and grp.pg is not None
    channels = 5
    rows = grp.table(channels, torch.device("cpu"))
    ok = ok and tuple(rows.shape) == (world, 2 * channels + 1) and rows.dtype == torch.float64 and not rows.any()
    g = torch.Generator().manual_seed(100 + rank)
    mine = torch.randn(2 * channels + 1, generator=g, dtype=torch.float64) * 1e3 + 1 / 3
    mine[-1] = float(3 * rank + 1)                                    # uneven counts: 1, 4, 7 values per channel
    rows[rank] = mine
    grp.exchange(rows)
    want = torch.stack([torch.randn(2 * channels + 1, generator=torch.Generator().manual_seed(100 + r), dtype=torch.float64) * 1e3 + 1 / 3 for r in range(world)])
    want[:, -1] = torch.tensor([3.0 * r + 1 for r in range(world)], dtype=torch.float64)
    ok = ok and torch.equal(rows, want) and grp.collectives == 1      # adding zeros is exact: every rank holds every rank's bits
    # a subgroup: ranks outside it keep a world of one (every rank makes the call)
    sub = optim.SyncBnGroup(ranks=[0, 1])
    ok = ok and ((sub.world, sub.rank) == (2, rank) if rank < 2 else (sub.world == 1 and not sub.active))
    q.put((rank, bool(ok), rows.numpy().tobytes()))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_zero_padded_exchange_returns_the_same_table_on_every_rank(world):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_exchange_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=120) for _ in procs]
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.kill()
    assert sorted(r[:2] for r in res) == [(r, True) for r in range(world)], [r[:2] for r in res]
    assert all(r[2] == res[0][2] for r in res)
