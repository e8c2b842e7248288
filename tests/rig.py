"""Shared scaffolding of the step-level and two-rank GPU tests: a process-wide fault latch, the launcher of the rank children (with its worker-side helpers) and
the small training step's seeded models, data pair, launch counts and byte snapshots.  An ordinary module: nothing runs at import, and torch / dcvgan_amd are
imported inside the functions, so a worker can import it before init_process_group.  Whatever differs between the callers is an argument."""
import hashlib
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# ---- 1. fault latch ---------------------------------------------------------------------------------------------------------------------------------------------
FAULTED = []                   # reasons; once non-empty, nothing else that asks stop_after_fault() is started on the GPU in this session
FAULT_STATUS = (134, 139, 124, 137)      # abort, segmentation fault, time limit (as exit statuses; a negative status is a signal)


def _reset_for_tests():
    FAULTED.clear()


def sync():
    """torch.cuda.synchronize() that remembers a device fault."""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        FAULTED.append(str(e)[:200])
        raise


def stop_after_fault():
    """After a device fault nothing else is started on the GPU."""
    if FAULTED:
        pytest.fail(f"not run: the device reported a fault earlier in this session ({FAULTED[0]})")


# ---- 2. rank launcher -------------------------------------------------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def run_ranks(worker, tmp_path, *extra, tag="", world=2, timeout):
    """`world` fresh children `python tests/<worker> RANK WORLD PORT OUT.json *extra` (never a re-exec of this process), each waited for with `timeout` seconds;
    -> their JSON results in rank order.  Every exit status must be 0; one that tells of a fault (a signal, FAULT_STATUS) or a timeout sets the latch, and a set
    latch keeps this from starting anything.  No retry."""
    assert world <= 2, world
    stop_after_fault()
    port = free_port()
    outs = [str(tmp_path / f"{tag}{r}.json") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, worker), str(r), str(world), str(port), outs[r], *extra], env=env) for r in range(world)]
    try:
        for r, p in enumerate(procs):
            try:
                status = p.wait(timeout=timeout)
            except subprocess.TimeoutExpired:
                FAULTED.append(f"{worker}: rank {r} still ran after {timeout} s")
                raise
            if status < 0 or status in FAULT_STATUS:
                FAULTED.append(f"{worker}: rank {r} ended with status {status}")
            assert status == 0, (worker, r, status)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return [json.load(open(o)) for o in outs]


def rank_args():
    """Worker side: -> (rank, world, port, out, extra) of the command line run_ranks() wrote."""
    return int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5:]


def init_rank(port, rank, world, **pg_kw):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = port
    dist.init_process_group("gloo", rank=rank, world_size=world, **pg_kw)


# ---- 3. step rig ------------------------------------------------------------------------------------------------------------------------------------------------
def small_cfg(name="isogd-depth", batchsize=2, width_div=8, **cfg_kw):
    from dcvgan_amd.configs import CONFIGS
    return CONFIGS[name].scaled(batchsize=batchsize, width_div=width_div, **cfg_kw)


def share_rng(models, philox_seed):
    """One PhiloxRng(philox_seed) as the random source of every model; -> it."""
    from dcvgan_amd.rng import PhiloxRng
    r = PhiloxRng(philox_seed)
    for m in models.values():
        m._rng = r
    return r


def seeded_models(cfg, device, torch_seed, philox_seed, sync_bn=False, broadcast=False):
    """manual_seed -> build_models -> (broadcast_module) -> one Philox stream on all models; -> (models, rng)."""
    import torch
    from dcvgan_amd import optim, trainer
    torch.manual_seed(torch_seed)
    models = trainer.build_models(cfg, device, sync_bn=sync_bn) if sync_bn else trainer.build_models(cfg, device)
    if broadcast:
        for m in models.values():
            optim.broadcast_module(m)
    return models, share_rng(models, philox_seed)


def clip_pair(cfg, device, seed, batch=2, frames=16, size=64, geo_channels=None):
    """-> (colour, geometry) clips uniform in [-1, 1), drawn in that order from one host generator."""
    import torch
    g = torch.Generator().manual_seed(seed)
    geo = cfg.channel if geo_channels is None else geo_channels
    xc = (torch.rand(batch, 3, frames, size, size, generator=g) * 2 - 1).to(device)
    return xc, (torch.rand(batch, geo, frames, size, size, generator=g) * 2 - 1).to(device)


def counted_steps(runner, xc, xg, ts, strict_from=0):
    """runner.step at every t of `ts`; -> (kernel launches per step, outputs).  From step index `strict_from` on a host synchronisation is an error (an
    iteration that still builds workspaces or optimiser state may need one: its caller passes 1)."""
    import torch
    from dcvgan_amd import native
    counts, outs = [], []
    try:
        for i, t in enumerate(ts):
            if i == strict_from:
                torch.cuda.set_sync_debug_mode("error")
            n0 = native.launch_count()
            outs.append(runner.step(xc, xg, t))
            counts.append(native.launch_count() - n0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return counts, outs


def byte_view(t):
    import torch
    return t.detach().cpu().reshape(-1).view(torch.uint8)


def state_bytes(models, opts=None, names=None):
    """-> {(model, key): bytes as a uint8 tensor} of every state_dict entry of models[n], n in `names` (default trainer.MODEL_NAMES), and with `opts` of both
    Adam moments of every parameter."""
    import torch
    from dcvgan_amd import trainer
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    snap = {}
    for n in (trainer.MODEL_NAMES if names is None else names):
        for k, v in models[n].state_dict().items():
            snap[(n, k)] = byte_view(v).clone()
        for i, p in enumerate(models[n].parameters() if opts is not None else ()):
            s = opts[n].state[p]
            snap[(n, i, "m")], snap[(n, i, "v")] = byte_view(s["exp_avg"]).clone(), byte_view(s["exp_avg_sq"]).clone()
    return snap


def sha_of(tensors):
    """SHA-256 of the tensors' bytes, in order."""
    return hashlib.sha256(b"".join(byte_view(t).numpy().tobytes() for t in tensors)).hexdigest()
