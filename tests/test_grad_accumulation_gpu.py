"""GPU: parameter-gradient sums are formed by the library's own kernels (ops.grad_target: the weight gradient's slab reduce adds into the tensor that holds the
first contribution; dcv_axpby for BatchNorm parameters), not by autograd's at::add launches — and the result is bit-identical to autograd's.

Sums arise (a) for every discriminator parameter in the D phase (D on the real and the fake batch, trainer.py:299-309 -> :319) and (b) in the G phase on top of the
D phase's gradients (trainer.py:356; the discriminators are zeroed only at :288-290).  VERDICT r4 item 4: torch's elementwise kernels carry packed-FP32 code the
library's build flag cannot reach; this removes them from the parameter path (and ~a hundred tiny launches per iteration)."""
import pytest
import torch

from tests import rig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _run(cfg_name, B, own, cl=False, steps=2):
    from dcvgan_amd import ops, ops_cl, trainer
    from dcvgan_amd.configs import CONFIGS
    dev = torch.device("cuda:0")
    cfg = CONFIGS[cfg_name].scaled(batchsize=B)
    xc, xg = rig.clip_pair(cfg, dev, 3, batch=B)
    old = ops._OWN_ACCUMULATION
    ops._OWN_ACCUMULATION = own
    ops_cl.enable(cl)
    try:
        models, _ = rig.seeded_models(cfg, dev, 11, 5)
        runner = trainer.StepRunner(cfg, models, trainer.build_optimizers(cfg, models), trainer.build_loss(cfg), sync_losses=True)
        losses = [runner.step(xc, xg, 2 + i) for i in range(steps)]
        grads = {f"{k}.{n}": p.grad.detach().clone().cpu() for k, m in models.items() for n, p in m.named_parameters() if p.grad is not None}
        params = torch.cat([v.detach().float().reshape(-1) for m in models.values() for v in m.state_dict().values()]).cpu()
        return losses, grads, params
    finally:
        ops._OWN_ACCUMULATION = old
        ops_cl.enable(False)


def _run_schedule(name, B, companion, cl):
    from dcvgan_amd import native, ops, ops_cl, trainer
    native.lib()
    old = (ops._WGRAD_SIDE, ops_cl._WGRAD_SIDE)
    ops._WGRAD_SIDE = companion
    ops_cl.enable(cl)
    try:
        cfg = rig.small_cfg(name, B, 2)
        models, _ = rig.seeded_models(cfg, DEV, 5, 17)
        runner = trainer.StepRunner(cfg, models, trainer.build_optimizers(cfg, models), trainer.build_loss(cfg), sync_losses=True)
        xc, xg = rig.clip_pair(cfg, DEV, 6, batch=B)
        outs = [runner.step(xc, xg, t) for t in (2, 9, 5)]
        return outs, torch.cat([p.detach().reshape(-1) for m in models.values() for p in m.parameters()]).clone()
    finally:
        ops_cl.enable(False)
        ops._WGRAD_SIDE, ops_cl._WGRAD_SIDE = old


@pytest.mark.parametrize("name,cl", [("isogd-depth", False), ("surreal-depth1", False), ("isogd-flow", True)])
def test_weight_gradients_on_the_companion_stream_change_no_bit(name, cl):
    """ops.wgrad_companion: the main chain's weight gradients run on a companion stream, joined by the autograd engine's end-of-backward callback.  Same kernels, same order
    of the sums into every parameter: three iterations (one of them without a generator update for surreal-depth1) give the losses and parameters of the in-stream
    schedule, bit for bit — on the fp32 path and on the 16-bit one."""
    la, pa = _run_schedule(name, 3, True, cl)
    lb, pb = _run_schedule(name, 3, False, cl)
    assert la == lb, (la, lb)
    assert torch.equal(pa, pb)


@pytest.mark.parametrize("name,cl", [("isogd-depth", False), ("surreal-depth1", False), ("isogd-depth", True)])
def test_own_gradient_sums_equal_autograds_bit_for_bit(name, cl):
    la, ga, pa = _run(name, 4, True, cl)
    lb, gb, pb = _run(name, 4, False, cl)
    assert la == lb
    assert ga.keys() == gb.keys()
    bad = [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert not bad, bad[:5]
    assert torch.equal(pa, pb)


def test_no_torch_add_for_parameter_gradients():
    """Count torch's elementwise launches in one iteration with and without the own accumulation (torch profiler, device activity)."""
    from torch.profiler import ProfilerActivity, profile

    def adds(own):
        from dcvgan_amd import ops, trainer
        dev = torch.device("cuda:0")
        cfg = rig.small_cfg(width_div=4)
        models, _ = rig.seeded_models(cfg, dev, 1, 5)
        xc = torch.rand(2, 3, 16, 64, 64, device=dev) * 2 - 1; xg = torch.rand(2, 1, 16, 64, 64, device=dev) * 2 - 1
        old = ops._OWN_ACCUMULATION
        ops._OWN_ACCUMULATION = own
        try:
            runner = trainer.StepRunner(cfg, models, trainer.build_optimizers(cfg, models), trainer.build_loss(cfg), sync_losses=False)
            runner.step(xc, xg, 1)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                runner.step(xc, xg, 2)
                torch.cuda.synchronize()
            return sum(e.count for e in prof.key_averages() if "vectorized_elementwise_kernel" in e.key and "add" in e.key.lower())
        finally:
            ops._OWN_ACCUMULATION = old

    with_own, without = adds(True), adds(False)
    # what remains are the activation-gradient fan-ins of the trainer's own graph (the fake clips feed three discriminators) and the loss sums
    assert with_own <= without - 50, (with_own, without)


@pytest.mark.parametrize("config,cl", [("isogd-depth", False), ("surreal-depth1", False), ("surreal-depth1", True)], ids=["isogd-depth", "surreal-depth1", "surreal-depth1-bf16cl"])
def test_no_torch_compute_kernel_in_the_iteration(config, cl):
    """one iteration of StepRunner (fp32 path; adversarial and hinge loss, the latter with the gradient discriminator outside the G loss)
    launches no torch compute kernel at all — the loss sums (ops.gan_loss_sum, ops.sum_scalars), the cotangent scaling (dcv_scale_dev), the fake clips' fan-in
    (ops.fan_out), the tiled latents (ops.tile_rows) and the backward roots are the library's; what torch still does is memory copies (the loss mirrors)."""
    from torch.profiler import ProfilerActivity, profile
    from dcvgan_amd import trainer
    from dcvgan_amd import ops_cl
    dev = torch.device("cuda:0")
    cfg = rig.small_cfg(config, width_div=4)
    ops_cl.enable(cl)
    try:
        models, _ = rig.seeded_models(cfg, dev, 1, 5)
        xc = torch.rand(2, 3, 16, 64, 64, device=dev) * 2 - 1; xg = torch.rand(2, cfg.channel, 16, 64, 64, device=dev) * 2 - 1
        runner = trainer.StepRunner(cfg, models, trainer.build_optimizers(cfg, models), trainer.build_loss(cfg), sync_losses=False)
        for t in (1, 2):      # both parities of the update gating (surreal-depth1: the D phase's backward every second iteration), Adam state exists
            runner.step(xc, xg, t)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            runner.step(xc, xg, 3)
            runner.step(xc, xg, 4)
            torch.cuda.synchronize()
    finally:
        ops_cl.enable(False)
    from torch.autograd import DeviceType
    kernels = {e.key: e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    foreign = {k[:160]: n for k, n in kernels.items() if "at::" in k or "torch" in k.lower()}
    assert not foreign, foreign
    assert any("gan_loss" in k for k in kernels) and any("scale_dev" in k for k in kernels) and any(("cl_gather" if cl else "gather_gemm") in k for k in kernels), sorted(kernels)[:40]
