"""CPU: the gradient guard's surface — symbols in the header and the binding, the ABI version, argument validation on the host before any launch,
GradGuard's own argument checks, build_optimizers(guard=...), and no CPU fallback."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcv_grad_guard_workspace_bytes", "dcv_grad_guard_measure", "dcv_adam_step_multi_guarded")


@pytest.fixture(scope="module")
def lib():
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.lib()


def test_symbols_in_header_and_binding(lib):
    from dcvgan_amd import native
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dcvgan_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(native.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in native.EXPORTS and hasattr(raw, n), n
    assert lib.dcv_version() == native.ABI_VERSION == 4      # added symbols only
    # the state layout the header documents is the one optim.GradGuard indexes
    from dcvgan_amd import optim
    for i, f in enumerate(optim.GradGuard.FIELDS):
        assert re.search(r"#define DCV_GUARD_%s +%d\b" % (f.upper(), i), hdr), (f, i)
    assert re.search(r"#define DCV_GUARD_STATE_FLOATS %d\b" % len(optim.GradGuard.FIELDS), hdr)


def test_argument_validation_needs_no_gpu(lib):
    from dcvgan_amd.native import DCV_EINVAL, DCV_EWORKSPACE
    assert lib.dcv_grad_guard_workspace_bytes(-1, 1) == 0 and b"grad_guard" in lib.dcv_last_error()
    assert lib.dcv_grad_guard_workspace_bytes(1, -1) == 0
    # one double and one count per 4096-element block, at most one ragged block per tensor
    assert lib.dcv_grad_guard_workspace_bytes(0, 0) >= 12
    assert lib.dcv_grad_guard_workspace_bytes(4096 * 10 + 5, 3) >= 13 * 12
    fake = ctypes.create_string_buffer(256)      # never dereferenced: the checks come before any launch
    a = ctypes.addressof(fake)
    ptrs = (ctypes.c_void_p * 1)(a)
    numel = (ctypes.c_int64 * 1)(8)
    ok = dict(n=1, g=ptrs, numel=numel, grad_scale=1.0, max_norm=0.0, skip=1, dyn=0, growth=2.0, backoff=0.5, interval=2000, state=a, ws=a, ws_bytes=256)

    def measure(**kw):
        k = dict(ok, **kw)
        return lib.dcv_grad_guard_measure(k["n"], k["g"], k["numel"], k["grad_scale"], k["max_norm"], k["skip"], k["dyn"], k["growth"], k["backoff"], k["interval"],
                                          k["state"], k["ws"], k["ws_bytes"], None)
    assert measure(n=-1) == DCV_EINVAL
    assert measure(g=None) == DCV_EINVAL
    assert measure(numel=None) == DCV_EINVAL
    assert measure(state=None) == DCV_EINVAL
    assert measure(ws=None) == DCV_EINVAL
    assert measure(grad_scale=0.0) == DCV_EINVAL
    assert measure(numel=(ctypes.c_int64 * 1)(-4)) == DCV_EINVAL
    assert measure(g=(ctypes.c_void_p * 1)(None)) == DCV_EINVAL
    assert measure(dyn=1, interval=0) == DCV_EINVAL
    assert measure(numel=(ctypes.c_int64 * 1)(4096 * 100), ws_bytes=256) == DCV_EWORKSPACE
    p4 = (ctypes.c_void_p * 1)(a)

    def step(**kw):
        k = dict(n=1, p=p4, g=p4, m=p4, v=p4, numel=numel, block=a, state=a)
        k.update(kw)
        return lib.dcv_adam_step_multi_guarded(k["n"], k["p"], k["g"], k["m"], k["v"], k["numel"], 1e-3, 0.5, 0.999, 1e-8, 0.0, k["block"], k["state"], None)
    assert step(n=-1) == DCV_EINVAL
    assert step(p=None) == DCV_EINVAL
    assert step(block=None) == DCV_EINVAL
    assert step(state=None) == DCV_EINVAL
    assert step(m=(ctypes.c_void_p * 1)(None)) == DCV_EINVAL
    assert step(numel=(ctypes.c_int64 * 1)(-1)) == DCV_EINVAL
    assert lib.dcv_launch_count() == 0


def test_grad_guard_validates_its_arguments():
    from dcvgan_amd import optim
    g = optim.GradGuard()
    assert g.max_norm is None and g.skip_nonfinite and not g.dynamic and g.init_scale == 1.0 and g.growth_interval == 2000
    optim.GradGuard(max_norm=1.5, loss_scale=65536.0, dynamic=True, growth_interval=3)
    for bad in (dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=float("nan")), dict(max_norm=float("inf")), dict(loss_scale=0.0), dict(loss_scale=float("inf")),
                dict(growth_factor=1.0), dict(backoff_factor=1.0), dict(backoff_factor=0.0), dict(growth_interval=0), dict(growth_interval=2.5)):
        with pytest.raises(ValueError):
            optim.GradGuard(**bad)


def test_build_optimizers_accepts_guard():
    from dcvgan_amd import optim, trainer
    from dcvgan_amd.configs import CONFIGS
    cfg = CONFIGS["isogd-depth"].scaled(batchsize=2, width_div=8)
    models = trainer.build_models(cfg, torch.device("cpu"))
    opts = trainer.build_optimizers(cfg, models, guard=dict(max_norm=2.0, dynamic=True))
    gd, gg = opts["idis"].guard, opts["ggen"].guard
    assert isinstance(gd, optim.GradGuard) and isinstance(gg, optim.GradGuard) and gd is not gg
    assert opts["vdis"].guard is gd and opts["gdis"].guard is gd and opts["cgen"].guard is gg      # the buckets' grouping
    assert gd.max_norm == 2.0 and gd.dynamic and len(gd.optimizers) == 3 and len(gg.optimizers) == 2
    plain = trainer.build_optimizers(cfg, models)
    assert all(o.guard is None for o in plain.values())


def test_guarded_adam_has_no_cpu_fallback():
    from dcvgan_amd import native, optim
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    guard = optim.GradGuard(max_norm=1.0)
    o = optim.Adam([p], guard=guard)
    with pytest.raises(native.NativeError):
        o.step()              # no measurement yet — and none is possible on the host
    with pytest.raises(native.NativeError):
        guard.measure()
    with pytest.raises(native.NativeError):
        guard.root(None)
    assert torch.equal(p.detach(), torch.ones(4))
