"""CPU: the weight EMA's surface — the entry point in the header and the binding, argument validation on the host before any launch, no CPU fallback,
and the checkpoint layout of optim.ModelEma."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.lib()


def _models():
    from dcvgan_amd import trainer
    from dcvgan_amd.configs import CONFIGS
    cfg = CONFIGS["isogd-depth"].scaled(batchsize=2, width_div=8)
    torch.manual_seed(3)
    return cfg, trainer.build_models(cfg, torch.device("cpu"))


def test_entry_in_header_and_binding(lib):
    from dcvgan_amd import native
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dcvgan_hip.h")).read(), flags=re.S)
    assert re.search(r"\bdcv_ema_update_multi\s*\(", hdr)
    assert re.search(r"#define DCV_EMA_BLOCK_BYTES 64\b", hdr)
    assert "dcv_ema_update_multi" in native.EXPORTS and hasattr(ctypes.CDLL(native.LIB_PATH), "dcv_ema_update_multi")
    assert lib.dcv_version() == native.ABI_VERSION == 4      # an added symbol only


def test_argument_validation_needs_no_gpu(lib):
    from dcvgan_amd.native import DCV_EINVAL
    fake = ctypes.create_string_buffer(256)      # never dereferenced: the checks come before any launch
    a = ctypes.addressof(fake)
    one = lambda v: (ctypes.c_void_p * 1)(v)
    ok = dict(n=1, ema=one(a), src=one(a), numel=(ctypes.c_int64 * 1)(8), mode=(ctypes.c_int32 * 1)(0), decay=0.999, warmup=1, block=a, state=None)
    before = lib.dcv_launch_count()

    def update(**kw):
        k = dict(ok, **kw)
        return lib.dcv_ema_update_multi(k["n"], k["ema"], k["src"], k["numel"], k["mode"], k["decay"], k["warmup"], k["block"], k["state"], None)
    assert update(ema=None) == DCV_EINVAL and b"ema_update_multi" in lib.dcv_last_error()
    assert update(src=None) == DCV_EINVAL
    assert update(numel=None) == DCV_EINVAL
    assert update(mode=None) == DCV_EINVAL
    assert update(n=-1) == DCV_EINVAL
    assert update(ema=one(None)) == DCV_EINVAL
    assert update(src=one(None)) == DCV_EINVAL
    assert update(numel=(ctypes.c_int64 * 1)(-1)) == DCV_EINVAL
    assert update(mode=(ctypes.c_int32 * 1)(2)) == DCV_EINVAL
    assert update(mode=(ctypes.c_int32 * 1)(-1)) == DCV_EINVAL
    assert update(decay=1.0) == DCV_EINVAL
    assert update(decay=-0.1) == DCV_EINVAL
    assert update(decay=float("nan")) == DCV_EINVAL
    assert update(block=None) == DCV_EINVAL
    # a bad entry behind the first launch's 24 tensors is found before that launch too
    n = 30
    many = dict(n=n, ema=(ctypes.c_void_p * n)(*[a] * n), src=(ctypes.c_void_p * n)(*[a] * n), numel=(ctypes.c_int64 * n)(*[8] * n))
    assert update(mode=(ctypes.c_int32 * n)(*([0] * 29 + [2])), **many) == DCV_EINVAL
    assert lib.dcv_launch_count() == before


def test_model_ema_has_no_cpu_fallback():
    from dcvgan_amd import native, optim
    _, models = _models()
    ema = optim.ModelEma(models)
    before = {k: v.clone() for k, v in ema.module("ggen").state_dict().items()}
    with pytest.raises(native.NativeError):
        ema.update()
    assert all(torch.equal(v, before[k]) for k, v in ema.module("ggen").state_dict().items())
    for bad in (1.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            optim.ModelEma(models, decay=bad)


def test_twins_and_state_dict_layout():
    from dcvgan_amd import optim, trainer
    cfg, models = _models()
    models["ggen"]._rng = object()
    ema = optim.ModelEma(models, decay=0.99, warmup=False)
    sd = ema.state_dict()
    assert list(sd) == ["ggen", "cgen", "num_updates", "decay", "warmup"]
    assert sd["num_updates"] == 0 and sd["decay"] == 0.99 and sd["warmup"] is False
    for n in ("ggen", "cgen"):
        live, twin = models[n], ema.module(n)
        assert type(twin) is type(live) and not twin.training
        assert list(sd[n]) == list(live.state_dict())
        assert all(torch.equal(sd[n][k], v) and sd[n][k].dtype == v.dtype for k, v in live.state_dict().items())
        assert not any(p.requires_grad for p in twin.parameters())
        assert not {t.data_ptr() for t in twin.state_dict().values()} & {t.data_ptr() for t in live.state_dict().values()}
        assert twin._rng is not None and twin._rng is not live._rng
    # one stream for all twins (two PhiloxRng objects would hand both twins the same values): consecutive draws take consecutive offsets
    assert ema.module("ggen")._rng is ema.module("cgen")._rng is ema.rng
    assert ema.module("ggen")._rng._next()[1] + 1 == ema.module("cgen")._rng._next()[1]
    # a host-built ModelEma keeps a checkpoint's count
    ema.load_state_dict(dict(sd, num_updates=7))
    assert ema.num_updates() == 7 and ema.state_dict()["num_updates"] == 7
    ema.reset()
    assert ema.num_updates() == 0
    assert models["ggen"].training      # the live models are left as they were
    # build_ema wires the G phase's guard, through the data-parallel wrapper too
    opts = trainer.build_optimizers(cfg, models, guard=dict(max_norm=2.0))
    assert trainer.build_ema(cfg, models, opts).guard is opts["ggen"].guard is not None
    assert trainer.build_ema(cfg, models, trainer.build_optimizers(cfg, models)).guard is None
    wrapped = dict(opts, ggen=optim.DataParallelAdam(opts["ggen"]))
    assert trainer.build_ema(cfg, models, wrapped, decay=0.9, warmup=False).guard is opts["ggen"].guard
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg))
    assert runner.ema is None
