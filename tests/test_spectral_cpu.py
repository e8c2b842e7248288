"""CPU: the surface of spectral normalisation — the entry points in the header and the binding, argument validation before any launch, the marks and
buffers of optim.spectral_norm, the checkpoint keys, the refusals, and deep copies."""
import copy
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dcv_spectral_workspace_bytes", "dcv_spectral_update_multi", "dcv_spectral_project_multi")


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


def test_entries_in_header_and_binding(lib):
    from dcvgan_amd import native
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dcvgan_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(native.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in native.EXPORTS and hasattr(raw, n), n
    # the binding's argument counts are the header's
    for n in NAMES:
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, hdr, flags=re.S).group(1)
        assert len(decl.split(",")) == len(native._SIGS[n][1]), n
    assert lib.dcv_version() == native.ABI_VERSION == 4      # added symbols only


def test_argument_validation_needs_no_gpu(lib):
    from dcvgan_amd.native import DCV_EINVAL, DCV_EWORKSPACE
    fake = ctypes.create_string_buffer(4096)      # never dereferenced: the checks come before any launch
    a = ctypes.addressof(fake) // 16 * 16 + 16
    one = lambda v: (ctypes.c_void_p * 1)(v)
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    before = lib.dcv_launch_count()
    assert lib.dcv_spectral_workspace_bytes(1, i32(4), i32(16)) >= 256
    assert lib.dcv_spectral_workspace_bytes(1, i32(0), i32(16)) == 0 and b"spectral_workspace_bytes" in lib.dcv_last_error()
    assert lib.dcv_spectral_workspace_bytes(1, i32(4), None) == 0
    assert lib.dcv_spectral_workspace_bytes(1, i32(1 << 20), i32(1 << 11)) == 0      # rows * cols > 2^30
    ok = dict(n=1, w=one(a), w_sn=one(a + 256), u=one(a + 512), v=one(a + 768), sigma=one(a + 1024), rows=i32(4), cols=i32(16), n_iter=1, eps=1e-12, ws=a + 2048,
              ws_bytes=1 << 20)

    def update(**kw):
        k = dict(ok, **kw)
        return lib.dcv_spectral_update_multi(k["n"], k["w"], k["w_sn"], k["u"], k["v"], k["sigma"], k["rows"], k["cols"], k["n_iter"], k["eps"], None, k["ws"],
                                             k["ws_bytes"], None)

    def project(**kw):
        k = dict(ok, **kw)
        return lib.dcv_spectral_project_multi(k["n"], k["w"], k["w_sn"], k["u"], k["v"], k["sigma"], k["rows"], k["cols"], k["eps"], k["ws"], k["ws_bytes"], None)
    for call in (update, project):
        assert call(n=-1) == DCV_EINVAL and b"spectral_" in lib.dcv_last_error()
        for name in ("w", "w_sn", "u", "v", "sigma"):
            assert call(**{name: None}) == DCV_EINVAL, name
            assert call(**{name: one(None)}) == DCV_EINVAL, name
        assert call(rows=None) == DCV_EINVAL and call(cols=i32(0)) == DCV_EINVAL and call(rows=i32(-3)) == DCV_EINVAL
        assert call(eps=0.0) == DCV_EINVAL and call(eps=float("nan")) == DCV_EINVAL
        assert call(ws=None) == DCV_EINVAL and call(ws=a + 2052) == DCV_EINVAL      # a workspace off the 16-byte grid
        assert call(w_sn=one(a)) == DCV_EINVAL                                      # the output (update) / the gradient (project) aliases its operand
        assert call(ws_bytes=64) == DCV_EWORKSPACE
    assert update(n_iter=-1) == DCV_EINVAL
    assert lib.dcv_launch_count() == before


def test_marks_buffers_and_checkpoint_keys():
    from dcvgan_amd import optim, trainer
    cfg, models = _models()
    plain = {n: list(m.state_dict()) for n, m in models.items()}
    opts = trainer.build_optimizers(cfg, models, guard={})
    sn = trainer.build_spectral_norm(cfg, models, opts, seed=5)
    assert sn.guard is opts["idis"].guard is not None and sn.guard is not opts["ggen"].guard
    convs = [c for n in ("idis", "vdis", "gdis") for c in models[n].modules() if isinstance(c, (torch.nn.Conv2d, torch.nn.Conv3d))]
    assert len(convs) == 14 and [id(c) for c in sn.convs] == [id(c) for c in convs]
    for c in convs:
        assert optim.is_spectral(c) and "_dcv_spectral" in c.__dict__ and "_dcv_spectral" not in c._modules and "_dcv_spectral" not in c._buffers
        assert isinstance(c.weight, torch.nn.Parameter) and c.weight.is_leaf and c.weight.requires_grad      # the Parameter stays the raw weight
        assert [k for k, _ in c.named_buffers()] == ["weight_u", "weight_v", "weight_sigma"]
        assert c.weight_u.shape == (c.weight.shape[0],) and c.weight_v.shape == (c.weight[0].numel(),) and c.weight_sigma.shape == (1,)
        assert abs(float(c.weight_u.double().norm()) - 1.0) < 1e-6 and abs(float(c.weight_v.double().norm()) - 1.0) < 1e-6
        assert c.__dict__["_dcv_spectral"].w_sn.shape == c.weight.shape
    for n in ("ggen", "cgen"):      # the generators are untouched
        assert list(models[n].state_dict()) == plain[n]
        assert not any(optim.is_spectral(c) for c in models[n].modules())
    for n in ("idis", "vdis", "gdis"):
        keys = list(models[n].state_dict())
        added = [k for k in keys if k not in plain[n]]
        assert [k for k in keys if k in plain[n]] == plain[n]
        want = sorted(f"{name}.{b}" for name, c in models[n].named_modules() if isinstance(c, (torch.nn.Conv2d, torch.nn.Conv3d)) for b in ("weight_u", "weight_v", "weight_sigma"))
        assert sorted(added) == want and len(want) > 0
    # the same seed gives the same start, another seed another
    _, again = _models()
    sn2 = optim.spectral_norm(again, seed=5)
    assert all(torch.equal(a.weight_u, b.weight_u) and torch.equal(a.weight_v, b.weight_v) for a, b in zip(sn.convs, sn2.convs))
    _, third = _models()
    assert not torch.equal(optim.spectral_norm(third, seed=6).convs[0].weight_u, sn.convs[0].weight_u)
    sd = sn.state_dict()
    assert list(sd) == ["eps", "u", "v", "sigma"] and len(sd["u"]) == 14 and sd["eps"] == 1e-12
    sn2.load_state_dict(sd)
    assert all(c.__dict__["_dcv_spectral"].version is None for c in sn2.convs)      # stale until refresh()
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg))
    assert runner.spectral is None
    assert trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), spectral=sn).spectral is sn
    wrapped = dict(opts, idis=optim.DataParallelAdam(opts["idis"]))
    _, fourth = _models()
    assert trainer.build_spectral_norm(cfg, fourth, wrapped)._dp == [wrapped["idis"]]


def test_no_cpu_fallback_and_refusals():
    from dcvgan_amd import layers, native, optim
    _, models = _models()
    with pytest.raises(native.NativeError, match="ConvTranspose"):
        optim.spectral_norm(models, names=("cgen",))
    assert not any(optim.is_spectral(c) for c in models["cgen"].modules())      # refused before the first mark
    with pytest.raises(native.NativeError, match="ConvTranspose"):
        optim.spectral_norm(torch.nn.Sequential(torch.nn.Conv2d(1, 2, 3, bias=False), torch.nn.ConvTranspose2d(2, 1, 3, bias=False)))
    with pytest.raises(ValueError):
        optim.spectral_norm(torch.nn.Sequential(torch.nn.ReLU()))
    with pytest.raises(ValueError):
        optim.spectral_norm(models, eps=0.0)
    sn = optim.spectral_norm(models, names=("idis",))
    with pytest.raises(native.NativeError, match="already marked"):
        optim.spectral_norm(models, names=("idis",))
    for call in (sn.update, sn.refresh, sn.project):
        before = [c.weight_u.clone() for c in sn.convs]
        for c in sn.convs:
            c.weight.grad = torch.zeros_like(c.weight)
        with pytest.raises(native.NativeError):
            call()
        assert all(torch.equal(a, c.weight_u) for a, c in zip(before, sn.convs))
    # a marked convolution whose W / sigma was never formed refuses to run (here: host models; on the device: a stale version)
    with pytest.raises(native.NativeError, match=r"update\(\).*refresh\(\)"):
        layers._w_eff(sn.convs[0], torch.zeros(2, 1, 64, 64))
    assert layers._w_eff(models["vdis"].main[1], torch.zeros(1)) is None      # unmarked: nothing
    sn.remove()
    assert not any(optim.is_spectral(c) for c in models["idis"].modules()) and not any("weight_u" in k for k in models["idis"].state_dict())


def test_a_deep_copy_carries_the_buffers_but_no_mark():
    from dcvgan_amd import optim
    _, models = _models()
    sn = optim.spectral_norm(models, names=("vdis",))
    twin = copy.deepcopy(models["vdis"])
    assert list(twin.state_dict()) == list(models["vdis"].state_dict())
    convs = [c for c in twin.modules() if isinstance(c, torch.nn.Conv3d)]
    assert len(convs) == len(sn.convs) == 5
    for c, live in zip(convs, sn.convs):
        assert not optim.is_spectral(c) and optim.is_spectral(live)
        assert torch.equal(c.weight_u, live.weight_u) and c.weight_u.data_ptr() != live.weight_u.data_ptr()
