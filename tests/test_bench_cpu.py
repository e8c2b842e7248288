"""CPU: bench.py's --dump-outputs writer (bench.dump_outputs) on CPU-built models — file names and types, the 64 MB cap at full width,
the whole state when it fits, and the same sample positions from call to call."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench)


def _models(name, **kw):
    from dcvgan_amd import trainer
    from dcvgan_amd.configs import CONFIGS
    cfg = CONFIGS[name].scaled(**kw) if kw else CONFIGS[name]
    torch.manual_seed(cfg.seed)
    return trainer.build_models(cfg, torch.device("cpu"))


def _flat(m):
    return torch.cat([t.detach().reshape(-1).float() for t in m.state_dict().values() if t.is_floating_point()]).numpy()


LOSSES = {"loss_idis": torch.tensor(1.25), "loss_vdis": torch.tensor(1.5), "loss_gdis": torch.tensor(0.75), "loss_gen": torch.tensor(2.0)}


def test_dump_holds_the_whole_state_when_it_fits(tmp_path):
    models = _models("isogd-depth", width_div=8)
    bench.dump_outputs(str(tmp_path), LOSSES, models)
    assert sorted(os.listdir(tmp_path)) == sorted([f"{k}.npy" for k in LOSSES] + [f"state_{n}.npy" for n in models])
    for k, v in LOSSES.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == np.float64 and got.shape == (1,) and got[0] == float(v)
    for n, m in models.items():
        got = np.load(tmp_path / f"state_{n}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, _flat(m)), n


def test_full_width_dump_is_capped_and_repeatable(tmp_path):
    models = _models("surreal-depth1")          # the largest state of the three configs: 86 MB of float32
    total = sum(_flat(m).size for m in models.values())
    assert total > bench.DUMP_STATE_ELEMENTS
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), LOSSES, models)
    bench.dump_outputs(str(b), LOSSES, models)
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 64 * 10**6
    for n, m in models.items():
        got, want = np.load(a / f"state_{n}.npy"), _flat(m)
        assert got.dtype == np.float32 and abs(got.size / want.size - bench.DUMP_STATE_ELEMENTS / total) < 0.01, n
        assert np.isin(got, want).all() and np.array_equal(got, np.load(b / f"state_{n}.npy")), n
