"""CPU: the composed-iteration checker (oracle/stepcheck.py) applied to the REFERENCE's own arithmetic — the pinned fp32 torch-CPU
oracle plays the checked implementation.  Shows (a) the checker's bars are ones the reference's fp32 path itself meets, so they are a
statement about arithmetic, not about which fp32 lottery ticket a run drew, and (b) it fails when something is actually wrong (a wrong
learning rate, a skipped step).  Test widths (ngf = ndf = 6), 3 iterations, adversarial loss + Noise, and hinge with num_gen_update 2."""
import types

import pytest
import torch

from oracle import dcvgan_oracle as O
from oracle import stepcheck as SC
from tests import goldenio as G

pytestmark = pytest.mark.usefixtures("golden_cpu_threads")


class _Fp32Runner:
    """trainer.StepRunner's duck type over the fp32 StepOracle; `layers`-like tap for its branch patterns."""

    def __init__(self, cfg, states):
        self.so = O.StepOracle(cfg, states)
        self.KINK_TAP = self.ARGMAX_TAP = None
        self.models = {n: types.SimpleNamespace(state_dict=lambda n=n: self.so.st[n], training=True) for n in SC.MODELS}
        self.opts = {n: types.SimpleNamespace(params=O.trainable(self.so.st[n]), state=self.so.opt[n].state) for n in SC.MODELS}
        gen_mode = not getattr(cfg, "start_in_eval", False)
        self.models["ggen"].training = self.models["cgen"].training = gen_mode

    @property
    def iteration(self):
        return self.so.iteration

    wrong_argmax = None      # a test's stand-in for a faulty arg-max kernel: (softmax maps, own index) -> the index the colour generator reads

    def step(self, xc, xg, t):
        with O.KinkTape() as tape, O.ArgmaxTape(edit=self.wrong_argmax) as parts:
            out = self.so.step(xc, xg, t)
        if self.KINK_TAP is not None:
            self.KINK_TAP.extend(tape.recorded)
        if self.ARGMAX_TAP is not None:
            self.ARGMAX_TAP.extend(parts.recorded)
        self.models["ggen"].training = self.models["cgen"].training = True
        return out


def _setup(fixture):
    fx = G.load(fixture)
    cfg = G.cfg_of(fx, loss=str(fx["meta/loss"]), num_gen_update=int(fx["meta/num_gen_update"]), num_dis_update=int(fx["meta/num_dis_update"]),
                   start_in_eval=bool(fx["meta/start_in_eval"]))
    xc, xg = G.real_clips(cfg.batchsize, cfg.channel, fx["meta/seed_data"])
    return fx, cfg, xc, xg


@pytest.mark.parametrize("fixture", ["step_depth_adv_g1.npz", "step_depth_adv_g1_evalstart.npz", "step_flow_hinge_g2.npz", "step_segm_adv_g2.npz"])
def test_reference_arithmetic_meets_the_step_bars(fixture):
    fx, cfg, xc, xg = _setup(fixture)
    torch.manual_seed(int(fx["meta/seed_run"]))
    run = _Fp32Runner(cfg, G.states(fx))
    forced = SC.ForcedStepOracle(cfg, run.so.rng.log)       # the log grows as the fp32 run draws; the replay reads behind it
    for it in range(int(fx["meta/iters"])):
        res = SC.checked_iteration(run, run.models, run.opts, forced, run, xc, xg, xc, xg, int(fx["meta/t_rands"][it]), cfg.lr)
        assert [res["losses"][k] for k in ("loss_idis", "loss_vdis", "loss_gdis", "loss_gen")] == pytest.approx(list(fx["losses"][it]), rel=1e-6)  # it IS the reference's run
        SC.assert_iteration(res, cfg.lr, f"{fixture} it {it + 1}")
    assert forced.rng.pos == len(run.so.rng.log)


def test_checker_catches_a_wrong_learning_rate_and_a_skipped_step():
    fx, cfg, xc, xg = _setup("step_depth_adv_g1.npz")
    torch.manual_seed(int(fx["meta/seed_run"]))
    run = _Fp32Runner(cfg, G.states(fx))
    for g in run.so.opt["cgen"].param_groups:
        g["lr"] *= 1.01                                      # 1 % off: far inside the old 5 % norm / cos > 0.9 bars
    forced = SC.ForcedStepOracle(cfg, run.so.rng.log)
    res = SC.checked_iteration(run, run.models, run.opts, forced, run, xc, xg, xc, xg, 3, cfg.lr)
    with pytest.raises(AssertionError):
        SC.assert_iteration(res, cfg.lr)
    bad = [r for r in res["rows"] if r["rel_l2"] > SC.UPDATE_TOL]
    assert bad and all(r["model"] == "cgen" for r in bad)
    # the double ggen step taken once
    torch.manual_seed(int(fx["meta/seed_run"]))
    run = _Fp32Runner(cfg, G.states(fx))
    inner, n = run.so.opt["ggen"].step, [0]

    def once():
        n[0] += 1
        if n[0] == 1:
            inner()
    run.so.opt["ggen"].step = once
    forced = SC.ForcedStepOracle(cfg, run.so.rng.log)
    res = SC.checked_iteration(run, run.models, run.opts, forced, run, xc, xg, xc, xg, 3, cfg.lr)
    with pytest.raises(AssertionError):
        SC.assert_iteration(res, cfg.lr)


# --------------------------------------------------------------------------- #
# the segmentation configuration: a third lottery, the arg-max in front of the colour generator (oracle.ArgmaxTape)
# --------------------------------------------------------------------------- #
def _segm_run(**runner_attrs):
    from tests import segmstep as S
    cfg = S.config()
    xc, xg = S.calibration_clips()
    _, st = S.initial_states(cfg)
    torch.manual_seed(S.SEED_RUN)
    run = _Fp32Runner(cfg, st)
    for k, v in runner_attrs.items():
        setattr(run, k, v)
    return S, cfg, xc, xg, run, SC.ForcedStepOracle(cfg, run.so.rng.log)


def test_reference_arithmetic_meets_the_step_bars_on_the_segmentation_config():
    """`CONFIGS["surreal-segm"]` at width / 8, B = 2, four iterations of the reference's own fp32 arithmetic.  Without the arg-max tape iteration 3
    fails (buffers 2.8e-4, update 1.8e-2 on cgen/down_blocks.5.main.0.weight, 656 kinks up to 0.44 rms from zero): ONE pixel of 131 072 whose two
    largest softmax values differ by 2.0e-9 in fp64 takes the other part in fp32.  With the fp64 side told which part the checked run chose, every
    bar holds unchanged (iteration 3: loss 9.4e-8, buffers 2.1e-7, worst update 6.0e-6) and the flip is REPORTED: one mismatch (the G phase's pass of iteration 3), inside
    both conditions of assert_iteration; the seven other passes have none (profiles/stepcheck_segm.txt).  Which pixels fp32 flips depends on the
    host's summation order, so the test asserts the conditions, not that count."""
    S, cfg, xc, xg, run, forced = _segm_run()
    for it, t in enumerate(S.T_RANDS):
        res = SC.checked_iteration(run, run.models, run.opts, forced, run, xc, xg, xc, xg, t, cfg.lr)
        print("\n".join(SC.report_lines(res, it + 1)[:5]))
        SC.assert_iteration(res, cfg.lr, f"surreal-segm / 8 it {it + 1}")
        assert len(res["argmax"]) == 2 and all(p == S.B * 16 * 64 * 64 for _, p, _ in res["argmax"])       # the D phase's fakes and the G phase's
        assert all(r["calls"] == (0 if r["model"] in ("idis", "vdis", "gdis") and (it + 1) % 2 else 2 if r["model"] == "ggen" else 1) for r in res["rows"])
    assert forced.rng.pos == len(run.so.rng.log)


def _swap_64_to_the_runner_up(x, own):
    """A faulty arg-max: at the first 64 pixels whose two largest values are more than 1e-3 apart, the runner-up."""
    top = x.topk(2, dim=1)
    far = ((top.values[:, :1] - top.values[:, 1:]) > 1e-3).flatten().nonzero().flatten()[:64]
    assert far.numel() == 64
    out = own.clone()
    out.view(-1)[far] = top.indices[:, 1:].reshape(-1)[far]
    return out


def test_checker_catches_a_wrong_part_map():
    """The checked run reads (and reports) a map with 64 pixels on the runner-up part although the gap is > 1e-3: the fp64 side follows the map, so
    every other bar still holds — which also shows that the tape steers it — and the mismatches are reported and refused by the gap condition."""
    S, cfg, xc, xg, run, forced = _segm_run(wrong_argmax=_swap_64_to_the_runner_up)
    res = SC.checked_iteration(run, run.models, run.opts, forced, run, xc, xg, xc, xg, S.T_RANDS[0], cfg.lr)
    assert [n for n, _, _ in res["argmax"]] == [64, 64] and all(gap > 1e-3 for _, _, gap in res["argmax"]), res["argmax"]
    with pytest.raises(AssertionError):
        SC.assert_iteration(res, cfg.lr)
    SC.assert_iteration(dict(res, argmax=[]), cfg.lr, "all but the arg-max conditions")
    # 16 such pixels are inside the count condition: the gap condition alone refuses them
    with pytest.raises(AssertionError):
        SC.assert_iteration(dict(res, argmax=[(16, p, gap) for _, p, gap in res["argmax"]]), cfg.lr)
    SC.assert_iteration(dict(res, argmax=[(16, p, SC.ARGMAX_GAP) for _, p, _ in res["argmax"]]), cfg.lr)
    with pytest.raises(AssertionError):
        SC.assert_iteration(dict(res, argmax=[(17, p, 0.0) for _, p, _ in res["argmax"]]), cfg.lr)


def test_checker_still_catches_a_wrong_learning_rate_with_the_argmax_tape():
    S, cfg, xc, xg, run, forced = _segm_run()
    for g in run.so.opt["cgen"].param_groups:
        g["lr"] *= 1.01
    res = SC.checked_iteration(run, run.models, run.opts, forced, run, xc, xg, xc, xg, S.T_RANDS[0], cfg.lr)
    assert len(res["argmax"]) == 2
    with pytest.raises(AssertionError):
        SC.assert_iteration(res, cfg.lr)
    bad = [r for r in res["rows"] if r["rel_l2"] > SC.UPDATE_TOL]
    assert bad and all(r["model"] == "cgen" for r in bad)
