"""Calibration of oracle/stepcheck.py: the REFERENCE's own arithmetic (the pinned fp32 torch-CPU oracle) as the checked implementation
against the teacher-forced fp64 oracle with its own activation pattern (and, for the segmentation head, its own part maps: oracle.ArgmaxTape).
Shows what any fp32 implementation scores under the bars the HIP path is held to.  CPU only:
    python3 tools/stepcheck_reference.py step_fullwidth_isogd_depth.npz step_fullwidth_surreal_depth1.npz step_fullwidth_isogd_flow.npz
        (full width: profiles/r03_step_parity/reference_fp32_cpu.txt)
    python3 tools/stepcheck_reference.py step_segm_adv_g2.npz segm segm --no-argmax-tape
        (profiles/stepcheck_segm.txt: the width-4 fixture, then `segm` = CONFIGS["surreal-segm"] at width / 8, B = 2, the four iterations of
        tests/segmstep.py; every name after --no-argmax-tape runs with the fp64 side left to its own arg-max, which is the lottery the tape removes)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tests.test_stepcheck_cpu import _Fp32Runner
from tests import fullwidth as FW, goldenio as G, segmstep as S
from oracle import stepcheck as SC
torch.set_num_threads(8)
taped = True
for fixture in sys.argv[1:]:
    if fixture == "--no-argmax-tape":
        taped = False
        continue
    if fixture == "segm":
        cfg = S.config()
        states = S.initial_states(cfg)[1]
        xc, xg = S.calibration_clips()
        seed_run, t_rands = S.SEED_RUN, S.T_RANDS
    else:
        fx = G.load(fixture)
        if "init/ggen/main.0.weight" in fx:     # a test-width fixture that carries its initial states
            cfg = G.cfg_of(fx, loss=str(fx["meta/loss"]), num_gen_update=int(fx["meta/num_gen_update"]), num_dis_update=int(fx["meta/num_dis_update"]),
                           start_in_eval=bool(fx["meta/start_in_eval"]))
            states = G.states(fx)
        else:
            cfg, models = FW.same_seed_models(fx)
            cfg.num_gen_update = int(fx["meta/num_gen_update"]); cfg.lr = {m: float(fx[f"meta/lr/{m}"]) for m in G.MODELS}
            states = FW.states_of(models)
        xc, xg = G.real_clips(cfg.batchsize, cfg.channel, fx["meta/seed_data"])
        seed_run, t_rands = int(fx["meta/seed_run"]), [int(t) for t in fx["meta/t_rands"]][:int(fx["meta/iters"])]
    torch.manual_seed(seed_run)
    run = _Fp32Runner(cfg, states)
    forced = SC.ForcedStepOracle(cfg, run.so.rng.log, argmax_tape=taped)
    for it, t in enumerate(t_rands):
        res = SC.checked_iteration(run, run.models, run.opts, forced, run, xc, xg, xc, xg, t, cfg.lr)
        rows = res["rows"]
        try:
            SC.assert_iteration(res, cfg.lr)
            verdict = "passes every bar"
        except AssertionError as e:
            verdict = "FAILS: " + str(e)[:160]
        print(fixture + ("" if taped else " (no arg-max tape)"), it+1, "loss_rel %.2e buf %.2e" % (res["loss_rel"], res["buffers_rel"]), "rel_l2", SC.worst(rows, "rel_l2"),
              "sens", sum(r["n_sensitive"] for r in rows), "off", sum(r["n_sensitive_off"] for r in rows), "kinks", res["kink_flips"], res["kink_total"], res["kink_worst_call"],
              "argmax", res["argmax"], verdict, flush=True)
