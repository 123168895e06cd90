"""What putting a checkpoint on the w8 grid (voicecraft_amd/quant.py) costs, measured with the fp32 oracle on the CPU: no GPU, no engine.
For tiny128 and tiny_h16, on the default synthetic weights and on the two trained-statistics settings (oracle/gen_golden.py STATS_A /
STATS_B with synth.trained_stats):
  rel_l2   worst and median per-step relative L2 of teacher-forced head logits, oracle(quantised) against oracle(original), on the
           original's 60-step greedy trajectory (muted terminator columns left out, as tests/test_gpu_model.py rel_l2 does)
  agree    share of those 60 steps at which all K arg-max tokens of the quantised model equal the original's (teacher-forced), and the
           number of leading steps a FREE-running greedy call of the quantised model stays on the original's trajectory
With --ffn-up every line also holds the THIRD matrix (quantize_state_dict_w8(..., ffn_up=True), what an engine created with `w8_up=True`
computes): "ffn_up" = the same figures for the three-matrix checkpoint against the original, and against the two-matrix checkpoint
(rel_l2_*_vs_two_matrices: what the third matrix adds), and the FFN up-projection's own weight movement.
No trained checkpoint exists on the machines this project is developed on: audible quality is unverified, the only gate is finiteness.
usage: python tools/w8_quality.py > profiles/w8_quality.log
       python tools/w8_quality.py --ffn-up > profiles/w8_up_quality.log"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from oracle.gen_golden import STATS_A, STATS_B
from oracle.voicecraft_oracle import VoiceCraftOracle
from voicecraft_amd import quant, synth

KNOBS = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=3)
STEPS = 60
FFN_UP = "--ffn-up" in sys.argv[1:]


def rel_l2(got, want):
    live = np.abs(want) < 1e3
    num = np.sqrt((((got - want) * live) ** 2).reshape(len(want), -1).sum(1))
    den = np.sqrt(((want * live) ** 2).reshape(len(want), -1).sum(1))
    return num / den


torch.set_num_threads(min(4, torch.get_num_threads()))
for preset in ("tiny128", "tiny_h16"):
    a = synth.make_args(preset)
    base = synth.make_state_dict(a, seed=3, head_gain=4.0)
    for name, sd in (("default", synth.make_state_dict(a, seed=0)), ("trained_stats_A", synth.trained_stats(base, a, **STATS_A)),
                     ("trained_stats_B", synth.trained_stats(base, a, **STATS_B))):
        sdq = quant.quantize_state_dict_w8(a, sd)
        x, xl, y = synth.random_prompt(a, 8, 20, seed=5)          # the length cap (10 frames per phoneme) ends the call after 60 steps
        tr = []
        VoiceCraftOracle(a, sd).inference_tts(x, xl, y, trace=tr, **KNOBS)
        want = torch.stack([t["logits"][0] for t in tr]).numpy()[:STEPS]
        toks = torch.stack([t["tokens"] for t in tr]).numpy()[:STEPS]
        orq = VoiceCraftOracle(a, sdq)
        got = orq.tts_logits_for_trajectory(x, y, toks, steps=list(range(len(toks)))).numpy().reshape(want.shape)
        assert np.isfinite(got).all()
        rel = rel_l2(got, want)
        agree = (got.argmax(-1) == want.argmax(-1)).all(axis=-1)
        trq = []
        orq.inference_tts(x, xl, y, trace=trq, **KNOBS)
        toksq = torch.stack([t["tokens"] for t in trq]).numpy()[:STEPS]
        n = min(len(toks), len(toksq))
        same = (toks[:n] == toksq[:n]).all(axis=-1)
        lead = int(n if same.all() else np.argmin(same))
        w = {m: float(((sdq[f"decoder.layers.0.{k}"] - sd[f"decoder.layers.0.{k}"]).norm() / sd[f"decoder.layers.0.{k}"].norm()))
             for m, (k, _) in quant.MATRICES.items()}
        line = {"preset": preset, "weights": name, "steps": int(len(toks)), "rel_l2_worst": round(float(rel.max()), 4),
                "rel_l2_median": round(float(np.median(rel)), 4), "teacher_forced_steps_agree": round(float(agree.mean()), 3),
                "free_running_leading_steps_equal": lead, "layer0_weight_rel_change": {m: round(v, 4) for m, v in w.items()}}
        if FFN_UP:
            sd3 = quant.quantize_state_dict_w8(a, sd, ffn_up=True)
            or3 = VoiceCraftOracle(a, sd3)
            got3 = or3.tts_logits_for_trajectory(x, y, toks, steps=list(range(len(toks)))).numpy().reshape(want.shape)
            assert np.isfinite(got3).all()
            rel3, rel32 = rel_l2(got3, want), rel_l2(got3, got)
            tr3 = []
            or3.inference_tts(x, xl, y, trace=tr3, **KNOBS)
            toks3 = torch.stack([t["tokens"] for t in tr3]).numpy()[:STEPS]
            n3 = min(len(toks), len(toks3))
            same3 = (toks[:n3] == toks3[:n3]).all(axis=-1)
            k1 = "decoder.layers.0." + quant.FFN_UP[0]
            line["ffn_up"] = {"rel_l2_worst": round(float(rel3.max()), 4), "rel_l2_median": round(float(np.median(rel3)), 4),
                              "rel_l2_worst_vs_two_matrices": round(float(rel32.max()), 4),
                              "rel_l2_median_vs_two_matrices": round(float(np.median(rel32)), 4),
                              "teacher_forced_steps_agree": round(float((got3.argmax(-1) == want.argmax(-1)).all(axis=-1).mean()), 3),
                              "teacher_forced_steps_agree_with_two_matrices": round(float((got3.argmax(-1) == got.argmax(-1)).all(axis=-1).mean()), 3),
                              "free_running_leading_steps_equal": int(n3 if same3.all() else np.argmin(same3)),
                              "layer0_weight_rel_change": round(float((sd3[k1] - sd[k1]).norm() / sd[k1].norm()), 4)}
        print(json.dumps(line), flush=True)
