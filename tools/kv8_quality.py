"""What reading the K / V cache through the kv8 grid (voicecraft_amd/quant.py kv8_roundtrip) costs in logits, measured with the fp32
oracle on the CPU: no GPU, no engine.  The kv8 test oracle (tests/kv8_cases.py Kv8Oracle: past rows through the round trip of their
bf16 values, the step's own rows as they are) against the plain oracle, both on the cached path, teacher-forced on the plain oracle's
60-step greedy trajectory; tiny128 and tiny_h16, on the default synthetic weights and the two trained-statistics settings
(oracle/gen_golden.py STATS_A / STATS_B), as tools/w8_quality.py does for `w8`:
  rel_l2   worst and median per-step relative L2 of the head logits (muted terminator columns left out)
  agree    share of the steps at which all K arg-max tokens equal the plain oracle's
  bf16     the same two figures for a round trip that only rounds the past rows to bf16 (what the engine's bf16 cache does): the yardstick
No trained checkpoint exists on the machines this project is developed on: audible quality is unverified.
usage: python tools/kv8_quality.py > profiles/kv8_quality.log"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from oracle.gen_golden import STATS_A, STATS_B
from oracle.voicecraft_oracle import VoiceCraftOracle
from voicecraft_amd import synth
import kv8_cases as kc

KNOBS = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=3)
STEPS = 60


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
        prompt = synth.random_prompt(a, 8, 20, seed=5)          # the length cap (10 frames per phoneme) ends the call after 60 steps
        tr = []
        VoiceCraftOracle(a, sd).inference_tts(*prompt, trace=tr, **KNOBS)
        want = torch.stack([t["logits"][0] for t in tr]).numpy()[:STEPS]
        toks = torch.stack([t["tokens"] for t in tr]).numpy()
        row = {"preset": preset, "weights": name, "steps": int(len(want))}
        for tag, rt in (("kv8", None), ("bf16", lambda t: t.bfloat16().float())):
            got = kc.cached_tts_logits(kc.Kv8Oracle(a, sd, roundtrip=rt), prompt, toks)[:STEPS]
            assert got.shape == want.shape and np.isfinite(got).all()
            rel = rel_l2(got[1:], want[1:])                     # (step 0 reads no cache)
            agree = (got.argmax(-1) == want.argmax(-1)).all(axis=-1)
            row[tag] = {"rel_l2_worst": round(float(rel.max()), 4), "rel_l2_median": round(float(np.median(rel)), 4),
                        "teacher_forced_steps_agree": round(float(agree.mean()), 3)}
        print(json.dumps(row), flush=True)
