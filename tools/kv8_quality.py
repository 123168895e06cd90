"""What reading the K / V cache through the kv8 grid (voicecraft_amd/quant.py kv8_roundtrip) costs in logits, measured with the fp32
oracle on the CPU: no GPU, no engine.  The kv8 test oracle (tests/kv8_cases.py Kv8Oracle: past rows through the round trip of their
bf16 values, the step's own rows as they are) against the plain oracle, both on the cached path, teacher-forced on the plain oracle's
60-step greedy trajectory; tiny128 and tiny_h16, on the default synthetic weights and the two trained-statistics settings
(oracle/gen_golden.py STATS_A / STATS_B), as tools/w8_quality.py does for `w8`:
  rel_l2   worst and median per-step relative L2 of the head logits (muted terminator columns left out)
  agree    share of the steps at which all K arg-max tokens equal the plain oracle's
  bf16     the same two figures for a round trip that only rounds the past rows to bf16 (what the engine's bf16 cache does): the yardstick
  kv8c     the centred mode (kv8="centred", tests/kv8c_cases.py Kv8cOracle): K read as c + kv8c_roundtrip(k, c), c the prompt's mean K row
No trained checkpoint exists on the machines this project is developed on: audible quality is unverified.
usage: python tools/kv8_quality.py > profiles/kv8c_quality.log          (profiles/kv8_quality.log: the run before the kv8c column)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import kv8c_cases as cc          # quality_row: the setup, the three round trips and the figures (the CPU quality test asserts on the same)

torch.set_num_threads(min(4, torch.get_num_threads()))
for preset in ("tiny128", "tiny_h16"):
    for weights in ("default", "trained_stats_A", "trained_stats_B"):
        print(json.dumps(cc.quality_row(preset, weights)), flush=True)
