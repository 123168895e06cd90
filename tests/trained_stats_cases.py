"""The checkpoints, prompts and oracle runs shared by tests/test_trained_stats_cpu.py (conditions on the inputs, checked on the
oracle alone) and tests/test_gpu_trained_stats.py (the engine against the oracle in the value regime of a trained checkpoint).

Everything is regenerated from seeds: `synth.make_state_dict` (frozen stream) + `synth.trained_stats` in one of the two settings of
oracle/gen_golden.py (STATS_A: large common offset that drifts, peaked attention, raw scores past the range of fp32 exp; STATS_B: a
few massive-activation channels).  `head_gain = 4` keeps every step's arg-max margin far above the fp32 oracle's own rounding."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle.gen_golden import STATS_A, STATS_B
from oracle.voicecraft_oracle import VoiceCraftOracle
from voicecraft_amd import synth

LAYERS = {"tiny": 4, "tiny_h16": 3, "tiny128": 3}
WSEED = 3
KNOBS = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=3)


def stats_kw(setting: str, **over) -> dict:
    kw = dict(STATS_A if setting == "A" else STATS_B)
    kw.update(over)
    return kw


def stats_key(setting: str, bf16: bool = False, **over):
    """Setting A runs with k_bias 40 in fp32 and 8 in bf16 (a shift of every score of a query by q . b costs bf16 K rows their mantissa)."""
    if setting == "A" and bf16:
        over.setdefault("k_bias", 8.0)
    return setting, tuple(sorted(over.items()))


@functools.lru_cache(maxsize=None)
def checkpoint(preset: str, key):
    """(args, state_dict, fp32 oracle) of a preset in a setting (`key` = stats_key(...))."""
    setting, over = key
    a = synth.make_args(preset, num_decoder_layers=LAYERS[preset])
    sd = synth.trained_stats(synth.make_state_dict(a, seed=WSEED, head_gain=4.0), a, **stats_kw(setting, **dict(over)))
    torch.set_num_threads(min(4, torch.get_num_threads()))      # tiny models: more threads only hand work back and forth
    return a, sd, VoiceCraftOracle(a, sd)


def prompt(a, u: int, seed: int):
    """Sequence u of the ragged family: Lx 4..6 phonemes, a prompt of 30..52 frames, 9..24 generated frames before the reference's
    length cap (10 frames per phoneme) ends it.  u = -1: the prompt shape of golden tts_stats_greedy."""
    if u < 0:
        return synth.random_prompt(a, 6, 40, seed=seed)
    Lx = 4 + u % 3
    g = 5 + 3 * (u % 6) + (u // 18)
    return synth.random_prompt(a, Lx, 10 * Lx - g, seed=seed)


def _trace(tr):
    return torch.stack([t["logits"][0] for t in tr]).numpy(), torch.stack([t["tokens"] for t in tr]).numpy()


def tts_run_seeded(preset: str, key, p):
    a, sd, orc = checkpoint(preset, key)
    tr = []
    res = orc.inference_tts(*p, trace=tr, **KNOBS)[0].numpy()
    return (p, res) + _trace(tr)


@functools.lru_cache(maxsize=None)
def tts_run(preset: str, key, u: int):
    """The oracle's greedy run of sequence u: (prompt, res [1,K,T'], logits [steps,K,V], tokens [steps,K])."""
    a = checkpoint(preset, key)[0]
    return tts_run_seeded(preset, key, prompt(a, u, PROMPT_SEEDS[(preset, key[0])][u + 1]))


def long_prompt(a, seed: int):
    """20 phonemes + 190 frames: a 211-row prefill pass (thirteen full 16-row tiles and a ragged one), then 14 decode steps."""
    return synth.random_prompt(a, 20, 190, seed=seed)


@functools.lru_cache(maxsize=None)
def long_run(preset: str, key):
    a = checkpoint(preset, key)[0]
    return tts_run_seeded(preset, key, long_prompt(a, LONG_SEEDS[(preset, key[0])]))


EDIT_SPANS = [(10, 18), (40, 47)]


def edit_prompt(a, seed: int):
    return synth.random_prompt(a, 9, 64, seed=seed)          # the prompt shape of golden edit_stats_2span


def edit_run_seeded(preset: str, key, p):
    a, sd, orc = checkpoint(preset, key)
    mi = torch.tensor([EDIT_SPANS], dtype=torch.int64)
    tr = []
    res = orc.inference(*p, mi, top_k=1, stop_repetition=-1, trace=tr).numpy()
    return (p, mi, res) + _trace(tr)


@functools.lru_cache(maxsize=None)
def edit_run(preset: str, key):
    a = checkpoint(preset, key)[0]
    return edit_run_seeded(preset, key, edit_prompt(a, EDIT_SEEDS[(preset, key[0])]))


# ---- what the GPU file runs in fp32 (free-running: the engine's tokens must equal the oracle's), by (preset, setting):
# one row (u = -1 and u = 0), 3 / 8 / 12 sequences on finished rows, 20 / 40 on the wide form, a two-span edit, a 215-row prefill
FP32_MODELS = [("tiny", "A"), ("tiny", "B"), ("tiny_h16", "A"), ("tiny_h16", "B")]
FP32_WIDE = [("tiny", "A", 20), ("tiny", "A", 40)]
FP32_EDIT = [("tiny", "A"), ("tiny128", "B"), ("tiny_h16", "A")]
FP32_LONG = [("tiny", "A"), ("tiny_h16", "B")]

# Prompt seeds, picked (first of base, base + 1000, ...) so that the fp32 oracle decides every greedy token of the run with room to
# spare: top-1 margin >= 100 x its own fp32-vs-float64 difference at every step (tests/test_trained_stats_cpu.py holds them to it).
# Entry u + 1 of a list is sequence u; entry 0 the one-row prompt (the golden cases tts_stats_greedy / edit_stats_2span use the
# ("tiny", "A") one-row seed and the ("tiny128", "B") editing seed).  bf16 runs are teacher-forced and reuse them.
PROMPT_SEEDS = {
    ("tiny", "A"): [14005, 4500, 2501, 2502, 7503, 2504, 20505, 2506, 1507, 508, 7509, 15510, 53511, 512, 6513, 7514, 3515, 13516, 517,
                    518, 22519, 2520, 11521, 36522, 12523, 2524, 4525, 4526, 3527, 23528, 15529, 530, 531, 2532, 14533, 16534, 21535,
                    536, 12537, 8538, 6539],
    ("tiny", "B"): [5, 500, 501, 502, 503, 504, 505, 506, 507, 508, 1509, 510, 511],
    ("tiny_h16", "A"): [11005, 4500, 3501, 6502, 6503, 2504, 13505, 506, 4507, 7508, 31509, 5510, 4511],
    ("tiny_h16", "B"): [5, 500, 501, 502, 503, 1504, 505, 506, 507, 508, 509, 1510, 511],
    ("tiny128", "A"): [5 + u + 495 * (u > 0) for u in range(41)],      # bf16 only
    ("tiny128", "B"): [5 + u + 495 * (u > 0) for u in range(41)],      # bf16 only
}
for _k in (("tiny_h16", "A"), ("tiny_h16", "B")):                       # sequences 12.. run in bf16 only
    PROMPT_SEEDS[_k] = PROMPT_SEEDS[_k] + [500 + u for u in range(12, 40)]
LONG_SEEDS = {("tiny", "A"): 2077, ("tiny_h16", "B"): 77, ("tiny128", "A"): 77, ("tiny128", "B"): 77}
EDIT_SEEDS = {("tiny", "A"): 7017, ("tiny128", "B"): 1017, ("tiny_h16", "A"): 39017}


def fp32_runs():
    """Every oracle run a fp32 GPU test compares tokens with: (id, logits [steps,K,V], one-pass evaluator taking an oracle)."""
    def tts_eval(preset, key, p, toks):
        return lambda orc: orc.tts_logits_for_trajectory(p[0], p[2], toks, steps=list(range(len(toks)))).numpy()
    for preset, s in FP32_MODELS:
        key = stats_key(s)
        n = max([12] + [B for (pp, ss, B) in FP32_WIDE if (pp, ss) == (preset, s)])
        for u in range(-1, n):
            p, res, lg, toks = tts_run(preset, key, u)
            yield f"{preset}-{s}-u{u}", preset, key, lg, tts_eval(preset, key, p, toks)
    for preset, s in FP32_LONG:
        key = stats_key(s)
        p, res, lg, toks = long_run(preset, key)
        yield f"{preset}-{s}-long", preset, key, lg, tts_eval(preset, key, p, toks)
    for preset, s in FP32_EDIT:
        key = stats_key(s)
        yield f"{preset}-{s}-edit", preset, key, edit_run(preset, key)[3], None      # (two spans: no one-pass form; the float64 loop is run)
