"""Option `kv8` against the same build's engine without it: THREE engines in one process on the same weights (giga830M, bf16, synthetic
checkpoint) - off, kv8=True ("on") and kv8="centred" - interleaved (same process, same clocks, alternating legs, the spread next to every
delta).  Every line compares on with off; the lines "centred vs off" and "centred vs on" follow it (the second is the one that says what
centring costs).
  kernels  vc_bench_kernel "attn" (1, 8 rows: 884 cached positions of one sequence), "wd_attn" (32, 64 rows: 884 positions of as many
           sequences) and "step" (1, 8 rows: the whole step without the sampler, the packer launch inside it on the kv8 engine)
  calls    whole inference_tts_multi calls of 8, 32 and 64 utterances (300 phonemes, 535 prompt frames, 48 forced steps: contexts of 836 .. 884
           positions, and both engines run the same steps): the decode loop's device time and the prefill's (vc_last_timing)
JSON lines on stdout.  usage: python tools/kv8_ab.py [reps = 7] [pairs = 5] [--kernels-only]        (profiles/kv8_ab.log, kv8c_ab.log)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from voicecraft_amd import synth
from voicecraft_amd.engine import VoiceCraftEngine

args = [v for v in sys.argv[1:] if not v.startswith("--")]
reps = int(args[0]) if args else 7
pairs = int(args[1]) if len(args) > 1 else 5
a = synth.make_args("giga830M")
sd = synth.make_state_dict(a, seed=0, perturb=False, mute_eos=True, fast=True)
engs = {}
for tag, kv8 in (("off", False), ("on", True), ("centred", "centred")):
    torch.cuda.synchronize()
    m0 = torch.cuda.mem_get_info()[0]
    engs[tag] = VoiceCraftEngine(a, sd, device="cuda:0", dtype="bf16", max_seqs=64, max_positions=1024, kv8=kv8)
    torch.cuda.synchronize()
    print(json.dumps({"engine": tag, "options": engs[tag].options(), "resident_GB": round((m0 - torch.cuda.mem_get_info()[0]) / 2 ** 30, 3)}), flush=True)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3)}


def report(what, rows, t, unit):
    for base, new in (("off", "on"), ("off", "centred"), ("on", "centred")):
        off, on = t[base], t[new]
        d = 100.0 * (np.asarray(on) / np.asarray(off) - 1.0)      # paired: leg i of `new` ran in the same round as leg i of `base`
        print(json.dumps({"what": what if new == "on" else f"{what}: {new} vs {base}", "rows": rows, "unit": unit, base: spread(off), new: spread(on),
                          "delta_pct": {"median": round(float(np.median(d)), 2), "min": round(float(d.min()), 2), "max": round(float(d.max()), 2)},
                          "faster_beyond_spread": bool(d.max() < 0), "slower_beyond_spread": bool(d.min() > 0)}), flush=True)


for which, rows_list in (("attn", (1, 8)), ("wd_attn", (32, 64)), ("step", (1, 8))):
    for rows in rows_list:
        t = {tag: [] for tag in engs}
        for e in engs.values():
            e.bench_kernel(which, n_rows=rows, iters=8)
        for r in range(reps):
            for tag, e in engs.items():
                t[tag].append(e.bench_kernel(which, n_rows=rows, iters=32 if which == "step" else 64)[0] * 1e3)
        report(which, rows, t, "us per launch")
if "--kernels-only" in sys.argv:
    sys.exit(0)
K, n = a.n_codebooks, 48
for B in (8, 32, 64):
    pr = [synth.random_prompt(a, 300, 535, seed=1 + u) for u in range(B)]
    forced = np.random.RandomState(B).randint(0, a.audio_vocab_size, size=(n, B, K)).astype(np.int64)
    for j in range(K):
        forced[n - K + j, :, :j] = a.empty_token
        forced[n - K + j, :, j] = a.eos if a.eos > 0 else a.eog
    xs, ys = [p[0][0] for p in pr], [p[2][0] for p in pr]
    t = {tag: [] for tag in engs}
    tp = {tag: [] for tag in engs}          # the same calls' prefill (the packer and, on the centred engine, kv8c_centre_k behind every pass)
    steps = {}
    for tag, e in engs.items():          # warm-up: captures the graphs of this width
        e.inference_tts_multi(xs, ys, top_k=1, _forced=forced)
    for r in range(pairs):
        for tag, e in engs.items():
            e.inference_tts_multi(xs, ys, top_k=1, _forced=forced)
            t[tag].append(e.last_timing_ms()["decode_ms"])
            tp[tag].append(e.last_timing_ms()["prefill_ms"])
            steps[tag] = e.last_steps
    assert steps["off"] == steps["on"] == steps["centred"], steps
    report(f"inference_tts_multi decode loop, {steps['on']} steps", B, t, "ms per call")
    report("inference_tts_multi prefill", B, tp, "ms per call")
