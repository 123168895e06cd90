"""In-process A/Bs of option `w8m` on ONE engine created with w8=, w8_rows=True, w8_mid=True and w8_wide=True (giga830M, bf16, the
QUANTISED synthetic checkpoint of tools/w8_ab.py): interleaved pairs of `w8m = 9` (bit 8: at every row count, whatever the win table
says) against `w8m = 0`, whose launches are the parent commit's machine code (profiles/w8_mid_kernel_body_diff.log).  Logits of forced
9-, 12- and 16-row calls are asserted equal between the legs first.  Then
  - the captured decode loop per step of inference_tts_multi with 9, 12 and 16 utterances,
  - the decode loop of a 16-utterance inference_tts_multi at bench.py's shapes (650 generated frames per utterance) with `w8r` and
    `w8w` on in both legs (the terminator is muted, so all 16 rows run to the end and neither of the two has a step to take).
Every line holds the median of the per-pair deltas and their min..max: plan_pass takes the form at a row count only where the whole
range of that count's decode-loop line is below zero, an unmeasured count following the nearest measured one (csrc/vc_engine_host.h W8_FORMS,
row `w8m`).  JSON lines on stdout.
usage: python tools/w8_mid_ab.py [pairs = 7] > profiles/w8_mid_ab.log"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from voicecraft_amd import quant, synth
from voicecraft_amd.engine import VoiceCraftEngine

pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
assert pairs >= 7, "at least 7 pairs per line"
ROWS = (9, 12, 16)
a = synth.make_args("giga830M")
K = a.n_codebooks
sdq = quant.quantize_state_dict_w8(a, synth.make_state_dict(a, seed=0, perturb=False, mute_eos=True, fast=True))
eng = VoiceCraftEngine(a, sdq, device="cuda:0", dtype="bf16", max_seqs=17, max_positions=1024, w8="as_is", w8_rows=True, w8_mid=True,
                       w8_wide=True)
print(json.dumps({"options": eng.options(), "packed_layers": sum(l["ffn_down"]["state"] == "packed" for l in eng.w8_stats())}), flush=True)
knobs = dict(top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)


def prompts(n, lx, frames=150):
    ps = [synth.random_prompt(a, lx, frames, seed=1 + u) for u in range(n)]
    return [p[0][0].cuda() for p in ps], [p[2][0].cuda() for p in ps]


# ---- the legs compute the same thing
N = 12
for rows in ROWS:
    xs, ys = prompts(rows, 20, 30)
    toks = np.random.RandomState(17).randint(0, a.audio_vocab_size, size=(N, rows, K)).astype(np.int64)
    for j in range(K):
        toks[N - K + j, :, :j] = a.empty_token
        toks[N - K + j, :, j] = a.eos
    lg = {}
    for v in (0, 9):
        eng.set_option("w8m", v)
        c0 = eng.launch_counts()["w8_mid"]
        lg[v] = eng.inference_tts_multi(xs, ys, top_k=1, _forced=toks, _logit_steps=N)[1].cpu().numpy()
        assert (eng.launch_counts()["w8_mid"] > c0) == bool(v)
    assert np.array_equal(lg[0], lg[9]), rows
    print(json.dumps({"logits_equal": True, "rows": rows, "steps": N}), flush=True)


# ---- captured decode loops (bench.ab_block: interleaved whole calls, device-timed loop per step taken)
def loop_ab(tag, call, **kw):
    t0 = time.time()
    r = bench.ab_block(eng, call, "w8m=0:9", pairs)
    print(json.dumps(dict(kw, what=tag, pairs=pairs, A="w8m=0", B="w8m=9", unit="decode ms per step taken", A_median=r["A_ms_median"],
                          B_median=r["B_ms_median"], median_delta_pct=r["median_delta_pct"], min_delta_pct=min(r["deltas_pct"]),
                          max_delta_pct=max(r["deltas_pct"]), whole_range_below_zero=max(r["deltas_pct"]) < 0,
                          steps=eng.last_steps, wall_s=round(time.time() - t0, 1))), flush=True)


for rows in ROWS:
    xs, ys = prompts(rows, 40)               # 250 generated frames per utterance (the reference's length cap)
    loop_ab("inference_tts_multi", lambda seed: eng.inference_tts_multi(xs, ys, silence_tokens=[1388, 1898, 131], _seed=seed, **knobs), rows=rows)
xs, ys = prompts(16, 80)                     # bench.py's shapes: 650 generated frames
loop_ab("inference_tts_multi, 16 utterances, w8r and w8w on",
        lambda seed: eng.inference_tts_multi(xs, ys, silence_tokens=[1388, 1898, 131], _seed=seed, **knobs), rows=16)
