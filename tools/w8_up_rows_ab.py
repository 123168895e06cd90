"""In-process A/Bs of option `w8ur` on ONE engine created with w8=, w8_rows=True, w8_mid=True and w8_up_rows=True (giga830M, bf16, the
synthetic checkpoint with THREE matrices quantised): interleaved pairs of `w8ur = 10` (bit 8: at every row count, whatever the win
table says) against `w8ur = 0`, whose launches are the parent commit's machine code (profiles/w8_up_rows_kernel_body_diff.log): that leg
is the baseline.  Logits of forced calls at every measured row count are asserted equal between the legs first.  Then
  - the isolated launch of the site (vc_bench_kernel "ffn1": eager, back to back, iteration i on the weights of layer i % L),
  - the captured decode loop per step of inference_tts_multi with 2, 4, 5, 8, 9, 12 and 16 utterances, `w8r` and `w8m` off,
  - the decode loop of an 8- and a 16-utterance inference_tts_multi at bench.py's shapes (650 generated frames per utterance) with
    `w8r` and `w8m` on in both legs (the terminator is muted, so all rows run to the end).
Every line holds the median of the per-pair deltas and their min..max: plan_pass takes the form at a row count only where the whole
range of that count's decode-loop line is below zero, an unmeasured count following the nearest measured one of the same kernel form
(2..4, 5..8, 9..16 rows; csrc/vc_engine_host.h W8_FORMS, row `w8ur`).  JSON lines on stdout.
usage: python tools/w8_up_rows_ab.py [pairs = 7] > profiles/w8_up_rows_ab.log"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from voicecraft_amd import quant, synth
from voicecraft_amd.engine import VoiceCraftEngine

pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
assert pairs >= 7, "at least 7 pairs per line"
ROWS = (2, 4, 5, 8, 9, 12, 16)
a = synth.make_args("giga830M")
K = a.n_codebooks
sdq = quant.quantize_state_dict_w8(a, synth.make_state_dict(a, seed=0, perturb=False, mute_eos=True, fast=True), ffn_up=True)
eng = VoiceCraftEngine(a, sdq, device="cuda:0", dtype="bf16", max_seqs=16, max_positions=1024, w8="as_is", w8_rows=True, w8_mid=True,
                       w8_up_rows=True)
print(json.dumps({"options": eng.options(), "packed_layers": sum(l["ffn_up_rows"]["state"] == "packed" for l in eng.w8_stats())}), flush=True)
knobs = dict(top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)
med = lambda xs: sorted(xs)[len(xs) // 2]


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
    for v in (0, 10):
        eng.set_option("w8ur", v)
        c0 = eng.launch_counts()["w8_up_rows"]
        lg[v] = eng.inference_tts_multi(xs, ys, top_k=1, _forced=toks, _logit_steps=N)[1].cpu().numpy()
        assert (eng.launch_counts()["w8_up_rows"] > c0) == bool(v)
    assert np.array_equal(lg[0], lg[10]), rows
    print(json.dumps({"logits_equal": True, "rows": rows, "steps": N}), flush=True)

# ---- the isolated launch
for rows in ROWS:
    def timed(v):
        eng.set_option("w8ur", v)
        return min(eng.bench_kernel("ffn1", n_rows=rows, iters=64)[0] for _ in range(2)) * 1e3
    timed(0); timed(10)
    a_us, b_us, deltas = [], [], []
    for i in range(pairs):
        t = {v: timed(v) for v in ((0, 10) if i % 2 == 0 else (10, 0))}
        a_us.append(t[0]); b_us.append(t[10]); deltas.append((t[10] - t[0]) / t[0] * 100.0)
    print(json.dumps(dict(what="ffn1", rows=rows, pairs=pairs, A="w8ur=0", B="w8ur=10", unit="us per launch, eager (vc_bench_kernel)",
                          A_median=round(med(a_us), 3), B_median=round(med(b_us), 3), median_delta_pct=round(med(deltas), 3),
                          min_delta_pct=round(min(deltas), 3), max_delta_pct=round(max(deltas), 3))), flush=True)


# ---- captured decode loops (bench.ab_block: interleaved whole calls, device-timed loop per step taken)
def loop_ab(tag, call, **kw):
    t0 = time.time()
    r = bench.ab_block(eng, call, "w8ur=0:10", pairs)
    print(json.dumps(dict(kw, what=tag, pairs=pairs, A="w8ur=0", B="w8ur=10", unit="decode ms per step taken", A_median=r["A_ms_median"],
                          B_median=r["B_ms_median"], median_delta_pct=r["median_delta_pct"], min_delta_pct=min(r["deltas_pct"]),
                          max_delta_pct=max(r["deltas_pct"]), whole_range_below_zero=max(r["deltas_pct"]) < 0,
                          steps=eng.last_steps, wall_s=round(time.time() - t0, 1))), flush=True)


eng.set_option("w8r", 0)
eng.set_option("w8m", 0)
for rows in ROWS:
    xs, ys = prompts(rows, 40)               # 250 generated frames per utterance (the reference's length cap)
    loop_ab("inference_tts_multi", lambda seed: eng.inference_tts_multi(xs, ys, silence_tokens=[1388, 1898, 131], _seed=seed, **knobs), rows=rows)
eng.set_option("w8r", 5)
eng.set_option("w8m", 1)
for rows in (8, 16):
    xs, ys = prompts(rows, 80)               # bench.py's shapes: 650 generated frames
    loop_ab(f"inference_tts_multi, {rows} utterances, w8r and w8m on",
            lambda seed: eng.inference_tts_multi(xs, ys, silence_tokens=[1388, 1898, 131], _seed=seed, **knobs), rows=rows)
