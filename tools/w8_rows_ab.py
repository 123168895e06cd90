"""In-process A/Bs of option `w8r` on ONE engine created with w8= and w8_rows=True (giga830M, bf16, the QUANTISED synthetic
checkpoint of tools/w8_ab.py): interleaved pairs of `w8r = mask` against `w8r = 0`, whose launches are the parent commit's machine code
(profiles/w8_rows_kernel_body_diff.log).  Logits of forced 3- and 8-row calls are asserted equal between the legs first.  Then
  - the isolated `rows_gemm_frp` and `rows_gemm_qp` launches and the eager `step` (vc_bench_kernel) at 2, 3, 4, 6 and 8 rows,
  - the captured decode loop per step of inference_tts_multi with 2, 3, 4, 6 and 8 utterances, one line per mask 1 / 4 / 5,
  - the decode loop of inference_tts_batch(batch_size=3) and of an 8-utterance inference_tts_multi at bench.py's shapes.
Every line holds the median of the per-pair deltas and their min..max: plan_pass takes the form at a row count only where the whole
range of the bit's decode-loop line is below zero (csrc/vc_engine_host.h W8_FORMS, row `w8r`).  JSON lines on stdout.
usage: python tools/w8_rows_ab.py [pairs = 7] > profiles/w8_rows_ab.log"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from voicecraft_amd import quant, synth
from voicecraft_amd.engine import VoiceCraftEngine

pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
assert pairs >= 7, "at least 7 pairs per line"
ROWS = (2, 3, 4, 6, 8)
a = synth.make_args("giga830M")
K = a.n_codebooks
sdq = quant.quantize_state_dict_w8(a, synth.make_state_dict(a, seed=0, perturb=False, mute_eos=True, fast=True))
eng = VoiceCraftEngine(a, sdq, device="cuda:0", dtype="bf16", max_seqs=8, max_positions=1024, w8="as_is", w8_rows=True)
MASK = eng.W8_ROWS_MASK
print(json.dumps({"options": eng.options(), "packed_layers": sum(all(v["state"] == "packed" for v in l.values()) for l in eng.w8_stats())}), flush=True)
knobs = dict(top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)


def prompts(n, lx, frames=150):
    ps = [synth.random_prompt(a, lx, frames, seed=1 + u) for u in range(n)]
    return [p[0][0].cuda() for p in ps], [p[2][0].cuda() for p in ps]


# ---- the legs compute the same thing
N = 12
for rows in (3, 8):
    xs, ys = prompts(rows, 20, 30)
    toks = np.random.RandomState(17).randint(0, a.audio_vocab_size, size=(N, rows, K)).astype(np.int64)
    for j in range(K):
        toks[N - K + j, :, :j] = a.empty_token
        toks[N - K + j, :, j] = a.eos
    lg = {}
    for v in (0, MASK):
        eng.set_option("w8r", v)
        c0 = eng.launch_counts()["w8_rows"]
        lg[v] = eng.inference_tts_multi(xs, ys, top_k=1, _forced=toks, _logit_steps=N)[1].cpu().numpy()
        assert (eng.launch_counts()["w8_rows"] > c0) == bool(v)
    assert np.array_equal(lg[0], lg[MASK]), rows
    print(json.dumps({"logits_equal": True, "rows": rows, "steps": N}), flush=True)

med = lambda xs: sorted(xs)[len(xs) // 2]


def line(tag, deltas, a_ms, b_ms, **kw):
    print(json.dumps(dict(kw, what=tag, pairs=len(deltas), A="w8r=0", A_median=round(med(a_ms), 5), B_median=round(med(b_ms), 5),
                          median_delta_pct=round(med(deltas), 3), min_delta_pct=round(min(deltas), 3), max_delta_pct=round(max(deltas), 3),
                          whole_range_below_zero=max(deltas) < 0)), flush=True)


# ---- isolated launches and the eager step
for rows in ROWS:
    for which, mask in (("rows_gemm_frp", 1), ("rows_gemm_qp", 4), ("step", MASK)):
        def timed(v):
            eng.set_option("w8r", v)
            return min(eng.bench_kernel(which, n_rows=rows, iters=64)[0] for _ in range(2)) * 1e3
        try:
            timed(0); timed(mask)
        except AssertionError as e:
            print(json.dumps({"what": which, "rows": rows, "not_launched": str(e)[-120:]}), flush=True)
            continue
        a_us, b_us, deltas = [], [], []
        for i in range(pairs):
            t = {v: timed(v) for v in ((0, mask) if i % 2 == 0 else (mask, 0))}
            a_us.append(t[0]); b_us.append(t[mask]); deltas.append((t[mask] - t[0]) / t[0] * 100.0)
        line(which, deltas, a_us, b_us, rows=rows, B=f"w8r={mask}", unit="us per launch, eager (vc_bench_kernel)")


# ---- captured decode loops (bench.ab_block: interleaved whole calls, device-timed loop per step taken)
def loop_ab(tag, call, masks, **kw):
    for mask in masks:
        t0 = time.time()
        r = bench.ab_block(eng, call, f"w8r=0:{mask}", pairs)
        print(json.dumps(dict(kw, what=tag, pairs=pairs, A="w8r=0", B=f"w8r={mask}", unit="decode ms per step taken", A_median=r["A_ms_median"],
                              B_median=r["B_ms_median"], median_delta_pct=r["median_delta_pct"], min_delta_pct=min(r["deltas_pct"]),
                              max_delta_pct=max(r["deltas_pct"]), whole_range_below_zero=max(r["deltas_pct"]) < 0,
                              steps=eng.last_steps, wall_s=round(time.time() - t0, 1))), flush=True)


for rows in ROWS:
    xs, ys = prompts(rows, 40)               # 250 generated frames per utterance (the reference's length cap)
    loop_ab("inference_tts_multi", lambda seed: eng.inference_tts_multi(xs, ys, silence_tokens=[1388, 1898, 131], _seed=seed, **knobs),
            (1, 4, MASK) if rows <= 6 else (1,), rows=rows)
xs, ys = prompts(8, 80)                      # bench.py's shapes: 650 generated frames
x1, xl1, y1 = xs[0][None], torch.tensor([xs[0].numel()]).cuda(), ys[0][None]
loop_ab("inference_tts_batch(batch_size=3)", lambda seed: eng.inference_tts_batch(x1, xl1, y1, batch_size=3, silence_tokens=[1388, 1898, 131],
                                                                                    _seed=seed, **knobs), (MASK,), rows=3)
loop_ab("inference_tts_multi, 8 utterances", lambda seed: eng.inference_tts_multi(xs, ys, silence_tokens=[1388, 1898, 131], _seed=seed, **knobs),
        (MASK,), rows=8)
