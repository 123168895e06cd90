"""In-process A/Bs of option `w8w` on ONE engine created with w8= and w8_wide=True (giga830M, bf16, max_seqs = 64, the QUANTISED
synthetic checkpoint of tools/w8_ab.py): interleaved pairs of `w8w = 8 | mask` (the form at every row count, whatever the win table
says) against `w8w = 0`, whose launches are the parent commit's machine code (profiles/w8_wide_kernel_body_diff.log).  Logits of forced
17-, 33- and 64-row calls are asserted equal between the legs first.  Then
  - the captured decode loop per step of inference_tts_multi with 17, 24, 32, 33, 48 and 64 utterances, one line per mask 1 / 4 / 5,
  - the same at 32 and 64 utterances, mask 5, on a second engine that also has kv8=True.
Every line holds the median of the per-pair deltas and their min..max: a (matrix, row count) stays in row `w8w` of W8_FORMS
(csrc/vc_engine_host.h) only where the whole range of its line is below zero; row counts between measured ones follow the nearest
measured count of the same number of row tiles (17..32, 33..64).  The isolated launches of the two sites (vc_bench_kernel "wd_ffn2",
"wd_qkv": eager, back to back, iteration i on the weights of layer i % L) at 32 and 64 rows come first.  JSON lines on stdout.
usage: python tools/w8_wide_ab.py [pairs = 7] > profiles/w8_wide_ab.log"""
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
ROWS = (17, 24, 32, 33, 48, 64)
a = synth.make_args("giga830M")
K = a.n_codebooks
sdq = quant.quantize_state_dict_w8(a, synth.make_state_dict(a, seed=0, perturb=False, mute_eos=True, fast=True))
knobs = dict(top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)


def make_engine(**kw):
    eng = VoiceCraftEngine(a, sdq, device="cuda:0", dtype="bf16", max_seqs=64, max_positions=1024, w8="as_is", w8_wide=True, **kw)
    st = eng.w8_stats()
    print(json.dumps({"options": eng.options(), "kv8": bool(kw.get("kv8")),
                      "packed_layers_wide": sum(l["ffn_down_wide"]["state"] == "packed" and l["qkv_wide"]["state"] == "packed" for l in st)}), flush=True)
    return eng


def prompts(n, lx, frames=150):
    ps = [synth.random_prompt(a, lx, frames, seed=1 + u) for u in range(n)]
    return [p[0][0].cuda() for p in ps], [p[2][0].cuda() for p in ps]


eng = make_engine()
MASK = eng.W8_WIDE_MASK

# ---- the legs compute the same thing
N = 12
for rows in (17, 33, 64):
    xs, ys = prompts(rows, 20, 30)
    toks = np.random.RandomState(17).randint(0, a.audio_vocab_size, size=(N, rows, K)).astype(np.int64)
    for j in range(K):
        toks[N - K + j, :, :j] = a.empty_token
        toks[N - K + j, :, j] = a.eos
    lg = {}
    for v in (0, 8 | MASK):
        eng.set_option("w8w", v)
        c0 = eng.launch_counts()["w8_wide"]
        lg[v] = eng.inference_tts_multi(xs, ys, top_k=1, _forced=toks, _logit_steps=N)[1].cpu().numpy()
        assert (eng.launch_counts()["w8_wide"] > c0) == bool(v)
    assert np.array_equal(lg[0], lg[8 | MASK]), rows
    print(json.dumps({"logits_equal": True, "rows": rows, "steps": N}), flush=True)


med = lambda xs: sorted(xs)[len(xs) // 2]

# ---- isolated launches
for rows in (32, 64):
    for which, mask in (("wd_ffn2", 1), ("wd_qkv", 4)):
        def timed(v):
            eng.set_option("w8w", v)
            return min(eng.bench_kernel(which, n_rows=rows, iters=64)[0] for _ in range(2)) * 1e3
        timed(0); timed(8 | mask)
        a_us, b_us, deltas = [], [], []
        for i in range(pairs):
            t = {v: timed(v) for v in ((0, 8 | mask) if i % 2 == 0 else (8 | mask, 0))}
            a_us.append(t[0]); b_us.append(t[8 | mask]); deltas.append((t[8 | mask] - t[0]) / t[0] * 100.0)
        print(json.dumps(dict(what=which, rows=rows, pairs=pairs, A="w8w=0", B=f"w8w={8 | mask}", unit="us per launch, eager (vc_bench_kernel)",
                              A_median=round(med(a_us), 3), B_median=round(med(b_us), 3), median_delta_pct=round(med(deltas), 3),
                              min_delta_pct=round(min(deltas), 3), max_delta_pct=round(max(deltas), 3))), flush=True)


# ---- captured decode loops (bench.ab_block: interleaved whole calls, device-timed loop per step taken)
def loop_ab(e, tag, call, masks, **kw):
    for mask in masks:
        t0 = time.time()
        r = bench.ab_block(e, call, f"w8w=0:{8 | mask}", pairs)
        print(json.dumps(dict(kw, what=tag, pairs=pairs, A="w8w=0", B=f"w8w={8 | mask}", unit="decode ms per step taken", A_median=r["A_ms_median"],
                              B_median=r["B_ms_median"], median_delta_pct=r["median_delta_pct"], min_delta_pct=min(r["deltas_pct"]),
                              max_delta_pct=max(r["deltas_pct"]), whole_range_below_zero=max(r["deltas_pct"]) < 0,
                              steps=e.last_steps, wall_s=round(time.time() - t0, 1))), flush=True)


def block(e, rows_list, masks, **kw):
    for rows in rows_list:
        xs, ys = prompts(rows, 24)
        loop_ab(e, "inference_tts_multi", lambda seed: e.inference_tts_multi(xs, ys, silence_tokens=[1388, 1898, 131], _seed=seed, **knobs),
                masks, rows=rows, **kw)


block(eng, ROWS, (1, 4, MASK))
del eng
torch.cuda.empty_cache()
eng = make_engine(kv8=True)
block(eng, (32, 64), (MASK,), kv8=True)
