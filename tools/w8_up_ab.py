"""In-process A/Bs of option `w8u` on ONE engine created with w8=, w8_wide=True and w8_up=True (giga830M, bf16, max_seqs = 64, the
synthetic checkpoint with THREE matrices on the grid: quant.quantize_state_dict_w8(..., ffn_up=True)): interleaved pairs of `w8u = 10`
(the form at every row count, whatever the win table says) against `w8u = 0`, whose launches are the parent commit's machine code
(profiles/w8_up_kernel_body_diff.log).  Logits of forced 17-, 33- and 64-row calls are asserted equal between the legs first.  Then
  - the isolated launch of the site (vc_bench_kernel "wd_ffn1": eager, back to back, iteration i on the weights of layer i % L) at 32
    and 64 rows,
  - the captured decode loop per step of inference_tts_multi with 17, 24, 32, 33, 48 and 64 utterances, `w8w = 0` in both legs (FFN-up
    alone), then `w8w = 13` in both legs (next to the FFN-down and QKV planes),
  - the same at 32 and 64 utterances on a second engine that has kv8=True (and no w8_wide).
Every line holds the median of the per-pair deltas and their min..max: a row count stays in row `w8u` of W8_FORMS (csrc/vc_engine_host.h) only
where the whole range of its FFN-up-alone line AND of its next-to-w8w line is below zero; row counts between measured ones follow the
nearest measured count of the same number of row tiles (17..32, 33..64).  JSON lines on stdout.
usage: python tools/w8_up_ab.py [pairs = 7] > profiles/w8_up_ab.log"""
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
sdq = quant.quantize_state_dict_w8(a, synth.make_state_dict(a, seed=0, perturb=False, mute_eos=True, fast=True), ffn_up=True)
knobs = dict(top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)


def make_engine(**kw):
    free0 = torch.cuda.mem_get_info()[0]
    eng = VoiceCraftEngine(a, sdq, device="cuda:0", dtype="bf16", max_seqs=64, max_positions=1024, w8="as_is", w8_up=True, **kw)
    st = eng.w8_stats()
    print(json.dumps({"options": eng.options(), "kv8": bool(kw.get("kv8")), "w8_wide": bool(kw.get("w8_wide")),
                      "packed_layers_up": sum(l["ffn_up_wide"]["state"] == "packed" for l in st),
                      "device_memory_taken_GB": round((free0 - torch.cuda.mem_get_info()[0]) / 1e9, 3)}), flush=True)
    return eng


def prompts(n, lx, frames=150):
    ps = [synth.random_prompt(a, lx, frames, seed=1 + u) for u in range(n)]
    return [p[0][0].cuda() for p in ps], [p[2][0].cuda() for p in ps]


eng = make_engine(w8_wide=True)

# ---- the legs compute the same thing
N = 12
for rows in (17, 33, 64):
    xs, ys = prompts(rows, 20, 30)
    toks = np.random.RandomState(17).randint(0, a.audio_vocab_size, size=(N, rows, K)).astype(np.int64)
    for j in range(K):
        toks[N - K + j, :, :j] = a.empty_token
        toks[N - K + j, :, j] = a.eos
    lg = {}
    for v in (0, 10):
        eng.set_option("w8u", v)
        c0 = eng.launch_counts()["w8_up"]
        lg[v] = eng.inference_tts_multi(xs, ys, top_k=1, _forced=toks, _logit_steps=N)[1].cpu().numpy()
        assert (eng.launch_counts()["w8_up"] > c0) == bool(v)
    assert np.array_equal(lg[0], lg[10]), rows
    print(json.dumps({"logits_equal": True, "rows": rows, "steps": N}), flush=True)


med = lambda xs: sorted(xs)[len(xs) // 2]

# ---- the isolated launch
for rows in (32, 64):
    def timed(v):
        eng.set_option("w8u", v)
        return min(eng.bench_kernel("wd_ffn1", n_rows=rows, iters=64)[0] for _ in range(2)) * 1e3
    timed(0); timed(10)
    a_us, b_us, deltas = [], [], []
    for i in range(pairs):
        t = {v: timed(v) for v in ((0, 10) if i % 2 == 0 else (10, 0))}
        a_us.append(t[0]); b_us.append(t[10]); deltas.append((t[10] - t[0]) / t[0] * 100.0)
    print(json.dumps(dict(what="wd_ffn1", rows=rows, pairs=pairs, A="w8u=0", B="w8u=10", unit="us per launch, eager (vc_bench_kernel)",
                          A_median=round(med(a_us), 3), B_median=round(med(b_us), 3), median_delta_pct=round(med(deltas), 3),
                          min_delta_pct=round(min(deltas), 3), max_delta_pct=round(max(deltas), 3))), flush=True)


# ---- captured decode loops (bench.ab_block: interleaved whole calls, device-timed loop per step taken)
def block(e, rows_list, **kw):
    for rows in rows_list:
        xs, ys = prompts(rows, 24)
        call = lambda seed: e.inference_tts_multi(xs, ys, silence_tokens=[1388, 1898, 131], _seed=seed, **knobs)
        t0 = time.time()
        r = bench.ab_block(e, call, "w8u=0:10", pairs)
        print(json.dumps(dict(kw, rows=rows, what="inference_tts_multi", pairs=pairs, A="w8u=0", B="w8u=10", unit="decode ms per step taken",
                              A_median=r["A_ms_median"], B_median=r["B_ms_median"], median_delta_pct=r["median_delta_pct"],
                              min_delta_pct=min(r["deltas_pct"]), max_delta_pct=max(r["deltas_pct"]),
                              whole_range_below_zero=max(r["deltas_pct"]) < 0, steps=e.last_steps, wall_s=round(time.time() - t0, 1))), flush=True)


for w8w in (0, 13):
    eng.set_option("w8w", w8w)
    block(eng, ROWS, w8w=w8w)
del eng
torch.cuda.empty_cache()
eng = make_engine(kv8=True)
block(eng, (32, 64), kv8=True)
