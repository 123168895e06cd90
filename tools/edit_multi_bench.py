"""Batched speech editing at BASELINE config 4's shape (include/vc_engine.h vc_edit_multi): giga830M, bf16, hipGraph on,
Lx 80, an 800-frame utterance per request with the span [300, 400) re-generated up to the reference's length cap.

One engine; for every batch size B of --batches (default 1, 8, 16) whole `inference_multi` calls of B requests are timed,
interleaved with single-request `inference` calls on the same engine (the 3-row-switch path of vc_edit, the baseline a batch
is compared with).  Per B it prints one JSON line: prefill ms, decode ms per step, generated codec tokens per second (host wall
of the whole call, as bench.py counts C4) and the re-pack count of the call (vc_debug_read "host_ms"[6]), medians over --reps.

    python tools/edit_multi_bench.py [--batches 1,8,16] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--batches", default="1,8,16")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--preset", default="giga830M")
    p.add_argument("--lx", type=int, default=80)
    args = p.parse_args()
    from voicecraft_amd import synth
    from voicecraft_amd.engine import VoiceCraftEngine
    a = synth.make_args(args.preset)
    sd = synth.make_state_dict(a, seed=0, perturb=False, mute_eos=True, fast=True)
    K = a.n_codebooks
    frames = 10 * args.lx
    span = (frames * 3 // 8, frames // 2)
    kept = frames - (span[1] - span[0])                  # frames of the utterance outside the span
    batches = [int(b) for b in args.batches.split(",")]
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype="bf16", max_seqs=max(batches), max_positions=1024, use_graph=True)
    prompts = [synth.random_prompt(a, args.lx, frames, seed=1 + u) for u in range(max(batches))]
    xs = [pr[0][0].cuda() for pr in prompts]
    ys = [pr[2][0].cuda() for pr in prompts]
    knobs = dict(top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3, silence_tokens=[1388, 1898, 131])

    def call(B, seed):
        """B = 0: one single-request `inference`; else one `inference_multi` of B requests."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if B == 0:
            res = eng.inference(xs[0][None], torch.tensor([args.lx]).cuda(), ys[0][None], torch.tensor([[list(span)]]),
                                _seed=seed, **knobs)
            tokens = (int(res.shape[2]) - kept) * K
        else:
            outs = eng.inference_multi(xs[:B], ys[:B], [[span]] * B, _seed=seed, **knobs)
            tokens = sum((int(o.shape[2]) - kept) * K for o in outs)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        t = eng.last_timing_ms()
        return dict(prefill_ms=t["prefill_ms"], decode_ms_per_step=t["decode_ms"] / max(1, eng.last_steps),
                    tok_s=tokens / wall, wall_ms=wall * 1e3, steps=eng.last_steps,
                    repacks=float(eng.debug_read("host_ms", (8,), torch.float64)[6]) if B else 0.0)

    for B in [0] + batches:                              # warm-up: graphs captured, caches touched
        call(B, seed=100 + B)
    runs = {B: [] for B in [0] + batches}
    for r in range(args.reps):
        for B in batches:                                # single and batched calls interleaved on the same engine
            runs[0].append(call(0, seed=r))
            runs[B].append(call(B, seed=r))
    med = {B: {k: statistics.median(x[k] for x in v) for k in v[0]} for B, v in runs.items()}
    for B in [0] + batches:
        m = med[B]
        print(json.dumps({"entry": "inference" if B == 0 else "inference_multi", "B": max(B, 1), "prefill_ms": round(m["prefill_ms"], 3),
                          "decode_ms_per_step": round(m["decode_ms_per_step"], 4), "tok_s": round(m["tok_s"], 1),
                          "repacks": m["repacks"], "steps": m["steps"], "wall_ms": round(m["wall_ms"], 2),
                          "x_single": round(m["tok_s"] / med[0]["tok_s"], 2)}), flush=True)


if __name__ == "__main__":
    main()
