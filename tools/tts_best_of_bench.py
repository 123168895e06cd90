"""Best-of-N sampling inside multi-utterance TTS calls (include/vc_engine.h vc_tts_multi_best_of) at BASELINE config 3's
utterance shape: giga830M, bf16, hipGraph on, Lx 80 (--ragged: spread over 40..80), 150-frame prompts, top-k 40,
stop_repetition 3, synthetic weights as bench.py builds them (muted terminator: every sample runs to the length cap).

One engine; for every B of --batches (default 1, 4, 8) whole `inference_tts_multi(batch_size=N)` calls of B utterances x N
samples are timed, interleaved on the same engine with B sequential `inference_tts_batch(batch_size=N)` calls (the baseline:
one call per sentence, as the reference's Long TTS makes them).  Per B it prints one JSON line: prefill ms (the K/V and
logits replication included), decode ms per step, kept-frame codec tokens per second over the host wall of the call, steps,
the call's re-pack count (vc_debug_read "host_ms"[6]) and the ratio to the sequential baseline; medians over --reps.

    python tools/tts_best_of_bench.py [--batches 1,4,8] [--n 3] [--reps 3] [--ragged]
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
    p.add_argument("--batches", default="1,4,8")
    p.add_argument("--n", type=int, default=3, help="samples per utterance (the app's sample_batch_size)")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--preset", default="giga830M")
    p.add_argument("--lx", type=int, default=80)
    p.add_argument("--frames", type=int, default=150)
    p.add_argument("--ragged", action="store_true", help="spread Lx over lx/2 .. lx")
    args = p.parse_args()
    from voicecraft_amd import synth
    from voicecraft_amd.engine import VoiceCraftEngine
    a = synth.make_args(args.preset)
    sd = synth.make_state_dict(a, seed=0, perturb=False, mute_eos=True, fast=True)
    K, N = a.n_codebooks, args.n
    batches = [int(b) for b in args.batches.split(",")]
    U = max(batches)
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype="bf16", max_seqs=U * N, max_positions=2048, use_graph=True)
    lxs = [args.lx - (u * (args.lx // 2)) // max(1, U - 1) if args.ragged else args.lx for u in range(U)]
    prompts = [synth.random_prompt(a, lxs[u], args.frames, seed=1 + u) for u in range(U)]
    xs = [pr[0][0].cuda() for pr in prompts]
    ys = [pr[2][0].cuda() for pr in prompts]
    knobs = dict(top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3, silence_tokens=[1388, 1898, 131])

    def timing(tokens, wall):
        t = eng.last_timing_ms()
        return dict(prefill_ms=t["prefill_ms"], decode_ms_per_step=t["decode_ms"] / max(1, eng.last_steps), tok_s=tokens / wall,
                    wall_ms=wall * 1e3, steps=eng.last_steps, repacks=float(eng.debug_read("host_ms", (8,), torch.float64)[6]))

    def call_multi(B, seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = eng.inference_tts_multi(xs[:B], ys[:B], batch_size=N, _seed=seed, **knobs)
        torch.cuda.synchronize()
        return timing(sum(int(o[1].shape[2]) * K for o in outs), time.perf_counter() - t0)

    def call_seq(B, seed):
        """B sequential inference_tts_batch calls: summed walls and steps, prefill / step time of the calls averaged."""
        parts = []
        for u in range(B):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res, gen = eng.inference_tts_batch(xs[u][None], torch.tensor([lxs[u]]).cuda(), ys[u][None], batch_size=N,
                                               _seed=seed + u, **knobs)
            torch.cuda.synchronize()
            parts.append(timing(int(gen.shape[2]) * K, time.perf_counter() - t0))
            parts[-1]["tokens"] = int(gen.shape[2]) * K
        wall = sum(x["wall_ms"] for x in parts) / 1e3
        return dict(prefill_ms=statistics.mean(x["prefill_ms"] for x in parts),
                    decode_ms_per_step=statistics.mean(x["decode_ms_per_step"] for x in parts),
                    tok_s=sum(x["tokens"] for x in parts) / wall, wall_ms=wall * 1e3, steps=sum(x["steps"] for x in parts),
                    repacks=sum(x["repacks"] for x in parts))

    for B in batches:                                    # warm-up: graphs captured, caches touched
        call_multi(B, seed=100 + B)
    call_seq(1, seed=99)
    runs = {B: {"multi": [], "seq": []} for B in batches}
    for r in range(args.reps):
        for B in batches:                                # batched and sequential calls interleaved on the same engine
            runs[B]["seq"].append(call_seq(B, seed=1000 * r))
            runs[B]["multi"].append(call_multi(B, seed=1000 * r))
    for B in batches:
        med = {kind: {k: statistics.median(x[k] for x in v) for k in v[0]} for kind, v in runs[B].items()}
        m, s = med["multi"], med["seq"]
        print(json.dumps({"entry": "inference_tts_multi", "B": B, "N": N, "rows": B * N, "ragged": args.ragged,
                          "prefill_ms": round(m["prefill_ms"], 3), "decode_ms_per_step": round(m["decode_ms_per_step"], 4),
                          "tok_s": round(m["tok_s"], 1), "steps": m["steps"], "repacks": m["repacks"], "wall_ms": round(m["wall_ms"], 2),
                          "seq_tok_s": round(s["tok_s"], 1), "seq_wall_ms": round(s["wall_ms"], 2),
                          "seq_decode_ms_per_step": round(s["decode_ms_per_step"], 4), "x_sequential": round(m["tok_s"] / s["tok_s"], 3)}),
              flush=True)


if __name__ == "__main__":
    main()
