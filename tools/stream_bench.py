"""Streaming TTS against the blocking request, on ONE engine, interleaved pairs (as tools/ab_sweep.py does):
python tools/stream_bench.py [--preset giga830M] [--pairs 10] [--chunks 8,25]

Workload: BASELINE config 3's utterance (giga830M shape, bf16, 80 phonemes, 150 prompt frames, top-k 40, seeded; the
synthetic checkpoint mutes the terminator, so 650 frames = 13 s are generated).  Prints JSON lines:
  * first_audio: host time from the call to the first waveform chunk (stream: tokens -> chunked codec decode on a side
    stream) against the blocking request = inference_tts + tokenizer.decode of the same utterance;
  * decode_loop: vc_last_timing ms[1] of the streamed call against the blocking call's, same pairs - with the codec chunks
    running next to it (stream_chunkN) and with the tokens merely consumed (tokens_only_chunkN);
  * codec_chunked: device time of a chunked decode of 650 frames (sum over the chunks) against one vc_codec_decode.
Synthetic weights may sample a special token id on codebook 0; the codec takes 0..2047, so ids are clamped before they are
decoded (both arms)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from voicecraft_amd import synth
from voicecraft_amd.codec import AudioTokenizer
from voicecraft_amd.engine import VoiceCraftEngine

p = argparse.ArgumentParser()
p.add_argument("--preset", default="giga830M")
p.add_argument("--lx", type=int, default=80)
p.add_argument("--prompt-frames", type=int, default=150)
p.add_argument("--top-k", type=int, default=40)
p.add_argument("--pairs", type=int, default=10)
p.add_argument("--chunks", default="8,25")
args = p.parse_args()
chunks = [int(c) for c in args.chunks.split(",")]
dev = torch.device("cuda", 0)
a = synth.make_args(args.preset)
sd = synth.make_state_dict(a, seed=0, perturb=False, mute_eos=True, fast=True)
eng = VoiceCraftEngine(a, sd, device=dev, dtype="bf16", max_seqs=1, max_positions=1024)
tok = AudioTokenizer(synth.make_codec_state_dict(0), device=dev, max_seconds=20.0)
x, xl, y = (t.to(dev) for t in synth.random_prompt(a, args.lx, args.prompt_frames, seed=1))
kn = dict(top_k=args.top_k, top_p=1.0, temperature=1.0, stop_repetition=3, silence_tokens=[1388, 1898, 131])
side = torch.cuda.Stream(device=dev)


def blocking(seed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res, gen = eng.inference_tts(x, xl, y, _seed=seed, **kn)
    wav = tok.decode([(gen.clamp(max=2047), None)])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return dict(total_ms=(t1 - t0) * 1e3, loop_ms=eng.last_timing_ms()["decode_ms"], frames=int(gen.shape[2]), samples=int(wav.shape[2]))


def streamed(seed, chunk):
    torch.cuda.synchronize()
    dec = tok.decode_stream()
    t0 = time.perf_counter()
    first, n_samples, n_chunks = None, 0, 0
    for _f, codes in eng.inference_tts_stream(x, xl, y, chunk_frames=chunk, _seed=seed, **kn):
        with torch.cuda.stream(side):
            wav = dec.feed(codes.clamp(max=2047))
        if wav.shape[2]:
            n_chunks += 1
            n_samples += int(wav.shape[2])
            if first is None:
                first = (time.perf_counter() - t0) * 1e3
    with torch.cuda.stream(side):
        n_samples += int(dec.feed(torch.empty((1, tok.n_q, 0), dtype=torch.int64, device=dev), last=True).shape[2])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return dict(first_ms=first, total_ms=(t1 - t0) * 1e3, loop_ms=eng.last_timing_ms()["decode_ms"], samples=n_samples, chunks=n_chunks,
                codec_ms=dec.ms)


def tokens_only(seed, chunk):
    """the streamed call with nobody decoding audio next to it: what the resumable loop itself costs"""
    torch.cuda.synchronize()
    for _f, _codes in eng.inference_tts_stream(x, xl, y, chunk_frames=chunk, _seed=seed, **kn):
        pass
    return dict(loop_ms=eng.last_timing_ms()["decode_ms"])


def stats(v):
    v = sorted(v)
    return dict(median=round(statistics.median(v), 3), min=round(v[0], 3), max=round(v[-1], 3), n=len(v))


blocking(0); streamed(0, chunks[0])                 # graphs captured, allocator warm
rows = {"blocking": [], **{f"stream{c}": [] for c in chunks}, **{f"tokens{c}": [] for c in chunks}}
for i in range(args.pairs):
    seed = 100 + i
    order = ["blocking"] + [f"stream{c}" for c in chunks] + [f"tokens{c}" for c in chunks]
    if i % 2:
        order.reverse()
    for arm in order:
        rows[arm].append(blocking(seed) if arm == "blocking" else
                         streamed(seed, int(arm[6:])) if arm.startswith("stream") else tokens_only(seed, int(arm[6:])))
frames = rows["blocking"][0]["frames"]
assert all(r["samples"] == rows["blocking"][0]["samples"] for arm in rows if not arm.startswith("tokens") for r in rows[arm])
print(json.dumps({"preset": args.preset, "frames": frames, "pairs": args.pairs, "options": eng.options()}), flush=True)
out = {"blocking_request_ms": stats([r["total_ms"] for r in rows["blocking"]])}
for c in chunks:
    out[f"stream_chunk{c}_first_audio_ms"] = stats([r["first_ms"] for r in rows[f"stream{c}"]])
    out[f"stream_chunk{c}_total_ms"] = stats([r["total_ms"] for r in rows[f"stream{c}"]])
print(json.dumps({"first_audio": out}), flush=True)
out = {"blocking_loop_ms": stats([r["loop_ms"] for r in rows["blocking"]])}
for c in chunks:
    out[f"stream_chunk{c}_loop_ms"] = stats([r["loop_ms"] for r in rows[f"stream{c}"]])
    d = [s["loop_ms"] / b["loop_ms"] - 1 for s, b in zip(rows[f"stream{c}"], rows["blocking"])]
    out[f"stream_chunk{c}_vs_blocking_pct"] = stats([100 * v for v in d])
    out[f"tokens_only_chunk{c}_loop_ms"] = stats([r["loop_ms"] for r in rows[f"tokens{c}"]])
    d = [s["loop_ms"] / b["loop_ms"] - 1 for s, b in zip(rows[f"tokens{c}"], rows["blocking"])]
    out[f"tokens_only_chunk{c}_vs_blocking_pct"] = stats([100 * v for v in d])
    out[f"stream_chunk{c}_codec_device_ms"] = stats([r["codec_ms"] for r in rows[f"stream{c}"]])
print(json.dumps({"decode_loop": out}), flush=True)

# ---- the codec alone: 650 frames, one call against chunks
codes = torch.randint(0, 2048, (1, tok.n_q, 650), device=dev)
one, chunked = [], {c: [] for c in chunks}
for _ in range(5):
    want = tok.decode([(codes, None)])
    one.append(tok.last_ms())
    for c in chunks:
        dec, got = tok.decode_stream(), []
        for f0 in range(0, 650, c):
            got.append(dec.feed(codes[:, :, f0: f0 + c], last=f0 + c >= 650))
        assert torch.equal(torch.cat(got, dim=2), want)
        chunked[c].append(dec.ms)
out = {"one_call_ms": stats(one[1:])}
for c in chunks:
    out[f"chunks_of_{c}_ms"] = stats(chunked[c][1:])
    out[f"chunks_of_{c}_ratio"] = round(statistics.median(chunked[c][1:]) / statistics.median(one[1:]), 2)
print(json.dumps({"codec_chunked": out, "lookahead_frames": tok.decode_stream().lookahead_frames}), flush=True)
