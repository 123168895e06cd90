"""In-process A/Bs of option `w8` on ONE engine created with w8= (giga830M, bf16, one utterance: bench.py's headline workload on the
QUANTISED synthetic checkpoint), with bench.py's own `ab_block` (interleaved pairs of whole calls, its rule for a default), as
tools/w13_ab.py does for `w13`.  The off-leg `w8=0` runs the default path (w13 = 5) on identical weights with identical outputs.
First the isolated launch times of the three big matrices (vc_bench_kernel) with the option off and on.  JSON lines on stdout.
usage: python tools/w8_ab.py w8=0:5,w8=0:1,w8=0:4 [runs of each = 1] [pairs = 7]         (profiles/w8_ab.log: 2 runs, 7 pairs)
       python tools/w8_ab.py --leg 0|5 [calls = 3]      one leg alone, for a kernel trace of it (rocprofv3 ... -- python tools/w8_ab.py --leg 5)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
from voicecraft_amd import quant, synth
from voicecraft_amd.engine import VoiceCraftEngine

leg = None
if sys.argv[1] == "--leg":
    leg, calls = int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 3
    specs = []
else:
    specs = sys.argv[1].split(",")
reps = int(sys.argv[2]) if leg is None and len(sys.argv) > 2 else 1
pairs = int(sys.argv[3]) if leg is None and len(sys.argv) > 3 else 7
a = synth.make_args("giga830M")
t0 = time.time()
sdq = quant.quantize_state_dict_w8(a, synth.make_state_dict(a, seed=0, perturb=False, mute_eos=True, fast=True))
t_quant = time.time() - t0
wl = bench.Workload("giga830M", "tts", 1, 80, 150, 40, "bf16", "cuda:0", sd=sdq)
plain = wl.eng                  # bench.py's engine: same capacities, no w8
wl.eng = eng = VoiceCraftEngine(a, sdq, device="cuda:0", dtype="bf16", max_seqs=plain.max_seqs, max_positions=plain.max_positions, w8="as_is")
del plain
print(json.dumps({"options": eng.options(), "quantize_s": round(t_quant, 1), "w8_layer0": eng.w8_stats()[0], "w13_layer0": eng.w13_stats()[0],
                  "packed_layers": sum(all(v["state"] == "packed" for v in l.values()) for l in eng.w8_stats())}), flush=True)
one_step = lambda seed: wl.call(seed)[1]
if leg is not None:
    eng.set_option("w8", leg)       # before the warm-up calls: a trace of this process holds one leg's launches only
for w in range(2):
    one_step(100 + w)
torch.cuda.synchronize()
if leg is not None:
    for c in range(calls):
        one_step(200 + c)
    torch.cuda.synchronize()
    print(json.dumps({"leg": leg, "options": eng.options(), "calls": calls, "launch_counts": eng.launch_counts()}), flush=True)
    sys.exit(0)
def kernels(tag):
    out = {}
    for kn in ("qkv", "ffn1", "ffn2"):
        eng.bench_kernel(kn, n_rows=1, iters=8)
        ms = min(eng.bench_kernel(kn, n_rows=1, iters=64)[0] for _ in range(3))
        out[kn] = round(ms * 1e3, 2)
    print(json.dumps({"isolated_us": out, "state": tag, "options": eng.options()}), flush=True)
for v in (0, 5):
    eng.set_option("w8", v)
    kernels(f"w8={v}")
for r in range(reps):
    for spec in specs:
        if not spec:
            continue
        t0 = time.time()
        res = bench.ab_block(eng, one_step, spec, pairs)
        res["rep"] = r
        res["wall_s"] = round(time.time() - t0, 1)
        print(json.dumps(res), flush=True)
