"""In-process A/Bs of option `w13` on ONE engine (giga830M, bf16, one utterance: bench.py's headline workload), with bench.py's own
`ab_block` (interleaved pairs of whole calls, its rule for a default) - what `bench.py --full --ab w13=A:B` reports as `ab`, without
paying the engine's creation and the rest of `--full` once per spec.  First the isolated launch times of the three big matrices
(vc_bench_kernel) with the option off and on.  JSON lines on stdout.
usage: python tools/w13_ab.py w13=0:5,w13=0:1,w13=0:4 [runs of each = 1] [pairs = 7]     (profiles/w13_ab.log: 2 runs, 7 pairs)
With VC_ENGINE_LIB naming a library that has no such option (the parent commit's), and an empty spec list, only the launch times."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench

specs = sys.argv[1].split(",")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 7
wl = bench.Workload("giga830M", "tts", 1, 80, 150, 40, "bf16", "cuda:0")
eng = wl.eng
print(json.dumps({"lib": os.path.basename(os.environ.get("VC_ENGINE_LIB", "")) or "default", "options": eng.options(),
                  "w13_layer0": eng.w13_stats()[0] if hasattr(eng, "w13_stats") and "w13" in eng.options() else None}), flush=True)
one_step = lambda seed: wl.call(seed)[1]
for w in range(2):
    one_step(100 + w)
torch.cuda.synchronize()
def kernels(tag):
    out = {}
    for kn in ("qkv", "ffn1", "ffn2"):
        eng.bench_kernel(kn, n_rows=1, iters=8)
        ms = min(eng.bench_kernel(kn, n_rows=1, iters=64)[0] for _ in range(3))
        out[kn] = round(ms * 1e3, 2)
    print(json.dumps({"isolated_us": out, "state": tag, "options": eng.options()}), flush=True)
if "w13" in eng.options():
    for v in (0, 5):
        eng.set_option("w13", v)
        kernels(f"w13={v}")
else:
    kernels("parent")
for r in range(reps):
    for spec in specs:
        if not spec:
            continue
        t0 = time.time()
        res = bench.ab_block(eng, one_step, spec, pairs)
        res["rep"] = r
        res["wall_s"] = round(time.time() - t0, 1)
        print(json.dumps(res), flush=True)
