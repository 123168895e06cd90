"""-m gpu: the K/V rows that DECODE steps write, at every decode position, against the float64 oracle (tests/decode_rows_cases.py,
DESIGN §5): what becomes of rows_attn_k's partials in the out-projection's merging prologues (slabs; finished rows at 2 / 4 / 8 splits,
fp32 and bf16 partials), of the normalised rows of unsplit launches, and of the QKV epilogue's cache write, from a short prompt until
the cache is full - every form past the first refill of its attention split.

fp32 rows are held to 16 times the fp32 oracle's own distance from the float64 oracle (a few 1e-5: one ignored position moves a row by
more than four such bars, tests/test_decode_rows_cpu.py).  bf16 rows are held to the project's 2e-2 relative L2 per row: that sees a
wrong slot, a missing partial or a stale row, NOT one position - the position-level evidence for bf16 is tests/test_gpu_decode_attn.py."""
import numpy as np
import pytest
import torch

import decode_rows_cases as dr

pytestmark = pytest.mark.gpu


# bf16 finished-row steps with a split attention hand their partials over in bf16 (option att_p16, the default) or in fp32: both
ARMS = [(dtype, rows, 1) for dtype, rows in dr.CASES] + \
       [("bf16", rows, 0) for rows, (form, nsplit) in dr.PLAN.items() if form == dr.FORM_FR and nsplit > 1]


@pytest.mark.parametrize("dtype,rows,att_p16", ARMS)
def test_every_decode_row_of_a_call_that_fills_its_cache(dtype, rows, att_p16):
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sd = dr.model()
    xs, ys, forced, P = dr.inputs(dtype, rows)
    n, S_max, (form, nsplit) = forced.shape[0], dr.max_positions(dtype, rows), dr.PLAN[rows]
    assert dr.plan(dtype, rows) == (form, nsplit)
    ref = dr.reference(dtype, rows)
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype=dtype, max_seqs=rows, max_positions=S_max, use_graph=False)
    eng.set_option("att_p16", att_p16)
    kn = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=3)
    c0 = eng.launch_counts()
    if rows == 1:
        x, y = xs[0].unsqueeze(0), ys[0].unsqueeze(0)
        eng.inference_tts(x.cuda(), torch.tensor([x.shape[1]]).cuda(), y.cuda(), **kn, _forced=forced[:, 0], _seed=1)
    else:
        eng.inference_tts_multi(xs, ys, **kn, _forced=forced, _seed=1)
    c1 = eng.launch_counts()
    c = {k: c1[k] - c0[k] for k in c1}
    assert eng.last_steps == n, (eng.last_steps, n)
    # the eager loop counts every launch: the attention once per layer and decode step, and the step's form
    L, fr, wide = dr.LAYERS, c["rows_gemm_fr"] + c["rows_gemm_frp"], c["mt2"] + c["mt4"] + c["wd"]
    assert c["rows_attn"] >= L * (n - 1) and c["tile_attn"] == L, c
    if "|fr=0," not in eng.options():
        if form == dr.FORM_SLAB:
            assert fr == 0 and wide == 0 and c["rows_gemm"] + c["row_gemm_fr1"] > 0, c
        elif form == dr.FORM_FR:
            assert fr >= 2 * L * (n - 1) and wide == 0, c
        else:
            assert wide > 0 and fr == 0, c
    H, hd = a.nhead, a.d_model // a.nhead
    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    worst = {}
    for l in range(1, L):
        for key in ("k", "v"):
            t = eng.debug_read(f"{key}cache{l}", (rows, H, S_max, hd), dtype=tdt).float().numpy()
            for u in range(rows):
                last = P[u] + n - 1                    # decode positions P[u] .. last - 1; the call wrote nothing beyond
                got = t[u, :, P[u]:last].transpose(1, 0, 2).reshape(last - P[u], a.d_model)
                want = ref["kv"][u][key][l][P[u]:last]
                err = dr.row_abs(got, want) if dtype == "fp32" else dr.row_rel(got, want)
                i = int(err.argmax())
                if err[i] > worst.get((key, l), (0.0,))[0]:
                    worst[(key, l)] = (float(err[i]), u, P[u] + i)
    bar = ref["bar"] if dtype == "fp32" else dr.BAR_BF16
    print(f"\n{dtype} {rows} rows att_p16 {att_p16} (form {form}, {nsplit} splits, {n} steps to position {max(P) + n - 2} of {S_max}): worst row (figure, sequence, "
          f"position) {worst}; bar {bar:.3g}" + (f" = 16 x the fp32 oracle's {ref['oracle_err']:.3g}" if dtype == "fp32" else ""))
    assert max(v[0] for v in worst.values()) <= bar, (worst, bar)
