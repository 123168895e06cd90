"""-m gpu: decode steps at the model widths that are no power of two against the float64 oracle (tests/odd_width_cases.py):
d = 768 / 1280 / 1536 / 1792 with 10 .. 56 heads, at every row count at which vc_debug_plan changes its mind, in both dtypes.  Each case
is one teacher-forced call of 12 steps; K and V of layer 1 are read back at EVERY position the call wrote, prompt and decode, and the
head logits of EVERY step, and each row is held to the case's bars: in fp32 16 times the fp32 oracle's own distance from the float64
oracle over the same sequences (about 2e-5 for K/V rows and 1e-5 for logits rows) and the arg-max of every codebook, in bf16 the
project's 2e-2 relative L2 per row.  The launch census must show the form the plan names.  One engine per (preset, dtype) serves that
pair's cases, and one engine is alive at a time.  Measured (profiles/odd_widths_pytest_gpu.log): the engine's worst fp32 K/V row lies
2.9 .. 5.0 times the fp32 oracle's own distance out, its worst logits row 0.7 .. 1.2 times; bf16 rows within 3.7e-3."""
import gc

import pytest
import torch

import odd_width_cases as ow

pytestmark = pytest.mark.gpu

# bf16 finished-row steps with a split attention hand their partials over in bf16 (option att_p16, the default) or in fp32: both
ARMS = [(preset, dtype, rows, 1) for preset, dtype, rows in ow.CASES] + \
       [(preset, dtype, rows, 0) for preset, dtype, rows in ow.CASES
        if dtype == "bf16" and ow.PLAN[(preset, dtype)][rows][0] == ow.FORM_FR and ow.PLAN[(preset, dtype)][rows][1] > 1]
ARMS.sort(key=lambda arm: (ow.PRESETS.index(arm[0]), ow.DTYPES.index(arm[1])))          # stable: the cases of an engine stay together

_ENGINE = {}


def _engine(preset, dtype):
    """The engine of (preset, dtype), created when its first case runs; the one before it is released first."""
    if (preset, dtype) not in _ENGINE:
        _ENGINE.clear()
        gc.collect()
        torch.cuda.empty_cache()
        from voicecraft_amd.engine import VoiceCraftEngine
        a, sd = ow.model(preset)
        _ENGINE[(preset, dtype)] = VoiceCraftEngine(a, sd, device="cuda:0", dtype=dtype, max_seqs=ow.MAX_SEQS, max_positions=ow.MAX_POSITIONS,
                                                    use_graph=False)
    return _ENGINE[(preset, dtype)]


@pytest.mark.parametrize("preset,dtype,rows,att_p16", ARMS)
def test_every_row_of_a_decode_call_at_an_odd_width(preset, dtype, rows, att_p16):
    a, _ = ow.model(preset)
    xs, ys, forced, P = ow.inputs(preset)
    form, nsplit = ow.PLAN[(preset, dtype)][rows]
    vec = ow.plan_vector(preset, dtype, rows)
    assert (vec[1], vec[2]) == (form, nsplit), vec
    eng = _engine(preset, dtype)
    eng.set_option("att_p16", att_p16)
    n, L, H, hd = ow.N_STEPS, a.num_decoder_layers, a.nhead, a.d_model // a.nhead
    kn = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=3)
    c0 = eng.launch_counts()
    if rows == 1:
        x, y = xs[0].unsqueeze(0), ys[0].unsqueeze(0)
        lg = eng.inference_tts(x.cuda(), torch.tensor([x.shape[1]]).cuda(), y.cuda(), **kn, _forced=forced[:, 0].copy(), _logit_steps=n, _seed=1)[2]
        lg = lg.cpu().numpy()[:, None]
    else:
        lg = eng.inference_tts_multi(xs[:rows], ys[:rows], **kn, _forced=forced[:, :rows].copy(), _logit_steps=n, _seed=1)[1].cpu().numpy()
    c1 = eng.launch_counts()
    c = {k: c1[k] - c0[k] for k in c1}
    assert eng.last_steps == n and lg.shape[:2] == (n, rows), (eng.last_steps, lg.shape)
    # the eager loop counts every launch: the attention once per layer and decode step, and the step's form
    fr, frp, wide = c["rows_gemm_fr"], c["rows_gemm_frp"], c["mt2"] + c["mt4"]
    census = {k: v for k, v in c.items() if v}
    assert c["rows_attn"] >= L * (n - 1), census
    if form == ow.FORM_SLAB:
        assert fr == 0 and wide == 0 and c["rows_gemm"] + c["row_gemm_fr1"] > 0, census
        if rows == 1:
            assert c["row_gemm_fr1"] >= L * (n - 1), census
    elif form == ow.FORM_FR:
        assert fr >= 2 * L * (n - 1) and wide == 0 and frp == 0 and c["rows_gemm_qp"] == 0, census      # no paired form at these widths
    else:
        assert wide > 0 and fr == 0 and c["wd"] == 0, census                 # rows_gemm_mt_k, not rows_gemm_wd_k
    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    got = {}
    for key in ("k", "v"):
        t = eng.debug_read(f"{key}cache1", (ow.MAX_SEQS, H, ow.MAX_POSITIONS, hd), dtype=tdt).float().numpy()
        got[key] = [t[u, :, : ow.positions(preset, u)].transpose(1, 0, 2).reshape(-1, a.d_model) for u in range(rows)]      # head-major rows
    fails, rep = ow.check_case(preset, dtype, rows, got["k"], got["v"], [lg[:, u] for u in range(rows)])
    own = f"; 16 x the fp32 oracle's {rep['oracle_kv']:.3g} / {rep['oracle_lg']:.3g}: the engine's worst is {rep['worst']['k'][0] / rep['oracle_kv']:.2f} / " \
          f"{rep['worst']['v'][0] / rep['oracle_kv']:.2f} / {rep['worst']['logits'][0] / rep['oracle_lg']:.2f} x the oracle's own, arg-max exceptions " \
          f"{rep['argmax_exceptions']}, misses {rep['argmax_misses']}" if dtype == "fp32" else ""
    print(f"\n{preset} {dtype} {rows} rows att_p16 {att_p16} (form {form}, {nsplit} splits): worst row (figure, sequence, position / step) "
          f"{({k: (float(f'{v[0]:.3g}'),) + v[1:] for k, v in rep['worst'].items()})}; bars K/V {rep['bar_kv']:.3g}, logits {rep['bar_lg']:.3g}{own}; census {census}")
    assert fails == [], (fails[:8], rep)
